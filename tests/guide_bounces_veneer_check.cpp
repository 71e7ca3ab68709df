// guide_bounces_veneer_check.cpp -- the guides through mirrors and glass in the C++ veneer, host only (no device is touched): the
// guideBounces() switch is off by default, is one object and keeps what it is given, next to guideSamples(); and the C ABI it is
// applied through refuses a null tracer by name, reached through the veneer's own header.  tests/test_guide_bounces_cpu.py compiles
// and runs it.
//   guide_bounces_veneer_check
#include <cstdio>
#include <cstring>

#include "../mygpuraytracer_amd/csrc/pathtrace_api.h"

static int fail(const char *what) {
    fprintf(stderr, "guide bounces veneer: %s\n", what);
    return 1;
}

int main() {
    if (guideBounces() != 0) return fail("guideBounces() is not off by default");
    if (guideSamples() != 0) return fail("guideSamples() is not off by default");
    int &b = guideBounces();
    b = 8;
    if (guideBounces() != 8 || &guideBounces() != &b) return fail("guideBounces() is not one object");
    if (guideSamples() != 0) return fail("guideBounces() and guideSamples() share their storage");
    guideBounces() = 0;
    if (ptx_set_guide_bounces(nullptr, 1) != PTX_ERR_INVALID || !strstr(ptx_last_error(), "ptx_set_guide_bounces"))
        return fail("ptx_set_guide_bounces(NULL) is not refused by name");
    int got = -1;
    if (ptx_get_guide_bounces(nullptr, &got) != PTX_ERR_INVALID || got != -1 || !strstr(ptx_last_error(), "ptx_get_guide_bounces"))
        return fail("ptx_get_guide_bounces(NULL) is not refused by name");
    printf("guide bounces veneer ok\n");
    return 0;
}
