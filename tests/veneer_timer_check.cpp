// veneer_timer_check.cpp -- the module timer of the C++ veneer (mygpuraytracer_amd/csrc/pathtrace_api.h) across two lives of the
// module's tracer in one process: pathtraceInit, timer().startGpuTimer(), a few pathtrace() calls, timer().endGpuTimer(),
// pathtraceFree -- twice.  Prints each round's interval for tests/test_gpu_tracer_life.py; exits 0 when both are positive.
//   veneer_timer_check SCENE W H DEPTH ITERS [device=N]
// device=N: the tracer is made on device N while device 0 is the current one at every startGpuTimer.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../mygpuraytracer_amd/csrc/pathtrace_api.h"

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]), depth = atoi(argv[4]), iters = atoi(argv[5]);
    int device = -1;
    if (argc > 6 && std::string(argv[6]).rfind("device=", 0) == 0) device = atoi(argv[6] + 7);
    if (device >= 0) pathtraceDevices().assign(1, device);
    Scene *scene = new Scene(argv[1]);
    scene->setResolution(w, h);
    scene->state.traceDepth = depth;
    scene->applyRunCudaCamera();
    bool ok = true;
    for (int round = 0; round < 2; round++) {
        pathtraceInit(scene);
        if (device >= 0 && hipSetDevice(0) != hipSuccess) { fprintf(stderr, "cannot make device 0 current\n"); return 1; }
        timer().startGpuTimer();
        for (int it = 1; it <= iters; it++) pathtrace(nullptr, 0, it);
        timer().endGpuTimer();
        const float ms = timer().getGpuElapsedTimeForPreviousOperation();      // (the caller's interval: no pathtrace() since its end)
        printf("round %d interval %g\n", round, ms);
        ok = ok && ms > 0.f;
        pathtraceFree();
    }
    delete scene;
    return ok ? 0 : 3;
}
