// display_veneer_check.cpp -- the veneer's preview with displayTransform() off and on: pathtraceInit, ITERS x pathtrace(pbo, 0, it) with
// the switch off (OUT.off.preview), GPUdenoise(true) + sendToGPU (OUT.off.denoised); then the switch on: one more pathtrace
// (OUT.on.preview), GPUdenoise(true) + sendToGPU (OUT.on.denoised), GPUdenoise() + sendToGPU from the host frame (OUT.on.host).  Every
// file is the pbo's W*H*4 bytes, for tests/test_gpu_display.py.  (pathtrace_raw / sendToGPU_raw are what pathtrace / sendToGPU run: this
// unit holds its pbo as a plain device pointer.)
//   display_veneer_check SCENE W H DEPTH ITERS OUT
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../mygpuraytracer_amd/csrc/pathtrace_api.h"

static void dump_pbo(const std::string &path, const void *pbo, size_t n) {
    std::vector<unsigned char> host(n);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host.data(), pbo, n, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "pbo read failed\n"); exit(1); }
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(host.data(), 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(1); }
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc < 7) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]), depth = atoi(argv[4]), iters = atoi(argv[5]);
    const std::string out = argv[6];
    Scene *scene = new Scene(argv[1]);
    scene->setResolution(w, h);
    scene->state.traceDepth = depth;
    scene->applyRunCudaCamera();
    if (displayTransform()) return 1;                  // off by default
    const size_t bytes = (size_t)w * h * 4;
    void *pbo = nullptr;
    pathtraceFree();
    pathtraceInit(scene);
    if (hipMalloc(&pbo, bytes) != hipSuccess) return 1;
    for (int it = 1; it <= iters; it++) mi355x::pathtrace_raw(pbo, 0, it);
    dump_pbo(out + ".off.preview", pbo, bytes);
    GPUdenoise(true);
    mi355x::sendToGPU_raw(pbo, iters);
    dump_pbo(out + ".off.denoised", pbo, bytes);
    if (displayStatus().frames != 0) return 1;         // nothing was metered: no handle exists

    displayTransform() = true;
    pathtrace(nullptr, 0, iters + 1);                  // no pbo: nothing written, nothing metered
    if (displayStatus().frames != 0) return 1;
    mi355x::pathtrace_raw(pbo, 0, iters + 2);
    dump_pbo(out + ".on.preview", pbo, bytes);
    if (displayStatus().frames != 1 || !(displayStatus().applied > 0.f)) return 1;
    GPUdenoise(true);
    mi355x::sendToGPU_raw(pbo, iters + 2);
    dump_pbo(out + ".on.denoised", pbo, bytes);
    GPUdenoise();
    mi355x::sendToGPU_raw(pbo, iters + 2);
    dump_pbo(out + ".on.host", pbo, bytes);
    if (displayStatus().frames != 3) return 1;
    pathtraceFree();                                   // a camera change does not reset the display handle
    pathtraceInit(scene);
    if (displayStatus().frames != 3) return 1;
    (void)hipFree(pbo);
    GPUdenoiseRelease();
    if (displayStatus().frames != 0) return 1;
    pathtraceFree();
    delete scene;
    printf("display veneer ok\n");
    return 0;
}
