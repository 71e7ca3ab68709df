// denoise_veneer_check.cpp -- the port of apps/src/main.cpp's `CPUdenoise(); sendToGPU(pbo, iteration);` through the C++ veneer:
// pathtraceInit, pathtrace x ITERS, GPUdenoise() (state.output), sendToGPU into a device pbo, then GPUdenoise(true) + sendToGPU straight
// from the device.  Writes OUT.output (W*H*3 floats), OUT.pbo and OUT.pbo_dev (W*H*4 bytes) for tests/test_gpu_denoise.py.
//   denoise_veneer_check SCENE W H DEPTH ITERS OUT
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../mygpuraytracer_amd/csrc/pathtrace_api.h"

static void dump(const std::string &path, const void *p, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(1); }
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
    pathtraceInit(scene);
    const size_t n = (size_t)w * h;
    uchar4 *pbo = nullptr;
    if (hipMalloc((void **)&pbo, n * 4) != hipSuccess || hipMemset(pbo, 0x5a, n * 4) != hipSuccess) { fprintf(stderr, "no device pbo\n"); return 1; }
    for (int it = 1; it <= iters; it++) pathtrace(pbo, 0, it);
    std::vector<unsigned char> host(n * 4);
    GPUdenoise();                                      // CPUdenoise's place: state.output = denoised state.image / iters
    sendToGPU(pbo, iters);
    if (hipMemcpy(host.data(), pbo, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    dump(out + ".output", scene->state.output.data(), n * 12);
    dump(out + ".pbo", host.data(), n * 4);
    if (hipMemset(pbo, 0x5a, n * 4) != hipSuccess) return 1;
    GPUdenoise(true);                                  // the result stays on the device and sendToGPU takes it from there
    sendToGPU(pbo, iters);
    if (hipMemcpy(host.data(), pbo, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    dump(out + ".pbo_dev", host.data(), n * 4);
    (void)hipFree(pbo);
    pathtraceFree();
    delete scene;
    printf("denoise veneer ok\n");
    return 0;
}
