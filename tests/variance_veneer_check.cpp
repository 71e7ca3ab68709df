// variance_veneer_check.cpp -- the reference's interactive loop (apps/src/main.cpp:221-271) through the C++ veneer with the variance-guided
// filter on (denoiseVariance()), with temporal reuse (TEMPORAL = 1) or without (0):
// on every camera change pathtraceFree(); pathtraceInit(scene); then pathtrace x ITERS, GPUdenoise(), sendToGPU.  Frame f's camera is the
// scene's after runOrbitScript of f - 1 steps "left:DX,0" (the headless driver's --frames).  Writes OUT.fN.output (W*H*3 floats of
// state.output) and OUT.fN.pbo (W*H*4 bytes) per frame for tests/test_gpu_variance.py.
//   variance_veneer_check SCENE W H DEPTH ITERS FRAMES DX OUT TEMPORAL
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
    if (argc < 10) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]), depth = atoi(argv[4]), iters = atoi(argv[5]), frames = atoi(argv[6]);
    const std::string step = std::string(";left:") + argv[7] + ",0", out = argv[8];
    Scene *scene = new Scene(argv[1]);
    scene->setResolution(w, h);
    scene->state.traceDepth = depth;
    const Camera base = scene->state.camera;
    denoiseTemporal() = atoi(argv[9]) != 0;
    denoiseVariance() = true;
    const size_t n = (size_t)w * h;
    uchar4 *pbo = nullptr;
    if (hipMalloc((void **)&pbo, n * 4) != hipSuccess) { fprintf(stderr, "no device pbo\n"); return 1; }
    std::vector<unsigned char> host(n * 4);
    std::string script;
    for (int f = 1; f <= frames; f++) {
        if (f > 1) script += step;
        scene->state.camera = base;
        if (!scene->runOrbitScript(script)) return 1;
        pathtraceFree();                               // main.cpp: camchanged -> iteration = 0, pathtraceFree(); pathtraceInit(scene)
        pathtraceInit(scene);
        for (int it = 1; it <= iters; it++) pathtrace(pbo, 0, it);
        GPUdenoise();
        sendToGPU(pbo, iters);
        if (hipMemcpy(host.data(), pbo, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
        dump(out + ".f" + std::to_string(f) + ".output", scene->state.output.data(), n * 12);
        dump(out + ".f" + std::to_string(f) + ".pbo", host.data(), n * 4);
    }
    GPUdenoiseRelease();
    (void)hipFree(pbo);
    pathtraceFree();
    delete scene;
    printf("variance veneer ok\n");
    return 0;
}
