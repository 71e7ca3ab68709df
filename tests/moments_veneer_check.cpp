// moments_veneer_check.cpp -- the reference's interactive loop (apps/src/main.cpp:221-271) through the C++ veneer with batch means on
// (momentsBatch() = K) and the filter on the measured variance (denoiseMeasured()): on every camera change pathtraceFree();
// pathtraceInit(scene); then pathtrace x ITERS (one batch after every K-th call), GPUdenoise().  Frame f's camera is the scene's after
// runOrbitScript of f - 1 steps "left:DX,0".  Writes OUT.fN.output (W*H*3 floats of state.output), OUT.fN.mean (W*H*3) and OUT.fN.cov
// (W*H*6) per frame for tests/test_gpu_moments.py.
//   moments_veneer_check SCENE W H DEPTH ITERS K FRAMES DX OUT
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
    const int w = atoi(argv[2]), h = atoi(argv[3]), depth = atoi(argv[4]), iters = atoi(argv[5]), k = atoi(argv[6]), frames = atoi(argv[7]);
    const std::string step = std::string(";left:") + argv[8] + ",0", out = argv[9];
    Scene *scene = new Scene(argv[1]);
    scene->setResolution(w, h);
    scene->state.traceDepth = depth;
    const Camera base = scene->state.camera;
    momentsBatch() = k;
    denoiseMeasured() = true;
    const size_t n = (size_t)w * h;
    std::vector<float> mean(n * 3), cov(n * 6);
    std::string script;
    for (int f = 1; f <= frames; f++) {
        if (f > 1) script += step;
        scene->state.camera = base;
        if (!scene->runOrbitScript(script)) return 1;
        pathtraceFree();                               // main.cpp: camchanged -> iteration = 0, pathtraceFree(); pathtraceInit(scene)
        pathtraceInit(scene);
        for (int it = 1; it <= iters; it++) pathtrace(nullptr, 0, it);
        GPUdenoise();
        int64_t samples = 0;
        if (ptx_moments_read(pathtraceMoments(), mean.data(), cov.data(), nullptr, &samples) != PTX_OK || samples != iters / k * k) {
            fprintf(stderr, "moments: %s (samples %lld)\n", ptx_last_error(), (long long)samples);
            return 1;
        }
        dump(out + ".f" + std::to_string(f) + ".output", scene->state.output.data(), n * 12);
        dump(out + ".f" + std::to_string(f) + ".mean", mean.data(), n * 12);
        dump(out + ".f" + std::to_string(f) + ".cov", cov.data(), n * 24);
    }
    GPUdenoiseRelease();
    pathtraceFree();
    delete scene;
    printf("moments veneer ok\n");
    return 0;
}
