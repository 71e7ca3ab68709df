// temporal_measured_veneer_check.cpp -- the reference's interactive loop (apps/src/main.cpp:221-271) through the C++ veneer with the
// history (denoiseTemporal()), batch means (momentsBatch() = K) and the measured variance (denoiseMeasured()) all on, which makes
// GPUdenoise ptx_denoise_temporal_measured: on every camera change pathtraceFree(); pathtraceInit(scene) (which starts the moments
// again); then pathtrace x ITERS (one batch after every K-th call), GPUdenoise().  Frame f's camera is the scene's after runOrbitScript
// of f - 1 steps "left:DX,0".  Writes OUT.fN.output (W*H*3 floats of state.output) per frame for tests/test_gpu_temporal_measured.py.
//   temporal_measured_veneer_check SCENE W H DEPTH ITERS K FRAMES DX OUT
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
    denoiseTemporal() = true;
    denoiseMeasured() = true;
    const size_t n = (size_t)w * h;
    std::string script;
    for (int f = 1; f <= frames; f++) {
        if (f > 1) script += step;
        scene->state.camera = base;
        if (!scene->runOrbitScript(script)) return 1;
        pathtraceFree();                               // main.cpp: camchanged -> iteration = 0, pathtraceFree(); pathtraceInit(scene)
        pathtraceInit(scene);
        for (int it = 1; it <= iters; it++) pathtrace(nullptr, 0, it);
        GPUdenoise();
        ptx_moments_summary sum;
        if (ptx_moments_summarize(pathtraceMoments(), nullptr, &sum) != PTX_OK || sum.batches != iters / k || sum.samples != iters / k * k) {
            fprintf(stderr, "moments: %s (batches %d, samples %lld)\n", ptx_last_error(), (int)sum.batches, (long long)sum.samples);
            return 1;
        }
        dump(out + ".f" + std::to_string(f) + ".output", scene->state.output.data(), n * 12);
    }
    GPUdenoiseRelease();
    pathtraceFree();
    delete scene;
    printf("temporal measured veneer ok\n");
    return 0;
}
