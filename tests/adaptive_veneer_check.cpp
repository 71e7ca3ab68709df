// adaptive_veneer_check.cpp -- the reference's interactive loop (apps/src/main.cpp:221-271) through the C++ veneer with adaptive sampling
// on (momentsBatch() = K, adaptiveTarget() = E): on every camera change pathtraceFree(); pathtraceInit(scene); then pathtrace x ITERS
// (one round of ptx_adaptive_add + ptx_adaptive_select after every K-th call), adaptiveFrame().  Frame f's camera is the scene's after
// runOrbitScript of f - 1 steps "left:DX,0".  Writes OUT.fN.frame (W*H*3 floats, the resolved frame), OUT.fN.samples (W*H int32) and
// OUT.fN.status (the last round's ptx_adaptive_status) per frame for tests/test_gpu_adaptive.py.
//   adaptive_veneer_check SCENE W H DEPTH ITERS K FRAMES DX E OUT
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
    if (argc < 11) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]), depth = atoi(argv[4]), iters = atoi(argv[5]), k = atoi(argv[6]), frames = atoi(argv[7]);
    const std::string step = std::string(";left:") + argv[8] + ",0", out = argv[10];
    Scene *scene = new Scene(argv[1]);
    scene->setResolution(w, h);
    scene->state.traceDepth = depth;
    const Camera base = scene->state.camera;
    if (adaptiveTarget() != 0.f || pathtraceAdaptive()) return 1;      // off by default
    momentsBatch() = k;
    adaptiveTarget() = (float)atof(argv[9]);
    const size_t n = (size_t)w * h;
    std::vector<int32_t> samples(n);
    std::string script;
    for (int f = 1; f <= frames; f++) {
        if (f > 1) script += step;
        scene->state.camera = base;
        if (!scene->runOrbitScript(script)) return 1;
        pathtraceFree();                               // main.cpp: camchanged -> iteration = 0, pathtraceFree(); pathtraceInit(scene)
        pathtraceInit(scene);
        if (adaptiveStatus().rounds != 0) return 1;    // pathtraceInit starts the frame over
        for (int it = 1; it <= iters; it++) pathtrace(nullptr, 0, it);
        const float *frame = adaptiveFrame();
        const ptx_adaptive_status st = adaptiveStatus();
        if (!frame || st.rounds != iters / k || ptx_adaptive_read(pathtraceAdaptive(), nullptr, samples.data(), nullptr, nullptr) != PTX_OK) {
            fprintf(stderr, "adaptive: %s (rounds %d)\n", ptx_last_error(), (int)st.rounds);
            return 1;
        }
        dump(out + ".f" + std::to_string(f) + ".frame", frame, n * 12);
        dump(out + ".f" + std::to_string(f) + ".samples", samples.data(), n * 4);
        dump(out + ".f" + std::to_string(f) + ".status", &st, sizeof st);
    }
    GPUdenoiseRelease();
    pathtraceFree();
    delete scene;
    printf("adaptive veneer ok\n");
    return 0;
}
