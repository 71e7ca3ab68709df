// adaptive_denoise_veneer_check.cpp -- adaptive_veneer_check.cpp's loop with the filter on (adaptiveDenoise() = true): on every camera
// change pathtraceFree(); pathtraceInit(scene); then pathtrace x ITERS (one round of ptx_adaptive_add + ptx_adaptive_select after every
// K-th call), adaptiveDenoisedFrame().  Frame f's camera is the scene's after runOrbitScript of f - 1 steps "left:DX,0".  Writes
// OUT.fN.denoised (W*H*3 floats, ptx_denoise_adaptive's frame) and OUT.fN.frame (the resolved frame the call leaves in the handle) per
// frame for tests/test_gpu_adaptive_denoise.py.
//   adaptive_denoise_veneer_check SCENE W H DEPTH ITERS K FRAMES DX E OUT
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
    if (adaptiveDenoise() || adaptiveDenoisedFrame()) return 1;        // off by default
    momentsBatch() = k;
    adaptiveTarget() = (float)atof(argv[9]);
    const size_t n = (size_t)w * h;
    std::vector<float> frame(n * 3);
    std::string script;
    for (int f = 1; f <= frames; f++) {
        if (f > 1) script += step;
        scene->state.camera = base;
        if (!scene->runOrbitScript(script)) return 1;
        pathtraceFree();                               // main.cpp: camchanged -> iteration = 0, pathtraceFree(); pathtraceInit(scene)
        pathtraceInit(scene);
        adaptiveDenoise() = true;
        if (adaptiveDenoisedFrame()) return 1;         // no round yet
        for (int it = 1; it <= iters; it++) pathtrace(nullptr, 0, it);
        adaptiveDenoise() = false;
        if (adaptiveDenoisedFrame()) return 1;         // the switch is off: nothing is filtered
        adaptiveDenoise() = true;
        const float *den = adaptiveDenoisedFrame();
        if (!den || adaptiveStatus().rounds != iters / k || ptx_adaptive_read(pathtraceAdaptive(), frame.data(), nullptr, nullptr, nullptr) != PTX_OK) {
            fprintf(stderr, "adaptive denoise: %s (rounds %d)\n", ptx_last_error(), (int)adaptiveStatus().rounds);
            return 1;
        }
        dump(out + ".f" + std::to_string(f) + ".denoised", den, n * 12);
        dump(out + ".f" + std::to_string(f) + ".frame", frame.data(), n * 12);
    }
    GPUdenoiseRelease();
    pathtraceFree();
    delete scene;
    printf("adaptive denoise veneer ok\n");
    return 0;
}
