// guides_veneer_check.cpp -- the sampled guides through the C++ veneer: antialiasing and depth of field on, guideSamples() = K, a batch
// of moments after every pathtrace() call, then GPUdenoise() plain and with denoiseMeasured().  Writes OUT.plain and OUT.measured
// (W*H*3 floats each) for tests/test_gpu_guides.py, which renders the same frames through the C ABI.
//   guides_veneer_check SCENE W H DEPTH ITERS K OUT
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../mygpuraytracer_amd/csrc/pathtrace_api.h"

static void dump(const std::string &path, const void *p, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(1); }
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc < 8) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]), depth = atoi(argv[4]), iters = atoi(argv[5]), k = atoi(argv[6]);
    const std::string out = argv[7];
    Scene *scene = new Scene(argv[1]);
    scene->setResolution(w, h);
    scene->state.traceDepth = depth;
    scene->applyRunCudaCamera();
    pathtraceOptions().antialiasing = 1;
    pathtraceOptions().depth_of_field = 1;
    guideSamples() = k;
    momentsBatch() = 1;
    pathtraceInit(scene);
    for (int it = 1; it <= iters; it++) pathtrace(nullptr, 0, it);
    const size_t n = (size_t)w * h;
    GPUdenoise();
    dump(out + ".plain", scene->state.output.data(), n * 12);
    int first = 0, count = 0;
    if (ptx_get_guide_samples(pathtraceHandle(), &first, &count) != PTX_OK || first != 1 || count != (k < iters ? k : iters)) {
        fprintf(stderr, "the tracer's guide samples are (%d, %d)\n", first, count);
        return 1;
    }
    denoiseVariance() = true;
    denoiseMeasured() = true;
    GPUdenoise();
    dump(out + ".measured", scene->state.output.data(), n * 12);
    GPUdenoiseRelease();
    pathtraceFree();
    delete scene;
    printf("guides veneer ok\n");
    return 0;
}
