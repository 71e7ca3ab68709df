// oidn_veneer_check.cpp -- the reference's CPUdenoise() (apps/src/main.cpp:167-219) as a caller of csrc/oidn_api.h would write it:
// newDevice, getError, setErrorFunction, commit, newFilter("RT"), setImage x 3, commit, execute -- on files tests/test_gpu_nn_image.py
// wrote: DIR holds rt_ldr_alb.tza, rt_alb.tza and rt_hdr_alb.tza (synthetic), IN.color and IN.albedo are W*H*3 floats.
//   oidn_veneer_check DIR W H IN OUT
// Writes OUT.ldr (the sequence as written), OUT.moved (after a commit that only moved the colour pointer), OUT.small (after a size
// change: the left W - 1 columns, read through a row stride), OUT.alb (albedo alone: rt_alb), OUT.hdr and OUT.scale (hdr, automatic
// scale), and checks the build counts and the two refusals itself.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../mygpuraytracer_amd/csrc/oidn_api.h"

using namespace oidn;

static int g_errors = 0;
static void count_error(void *user, Error code, const char *message) {
    (void)user; (void)code;
    g_errors++;
    fprintf(stderr, "error function: %s\n", message);
}

static std::vector<float> slurp(const std::string &path, size_t count) {
    std::vector<float> v(count);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f || fread(v.data(), sizeof(float), count, f) != count) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
    fclose(f);
    return v;
}

static void dump(const std::string &path, const void *p, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const int width = atoi(argv[2]), height = atoi(argv[3]);
    const std::string in = argv[4], out = argv[5];
    const size_t n = (size_t)width * height * 3;
    std::vector<float> color = slurp(in + ".color", n), albedo = slurp(in + ".albedo", n), output(n, -7.f);
    setWeightsDirectory(argv[1]);

    DeviceRef device = newDevice(DeviceType::Default);
    const char *errorMessage;
    EXPECT(device.getError(errorMessage) == Error::None);
    device.setErrorFunction(count_error);
    device.commit();
    FilterRef filter = device.newFilter("RT");
    filter.setImage("color", color.data(), Format::Float3, width, height);
    filter.setImage("albedo", albedo.data(), Format::Float3, width, height);
    filter.setImage("output", output.data(), Format::Float3, width, height);
    filter.commit();
    filter.execute();
    EXPECT(device.getError(errorMessage) == Error::None && g_errors == 0);
    EXPECT(filter.get<int>("networkBuilds") == 1 && filter.get<int>("alignment") == 16 && filter.get<int>("overlap") == 96);
    EXPECT(filter.get<int>("maxMemoryMB") == 3000 && !filter.get<bool>("hdr"));
    dump(out + ".ldr", output.data(), n * sizeof(float));

    // only a pointer moves: the network stays
    std::vector<float> moved(color);
    std::fill(output.begin(), output.end(), -7.f);
    filter.setImage("color", moved.data(), Format::Float3, width, height);
    filter.execute();                                  // (not committed: refused)
    EXPECT(device.getError(errorMessage) == Error::InvalidOperation && g_errors == 1);
    filter.commit();
    filter.execute();
    EXPECT(device.getError() == Error::None && filter.get<int>("networkBuilds") == 1);
    dump(out + ".moved", output.data(), n * sizeof(float));

    // another size: a new network.  The left W - 1 columns of the same buffers, through their row stride.
    if (width > 1) {
        const size_t row = (size_t)width * 3 * sizeof(float);
        std::vector<float> small((size_t)(width - 1) * height * 3, -7.f);
        filter.setImage("color", color.data(), Format::Float3, width - 1, height, 0, 0, row);
        filter.setImage("albedo", albedo.data(), Format::Float3, width - 1, height, 0, 0, row);
        filter.setImage("output", small.data(), Format::Float3, width - 1, height);
        filter.commit();
        filter.execute();
        EXPECT(device.getError() == Error::None && filter.get<int>("networkBuilds") == 2);
        dump(out + ".small", small.data(), small.size() * sizeof(float));
    }

    {   // albedo alone: rt_alb, the prefilter's albedo role
        FilterRef aux = device.newFilter("RT");
        std::fill(output.begin(), output.end(), -7.f);
        aux.setImage("albedo", albedo.data(), Format::Float3, width, height);
        aux.setImage("output", output.data(), Format::Float3, width, height);
        aux.commit();
        aux.execute();
        EXPECT(device.getError() == Error::None && aux.get<int>("networkBuilds") == 1);
        dump(out + ".alb", output.data(), n * sizeof(float));
        aux.set("hdr", true);
        aux.commit();
        EXPECT(device.getError(errorMessage) == Error::InvalidOperation && strstr(errorMessage, "albedo filtering"));
    }
    {   // hdr with the automatic scale: rt_hdr_alb
        FilterRef hdr = device.newFilter("RT");
        std::fill(output.begin(), output.end(), -7.f);
        hdr.setImage("color", color.data(), Format::Float3, width, height);
        hdr.setImage("albedo", albedo.data(), Format::Float3, width, height);
        hdr.setImage("output", output.data(), Format::Float3, width, height);
        hdr.set("hdr", true);
        hdr.commit();
        hdr.execute();
        EXPECT(device.getError() == Error::None);
        const float scale = hdr.get<float>("scale");
        dump(out + ".hdr", output.data(), n * sizeof(float));
        dump(out + ".scale", &scale, sizeof scale);
        FilterRef copy = hdr;                          // handles are shared references
        EXPECT(copy.get<bool>("hdr") && copy.getHandle() == hdr.getHandle());
    }
    {   // no such weight file; no such filter
        const int before = g_errors;
        FilterRef alone = device.newFilter("RT");
        alone.setImage("color", color.data(), Format::Float3, width, height);
        alone.setImage("output", output.data(), Format::Float3, width, height);
        alone.commit();
        EXPECT(device.getError(errorMessage) == Error::InvalidOperation && strstr(errorMessage, "rt_ldr.tza"));
        FilterRef lightmap = device.newFilter("RTLightmap");
        EXPECT(!lightmap && device.getError() == Error::InvalidArgument && device.getError() == Error::None);
        EXPECT(g_errors == before + 2);
    }
    printf("oidn veneer ok\n");
    return 0;
}
