// oidn_conformance_check.cpp -- the cases of OIDN's conformance program (its apps/oidnTest.cpp), restated in this project's words against
// csrc/oidn_api.h and run on the GPU by tests/test_gpu_oidn_conformance.py.  Plain main, nothing caught: a veneer call does not throw.
// Compiled with -DOIDN_FILTER_RTLIGHTMAP, so its newDevice offers the lightmap filter.
//   argv: <weights dir> <prefix>.  The directory holds synthetic blobs under OIDN's names (rt_hdr, rt_ldr, rt_hdr_alb, rt_ldr_alb,
//   rt_hdr_alb_nrm, rt_ldr_alb_nrm, rtlightmap_hdr, rtlightmap_dir).  <prefix>.lightmap_in is W*H*3 floats (33 x 17); the two lightmap
//   results go to <prefix>.lightmap_hdr and <prefix>.lightmap_dir for the test to compare with the Python call's bytes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../mygpuraytracer_amd/csrc/oidn_api.h"

using namespace oidn;

static int g_line = 0;
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); g_line = __LINE__; return false; } } while (0)
#define RUN(call) do { if (!(call)) { fprintf(stderr, "failed: %s\n", #call); return 1; } printf("ok: %s\n", #call); fflush(stdout); } while (0)

// an image in memory of a device's buffer, as the reference's ImageBuffer holds one
struct Image {
    BufferRef buffer;
    int w = 0, h = 0;
    Image() {}
    Image(const DeviceRef &device, int w_, int h_, float value = 0.5f) : buffer(device.newBuffer((size_t)w_ * h_ * 3 * sizeof(float))), w(w_), h(h_) {
        for (size_t i = 0; i < size(); i++) data()[i] = value;
    }
    float *data() const { return static_cast<float *>(buffer.getData()); }
    size_t size() const { return (size_t)w * h * 3; }
};

static void set(FilterRef &f, const char *name, const Image &im) { f.setImage(name, im.data(), Format::Float3, im.w, im.h); }
static void set_buffer(FilterRef &f, const char *name, const Image &im) { f.setImage(name, im.buffer, Format::Float3, im.w, im.h); }

static bool between(const Image &im, float a, float b) {
    for (size_t i = 0; i < im.size(); i++) {
        const float x = im.data()[i];
        if (!std::isfinite(x) || x < a || x > b) { fprintf(stderr, "value %zu is %g\n", i, x); return false; }
    }
    return true;
}

static DeviceRef committed_device() {
    DeviceRef device = newDevice();
    device.commit();
    return device;
}

static bool single_filter(int frames, bool through_buffers) {
    const int W = 257, H = 89;
    DeviceRef device = committed_device();
    REQUIRE(device && device.getError() == Error::None);
    FilterRef filter = device.newFilter("RT");
    REQUIRE(bool(filter));
    Image image(device, W, H);
    REQUIRE(image.buffer && image.buffer.getSize() == image.size() * 4);
    if (through_buffers) { set_buffer(filter, "color", image); set_buffer(filter, "output", image); }          // in place
    else { set(filter, "color", image); set(filter, "output", image); }
    filter.commit();
    REQUIRE(device.getError() == Error::None);
    for (int i = 0; i < frames; i++) {
        filter.execute();
        REQUIRE(device.getError() == Error::None);
    }
    REQUIRE(between(image, 0.f, 1.f) && filter.get<int>("networkBuilds") == 1);
    return true;
}

static bool one_filter_at_a_time(const std::vector<int> &sizes) {
    DeviceRef device = committed_device();
    for (const int n : sizes) {
        FilterRef filter = device.newFilter("RT");
        REQUIRE(bool(filter));
        Image image(device, n, n);
        set(filter, "color", image);
        set(filter, "output", image);
        filter.commit();
        REQUIRE(device.getError() == Error::None);
        filter.execute();
        REQUIRE(device.getError() == Error::None && between(image, 0.f, 1.f));
    }
    return true;
}

static bool several_filters(const std::vector<int> &sizes) {
    DeviceRef device = committed_device();
    std::vector<FilterRef> filters;
    std::vector<Image> images;
    for (const int n : sizes) {
        filters.push_back(device.newFilter("RT"));
        REQUIRE(bool(filters.back()));
        images.push_back(Image(device, n, n));
        set(filters.back(), "color", images.back());
        set(filters.back(), "output", images.back());
        filters.back().commit();
        REQUIRE(device.getError() == Error::None);
    }
    for (size_t i = 0; i < filters.size(); i++) {
        filters[i].execute();
        REQUIRE(device.getError() == Error::None && between(images[i], 0.f, 1.f));
    }
    return true;
}

static bool two_devices() {
    const int sizes[2] = {111, 80};
    DeviceRef devices[2];
    FilterRef filters[2];
    Image images[2];
    for (int i = 0; i < 2; i++) {
        devices[i] = committed_device();
        REQUIRE(devices[i] && devices[i].getError() == Error::None);
        filters[i] = devices[i].newFilter("RT");
        images[i] = Image(devices[i], sizes[i], sizes[i]);
        set(filters[i], "color", images[i]);
        set(filters[i], "output", images[i]);
        filters[i].commit();
        REQUIRE(devices[i].getError() == Error::None);
    }
    for (int i = 0; i < 2; i++) {
        filters[i].execute();
        REQUIRE(devices[i].getError() == Error::None && between(images[i], 0.f, 1.f));
    }
    return true;
}

enum Update { NONE, SAME_SIZE, DOUBLED, REMOVE_IMAGE, SET_NULL, HDR_OFF };

static bool filter_update(Update what) {
    const int W = 53, H = 149;
    DeviceRef device = committed_device();
    FilterRef filter = device.newFilter("RT");
    Image color(device, W, H), albedo(device, W, H), output(device, W, H);
    set(filter, "color", color);
    set(filter, "albedo", albedo);
    set(filter, "output", output);
    filter.set("hdr", true);
    filter.commit();
    REQUIRE(device.getError() == Error::None);
    filter.execute();
    REQUIRE(device.getError() == Error::None);
    int builds = 1;
    switch (what) {
    case NONE: break;
    case SAME_SIZE:
        color = Image(device, W, H);
        set(filter, "color", color);
        break;
    case DOUBLED:
        color = Image(device, W * 2, H * 2); albedo = Image(device, W * 2, H * 2); output = Image(device, W * 2, H * 2);
        set(filter, "color", color);
        set(filter, "albedo", albedo);
        set(filter, "output", output);
        builds = 2;
        break;
    case REMOVE_IMAGE: filter.removeImage("albedo"); builds = 2; break;
    case SET_NULL: filter.setImage("albedo", nullptr, Format::Float3, 0, 0); builds = 2; break;
    case HDR_OFF: filter.set("hdr", false); builds = 2; break;                       // another weight file
    }
    filter.commit();
    REQUIRE(device.getError() == Error::None);
    filter.execute();
    REQUIRE(device.getError() == Error::None && filter.get<int>("networkBuilds") == builds);
    REQUIRE(between(output, 0.f, std::numeric_limits<float>::max()));
    return true;
}

static bool image_size(int W, int H) {
    DeviceRef device = committed_device();
    FilterRef filter = device.newFilter("RT");
    const int N = W * H * 3 > 1 ? W * H * 3 : 1;
    std::vector<float> input(N + 2, 0.5f), output(N + 2, -7.f);
    filter.setImage("color", input.data(), Format::Float3, W, H);
    filter.setImage("output", output.data(), Format::Float3, W, H);
    filter.commit();
    REQUIRE(device.getError() == Error::None);
    filter.execute();
    REQUIRE(device.getError() == Error::None);
    for (int i = 0; i < N + 2; i++) REQUIRE((i < W * H * 3) ? (output[i] >= 0.f && output[i] <= 1.f) : output[i] == -7.f);
    return true;
}

static bool sanitization(bool hdr, float value) {
    const int W = 191, H = 47;
    DeviceRef device = committed_device();
    FilterRef filter = device.newFilter("RT");
    Image input(device, W, H, value), output(device, W, H, -7.f);
    set(filter, "color", input);
    set(filter, "albedo", input);
    set(filter, "normal", input);
    set(filter, "output", output);
    filter.set("hdr", hdr);
    filter.commit();
    REQUIRE(device.getError() == Error::None);
    filter.execute();
    REQUIRE(device.getError() == Error::None);
    REQUIRE(between(output, 0.f, hdr ? std::numeric_limits<float>::max() : 1.f));
    return true;
}

struct Progress {
    double n = 0, nMax;
    int calls = 0;
    bool sane = true;
    explicit Progress(double nMax_) : nMax(nMax_) {}
};

static bool on_progress(void *user, double n) {
    Progress *p = static_cast<Progress *>(user);
    if (!(std::isfinite(n) && n >= 0 && n <= 1) || n < p->n) p->sane = false;       // between 0 and 1, never decreasing
    p->n = n;
    p->calls++;
    return n < p->nMax;
}

static bool progress(double nMax, int W, int H, int maxMemoryMB, int least_calls) {
    DeviceRef device = committed_device();
    FilterRef filter = device.newFilter("RT");
    Image image(device, W, H), before(device, W, H);
    set(filter, "color", image);
    set(filter, "output", image);                                                   // in place
    Progress p(nMax);
    filter.setProgressMonitorFunction(on_progress, &p);
    filter.set("maxMemoryMB", maxMemoryMB);
    filter.commit();
    REQUIRE(device.getError() == Error::None);
    filter.execute();
    REQUIRE(p.sane);
    if (nMax <= 1) {
        const char *message = nullptr;
        REQUIRE(device.getError(message) == Error::Cancelled && message && !strcmp(message, "execution was cancelled"));
        REQUIRE(p.n >= nMax);                                                       // not cancelled too early
        REQUIRE(nMax > 0 || p.calls == 1);
        REQUIRE(!memcmp(image.data(), before.data(), image.size() * 4));            // a cancelled host execute writes nothing
        filter.setProgressMonitorFunction(nullptr);
        filter.execute();                                                           // the filter stays usable
        REQUIRE(device.getError() == Error::None && memcmp(image.data(), before.data(), image.size() * 4));
    } else {
        REQUIRE(device.getError() == Error::None);
        REQUIRE(p.n == 1 && p.calls >= least_calls);
        REQUIRE(memcmp(image.data(), before.data(), image.size() * 4));
    }
    return true;
}

static bool lightmap(const std::string &prefix, bool directional) {
    const int W = 33, H = 17;
    std::vector<float> in((size_t)W * H * 3), out((size_t)W * H * 3, -7.f);
    FILE *f = fopen((prefix + ".lightmap_in").c_str(), "rb");
    REQUIRE(f && fread(in.data(), 4, in.size(), f) == in.size());
    fclose(f);
    DeviceRef device = committed_device();
    FilterRef filter = device.newFilter("RTLightmap");
    REQUIRE(bool(filter) && device.getError() == Error::None);
    filter.setImage("color", in.data(), Format::Float3, W, H);
    filter.setImage("output", out.data(), Format::Float3, W, H);
    filter.set("directional", directional);
    filter.set("inputScale", 0.5f);
    filter.commit();
    REQUIRE(device.getError() == Error::None);
    filter.execute();
    REQUIRE(device.getError() == Error::None && filter.get<float>("scale") == 0.5f);
    f = fopen((prefix + (directional ? ".lightmap_dir" : ".lightmap_hdr")).c_str(), "wb");
    REQUIRE(f && fwrite(out.data(), 4, out.size(), f) == out.size());
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    setWeightsDirectory(argv[1]);
    const std::string prefix = argv[2];
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    RUN(single_filter(1, false));
    RUN(single_filter(3, false));
    RUN(single_filter(3, true));
    RUN(one_filter_at_a_time({63, 511, 257}));
    RUN(several_filters({63, 63, 63}));
    RUN(several_filters({63, 511}));
    RUN(several_filters({511, 63, 257}));
    RUN(two_devices());
    RUN(filter_update(NONE));
    RUN(filter_update(SAME_SIZE));
    RUN(filter_update(DOUBLED));
    RUN(filter_update(REMOVE_IMAGE));
    RUN(filter_update(SET_NULL));
    RUN(filter_update(HDR_OFF));
    RUN(image_size(0, 0));
    RUN(image_size(0, 1));
    RUN(image_size(1, 0));
    RUN(image_size(1, 1));
    RUN(image_size(1, 2));
    RUN(image_size(2, 1));
    RUN(image_size(2, 2));
    RUN(sanitization(true, nan));
    RUN(sanitization(true, inf));
    RUN(sanitization(true, -inf));
    RUN(sanitization(true, -100.f));
    RUN(sanitization(false, nan));
    RUN(sanitization(false, inf));
    RUN(sanitization(false, 10.f));
    RUN(sanitization(false, -2.f));
    // maxMemoryMB = 0 is "no limit" here: one tile, eighteen reports after the first; 289 x 17 under 1 MiB: two tiles and, in place, the copy-out
    RUN(progress(1000, 65, 33, 0, 19));
    RUN(progress(0.5, 65, 33, 0, 0));
    RUN(progress(0, 65, 33, 0, 0));
    RUN(progress(1, 65, 33, 0, 0));
    RUN(progress(1000, 289, 17, 1, 38));
    RUN(progress(0.5, 289, 17, 1, 0));
    RUN(progress(0, 289, 17, 1, 0));
    RUN(progress(1, 289, 17, 1, 0));
    RUN(lightmap(prefix, false));
    RUN(lightmap(prefix, true));
    printf("oidn conformance ok\n");
    return 0;
}
