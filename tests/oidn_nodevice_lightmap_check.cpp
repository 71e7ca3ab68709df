// oidn_nodevice_lightmap_check.cpp -- csrc/oidn_api.h's newer half where no HIP device is visible (tests/test_oidn_lightmap_cpu.py compiles
// it with and without -DOIDN_FILTER_RTLIGHTMAP and runs it with HIP_VISIBLE_DEVICES empty; argv[1] is a 3-input weight blob): the
// RTLightmap filter is offered exactly to a translation unit that asks, with its parameter names and refusals; the weight table; buffers
// (size, data, map, the out-of-range image, the lifetime of a buffer whose BufferRef is gone); Format's numbers; filters of 0 x 0,
// 0 x 1 and 1 x 0 images, which commit and execute without a device; the device's parameters.  Compiled with -DSECOND_UNIT it is the
// other half of a program made of both kinds of translation unit.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mygpuraytracer_amd/csrc/oidn_api.h"

using namespace oidn;

#if defined(OIDN_FILTER_RTLIGHTMAP)
static const bool ASKED = true;
#else
static const bool ASKED = false;
#endif

#if defined(SECOND_UNIT)

bool second_unit_asked() { return ASKED; }
bool second_unit_gets_the_lightmap_filter() {
    DeviceRef device = newDevice();
    return bool(device.newFilter("RTLightmap"));
}

#else

#if defined(WITH_SECOND_UNIT)
bool second_unit_asked();
bool second_unit_gets_the_lightmap_filter();
#endif

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); return 1; } } while (0)

static std::vector<unsigned char> read_all(const char *path) {
    std::vector<unsigned char> blob;
    if (FILE *f = fopen(path, "rb")) {
        unsigned char buf[4096];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + got);
        fclose(f);
    }
    return blob;
}

int main(int argc, char **argv) {
    EXPECT(argc > 1);
    std::vector<unsigned char> weights = read_all(argv[1]);
    EXPECT(weights.size() > 1000);
    const char *message = nullptr;

    // Format's numbers are OIDN's: Format(int(dataType) + channels - 1)
    EXPECT((int)Format::Undefined == 0 && (int)Format::Float == 1 && (int)Format::Float2 == 2 && (int)Format::Float3 == 3 && (int)Format::Float4 == 4);
    EXPECT((int)Format::Half == 257 && (int)Format::Half2 == 258 && (int)Format::Half3 == 259 && (int)Format::Half4 == 260);
    EXPECT(Format(int(Format::Half) + 3 - 1) == Format::Half3 && Format(int(Format::Float) + 3 - 1) == Format::Float3);
    EXPECT(detail::formatChannels(Format::Half4) == 4 && detail::formatChannelSize(Format::Half4) == 2 && detail::formatChannels(Format::Undefined) == 0);
    EXPECT(!strcmp(detail::lightmapWeightsName(false), "rtlightmap_hdr") && !strcmp(detail::lightmapWeightsName(true), "rtlightmap_dir"));

    const DeviceRef device = newDevice();              // (const: newBuffer and newFilter are const members)
    DeviceRef handle = device;
    EXPECT(device && handle.getError() == Error::None);
    EXPECT(handle.get<bool>("filterRTLightmap") == ASKED);

    // the device's parameters: kept and read back, the version is the restated interface's
    handle.set("numThreads", 7);
    handle.set("setAffinity", false);
    handle.set("verbose", 2);
    EXPECT(handle.get<int>("numThreads") == 7 && !handle.get<bool>("setAffinity") && handle.get<int>("verbose") == 2);
    EXPECT(handle.get<int>("version") == 10402 && handle.get<int>("versionMajor") == 1 && handle.get<int>("versionMinor") == 4 && handle.get<int>("versionPatch") == 2);
    EXPECT(handle.getError() == Error::None);
    handle.get<int>("nonesuch");
    EXPECT(handle.getError() == Error::InvalidArgument);

    // the filter: only for a caller that asked
    FilterRef lightmap = device.newFilter("RTLightmap");
    if (!ASKED) {
        EXPECT(!lightmap && handle.getError(message) == Error::InvalidArgument && message);
        DeviceRef asks = newDevice();
        asks.set("filterRTLightmap", true);            // the request by hand
        EXPECT(asks.newFilter("RTLightmap") && asks.getError() == Error::None);
    } else {
        EXPECT(lightmap && handle.getError() == Error::None);
        lightmap.set("directional", true);
        EXPECT(lightmap.get<bool>("directional") && handle.getError() == Error::None);
        lightmap.set("hdr", true);
        EXPECT(handle.getError(message) == Error::InvalidArgument && !strcmp(message, "unknown filter parameter"));
        lightmap.set("srgb", true);
        EXPECT(handle.getError() == Error::InvalidArgument);
        lightmap.set("cleanAux", true);
        EXPECT(handle.getError() == Error::InvalidArgument);
        lightmap.get<bool>("hdr");
        EXPECT(handle.getError() == Error::InvalidArgument);
        float px[3] = {0.f, 0.f, 0.f};
        lightmap.setImage("albedo", px, Format::Float3, 1, 1);
        EXPECT(handle.getError() == Error::InvalidArgument);
        lightmap.set("maxMemoryMB", 100);
        lightmap.set("inputScale", 0.5f);
        EXPECT(lightmap.get<int>("maxMemoryMB") == 100 && lightmap.get<float>("hdrScale") == 0.5f && lightmap.get<int>("alignment") == 16 &&
               lightmap.get<int>("overlap") > 0 && handle.getError() == Error::None);
        // no weights and no directory: the commit of a 0 x 0 filter names the file it wants
        lightmap.setImage("color", px, Format::Float3, 0, 0);
        lightmap.setImage("output", px, Format::Float3, 0, 0);
        setWeightsDirectory("/nonexistent-weights-directory");
        lightmap.commit();
        EXPECT(handle.getError(message) == Error::InvalidOperation && strstr(message, "rtlightmap_dir.tza"));
        lightmap.set("directional", false);
        lightmap.commit();
        EXPECT(handle.getError(message) == Error::InvalidOperation && strstr(message, "rtlightmap_hdr.tza"));
        lightmap.setData("weights", weights.data(), weights.size());
        lightmap.commit();
        EXPECT(handle.getError() == Error::None);
        lightmap.execute();
        EXPECT(handle.getError() == Error::None);
    }
    EXPECT(device.newFilter("RT") && !device.newFilter("RTX") && handle.getError() == Error::InvalidArgument);

    // buffers
    {
        BufferRef owned = device.newBuffer(1000);
        EXPECT(owned && owned.getSize() == 1000 && owned.getData() && ((size_t)owned.getData() & 127) == 0);
        memset(owned.getData(), 0x5a, 1000);
        EXPECT(owned.map(Access::Read, 10, 20) == (char *)owned.getData() + 10 && owned.map() == owned.getData());
        owned.unmap(owned.getData());
        EXPECT(owned.map(Access::Write, 990, 11) == nullptr && handle.getError() == Error::InvalidArgument);
        float mine[12];
        BufferRef shared = device.newBuffer(mine, sizeof mine);
        EXPECT(shared && shared.getData() == mine && shared.getSize() == sizeof mine);
        BufferRef copy = shared, moved = static_cast<BufferRef &&>(copy);
        EXPECT(moved.getData() == mine && !copy && copy.getSize() == 0 && copy.getData() == nullptr);
        BufferRef empty = device.newBuffer(0);
        EXPECT(empty && empty.getSize() == 0 && empty.getData() == nullptr && handle.getError() == Error::None);

        FilterRef filter = device.newFilter("RT");
        // 2 x 2 Float3 is 48 bytes: it fits `mine` exactly, and not one byte later
        filter.setImage("color", shared, Format::Float3, 2, 2);
        EXPECT(handle.getError() == Error::None);
        filter.setImage("color", shared, Format::Float3, 2, 2, 4);
        EXPECT(handle.getError(message) == Error::InvalidArgument && strstr(message, "out of range"));
        filter.setImage("color", shared, Format::Float3, 1, 2, 0, 12, 36);          // rows 36 apart: 36 + 12 = 48
        EXPECT(handle.getError() == Error::None);
        filter.setImage("color", shared, Format::Float3, 1, 2, 0, 12, 40);
        EXPECT(handle.getError() == Error::InvalidArgument);
        filter.setImage("color", shared, Format::Float4, 3, 1);                     // 48 bytes
        EXPECT(handle.getError() == Error::None);
        filter.setImage("color", shared, Format::Float4, 1, 4);
        EXPECT(handle.getError() == Error::InvalidArgument);
        filter.setImage("color", shared, Format::Float3, (size_t)-1 / 4, (size_t)-1 / 4);      // overflows size_t: refused, not wrapped
        EXPECT(handle.getError() == Error::InvalidArgument);
        filter.setImage("color", shared, Format::Undefined, 1, 1);
        EXPECT(handle.getError() == Error::InvalidArgument);
        filter.setImage("color", shared, Format::Float3, 0, 0, 48);                 // empty, at the very end
        EXPECT(handle.getError() == Error::None);
        filter.setImage("color", shared, Format::Float3, 0, 0, 49);
        EXPECT(handle.getError() == Error::InvalidArgument);
        filter.setImage("color", BufferRef(), Format::Float3, 1, 1);
        EXPECT(handle.getError() == Error::InvalidArgument);
        // an image keeps its buffer alive: the BufferRef goes, the 0 x 1 filter still commits and executes
        {
            BufferRef gone = device.newBuffer(64);
            filter.setImage("color", gone, Format::Float3, 0, 1);
            filter.setImage("output", gone, Format::Float3, 0, 1);
        }
        filter.setData("weights", weights.data(), weights.size());
        filter.commit();
        EXPECT(handle.getError(message) == Error::None);
        filter.execute();
        EXPECT(handle.getError() == Error::None && filter.get<int>("networkBuilds") == 0);
        // with imagesOnDevice a buffer image is refused
        DeviceRef on_device = newDevice();
        on_device.set("imagesOnDevice", true);
        FilterRef f2 = on_device.newFilter("RT");
        f2.setImage("color", on_device.newBuffer(64), Format::Float3, 1, 1);
        EXPECT(on_device.getError() == Error::InvalidOperation);
    }

    // images of size 0: every check but the network; no device needed
    const int sizes[3][2] = {{0, 0}, {0, 1}, {1, 0}};
    for (const auto &wh : sizes) {
        float in[3] = {0.5f, 0.5f, 0.5f}, out[3] = {-7.f, -7.f, -7.f};
        FilterRef filter = device.newFilter("RT");
        filter.setImage("color", in, Format::Float3, wh[0], wh[1]);
        filter.setImage("output", out, Format::Float3, wh[0], wh[1]);
        filter.execute();
        EXPECT(handle.getError() == Error::InvalidOperation);                       // not committed
        filter.commit();
        EXPECT(handle.getError(message) == Error::InvalidOperation && strstr(message, "rt_ldr.tza"));      // the weights are looked for
        filter.setData("weights", weights.data(), 100);
        filter.commit();
        EXPECT(handle.getError() == Error::InvalidOperation);                       // ... and parsed
        filter.setData("weights", weights.data(), weights.size());
        filter.set("hdr", true);
        filter.set("srgb", true);
        filter.commit();
        EXPECT(handle.getError() == Error::InvalidOperation);                       // hdr with srgb
        filter.set("srgb", false);
        filter.setImage("albedo", in, Format::Float3, 1, 1);
        filter.commit();
        EXPECT(handle.getError() == Error::InvalidOperation);                       // image size mismatch
        filter.setImage("albedo", nullptr, Format::Float3, 0, 0);                   // removes it
        filter.setImage("output", out, Format::Float2, wh[0], wh[1]);
        filter.commit();
        EXPECT(handle.getError(message) == Error::InvalidOperation && strstr(message, "output image format"));
        filter.setImage("output", out, Format::Float3, wh[0], wh[1]);
        filter.commit();
        EXPECT(handle.getError(message) == Error::None);
        filter.execute();
        filter.execute();
        EXPECT(handle.getError() == Error::None && out[0] == -7.f && filter.get<int>("networkBuilds") == 0);
        filter.setProgressMonitorFunction([](void *, double) { return false; }, nullptr);
        filter.execute();                                                           // nothing runs, nothing to cancel
        EXPECT(handle.getError() == Error::None);
    }
    // a 1 x 1 filter does need the device, which never was committed
    {
        float in[3] = {0.5f, 0.5f, 0.5f};
        FilterRef filter = device.newFilter("RT");
        filter.setImage("color", in, Format::Float3, 1, 1);
        filter.setImage("output", in, Format::Float3, 1, 1);
        filter.setData("weights", weights.data(), weights.size());
        filter.commit();
        EXPECT(handle.getError() == Error::InvalidOperation);
    }
    FilterRef none;
    none.setProgressMonitorFunction(nullptr);
    EXPECT(DeviceRef().getError() == Error::InvalidArgument);
    EXPECT(!DeviceRef().newBuffer(16) && DeviceRef().getError() == Error::InvalidArgument);

#if defined(WITH_SECOND_UNIT)
    EXPECT(second_unit_asked() != ASKED);
    EXPECT(second_unit_gets_the_lightmap_filter() == second_unit_asked());
    EXPECT(bool(newDevice().newFilter("RTLightmap")) == ASKED);
#endif
    printf("oidn nodevice lightmap ok (%s)\n", ASKED ? "asked" : "not asked");
    return 0;
}

#endif
