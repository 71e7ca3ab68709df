// oidn_nodevice_check.cpp -- csrc/oidn_api.h where no HIP device is visible (tests/test_nn_image_cpu.py compiles it and runs it with
// HIP_VISIBLE_DEVICES empty): committing the device leaves UnsupportedHardware, which getError hands out once and the error function
// sees once; a filter of such a device refuses its commit; calls on null handles are InvalidArgument, kept per thread; nothing throws.
#include <cstdio>
#include <cstring>

#include "../mygpuraytracer_amd/csrc/oidn_api.h"

using namespace oidn;

static int g_calls = 0;
static Error g_last = Error::None;
static void on_error(void *user, Error code, const char *message) {
    g_calls++;
    g_last = code;
    *static_cast<int *>(user) += (int)strlen(message) > 0;
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    int with_text = 0;
    DeviceRef device = newDevice();
    const char *message = nullptr;
    EXPECT(device && device.getError(message) == Error::None && message == nullptr);
    device.setErrorFunction(on_error, &with_text);
    device.commit();
    EXPECT(g_calls == 1 && g_last == Error::UnsupportedHardware && with_text == 1);
    EXPECT(device.getError(message) == Error::UnsupportedHardware && message && strstr(message, "no HIP device"));
    EXPECT(device.getError(message) == Error::None && message == nullptr);

    float pixels[3] = {0.f, 0.f, 0.f};
    FilterRef filter = device.newFilter("RT");
    EXPECT(filter && device.getError() == Error::None);
    filter.setImage("color", pixels, Format::Float3, 1, 1);
    filter.setImage("output", pixels, Format::Float3, 1, 1);
    filter.commit();                                   // the device never was committed
    EXPECT(device.getError(message) == Error::InvalidOperation && g_calls == 2);
    filter.set("hdr", true);
    filter.set("srgb", true);
    EXPECT(filter.get<bool>("hdr") && filter.get<bool>("srgb") && filter.get<int>("maxMemoryMB") == 3000);
    filter.set("inputScale", 0.5f);
    EXPECT(filter.get<float>("hdrScale") == 0.5f && device.getError() == Error::None);
    filter.setImage("colour", pixels, Format::Float3, 1, 1);
    EXPECT(device.getError() == Error::InvalidArgument);
    EXPECT(filter.get<int>("networkBuilds") == 0 && device.getError() == Error::None);
    DeviceRef second = device;                         // copies share the device and its error state
    EXPECT(!device.newFilter("RTLightmap") && second.getError() == Error::InvalidArgument && device.getError() == Error::None);

    // null handles: InvalidArgument, read through a null DeviceRef on the same thread
    const int calls = g_calls;
    FilterRef none;
    EXPECT(!none);
    none.commit();
    none.execute();
    none.setImage("color", pixels, Format::Float3, 1, 1);
    EXPECT(none.get<int>("networkBuilds") == 0);
    DeviceRef null;
    EXPECT(!null && null.getError(message) == Error::InvalidArgument && message && null.getError() == Error::None);
    null.commit();
    EXPECT(!null.newFilter("RT") && null.getError() == Error::InvalidArgument);
    EXPECT(g_calls == calls && device.getError() == Error::None);
    printf("oidn nodevice ok\n");
    return 0;
}
