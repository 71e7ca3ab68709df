// oidn_api.h -- Open Image Denoise's C++ names over this library's network denoiser (ptx_nn_* of include/mi355x_pathtracer.h), so that
// a caller written against OIDN -- the reference's CPUdenoise(), apps/src/main.cpp:167-219: newDevice, newFilter("RT"), setImage x 3,
// commit, execute -- compiles and runs with this header in place of OIDN's.  Written in this project's words: the interface has OIDN's
// shape, the text is ours, and what stands behind it is ptx_nn_denoise_images_* (csrc/pt_nn_image.hip), whose descriptor setImage fills.
//
// Offered: DeviceType, Error, Format; newDevice, DeviceRef, FilterRef with the calls below; the "RT" filter.  Not offered: BufferRef,
// the progress monitor, the RTLightmap filter, the C API.  No weights ship: see Weights.
//
// Behaviour, restated from OIDN's UNetFilter::init and RTFilter (core/unet.cpp:241-353, :596-687):
//   Errors: no veneer call throws.  A failed call leaves its error with the device -- the first is kept until getError reads it --
//     and hands it to the device's error function, when one is set (what that function throws is the caller's own and passes through,
//     as main.cpp:92-95 relies on).  Calls on a null DeviceRef / FilterRef are InvalidArgument, kept per thread and read by
//     DeviceRef().getError.  newFilter of any type but "RT" is InvalidArgument and gives a null FilterRef.
//   Parameters (unet.cpp:655-687): hdr, srgb, cleanAux (bool); maxMemoryMB (int, default 3000: ptx_nn_create_tiled's limit);
//     inputScale, with hdrScale as its older name (float, default NaN: automatic); read-only alignment = 16 and overlap = 96.
//   commit (unet.cpp:250-278) refuses with InvalidOperation: no input image; no output image; an input of another size than the
//     output; inputs of mixed formats; hdr with srgb; and what the weight table refuses.
//   Weights (unet.cpp:290-336, :596-611): the caller's "weights" data when set; else the file <dir>/<name>.tza, <dir> from
//     setWeightsDirectory() or the environment variable MI355X_OIDN_WEIGHTS, <name> by the inputs: colour alone rt_hdr / rt_ldr; colour +
//     albedo rt_hdr_alb / rt_ldr_alb; colour + albedo + normal rt_{hdr,ldr}_alb_nrm, with cleanAux rt_{hdr,ldr}_calb_cnrm; albedo alone
//     rt_alb (hdr refused; PTX_NN_ROLE_ALBEDO); normal alone rt_nrm (hdr and srgb refused; PTX_NN_ROLE_NORMAL); anything else
//     "unsupported combination of input features".  No directory or no such file: InvalidOperation.
//   The network (a ptx_nn) is built by the first commit and by a commit after a change of the size, the weights, maxMemoryMB or the
//     number of inputs; a commit that changes only pointers, offsets, strides, formats, hdr, srgb or inputScale keeps it.
//     get<int>("networkBuilds"), an extension, counts the builds.
//   execute runs ptx_nn_denoise_images_host with samples = 1 and waits.  With the extension device.set("imagesOnDevice", true) before
//     device.commit(), image pointers are device pointers and execute runs ptx_nn_denoise_images_device on the default stream and waits.
//     get<float>("scale"), an extension: the scale the last execute used.  device.set("deviceOrdinal", k), an extension: the HIP device.
#pragma once
#include <stddef.h>

namespace oidn {

enum class DeviceType { Default, CPU };
enum class Error { None, Unknown, InvalidArgument, InvalidOperation, OutOfMemory, UnsupportedHardware, Cancelled };
enum class Format { Undefined, Float3, Half3 };

typedef void (*ErrorFunction)(void *userPtr, Error code, const char *message);

// Extension: where the weight files are looked for (NULL or "": the environment variable MI355X_OIDN_WEIGHTS alone).  Process-wide.
void setWeightsDirectory(const char *dir);

namespace detail {

struct Device;
struct Filter;
void retain(Device *d);
void release(Device *d);
void retain(Filter *f);
void release(Filter *f);

// The weight table: the file name without directory and extension for these inputs, or NULL with *why the refusal.  role receives
// PTX_NN_ROLE_COLOR (0), _ALBEDO (1) or _NORMAL (2).  Host only and inline, so that a check can call it without the library.
inline const char *weightsName(bool color, bool albedo, bool normal, bool hdr, bool srgb, bool cleanAux, int *role, const char **why) {
    *why = nullptr;
    *role = 0;
    if (hdr && srgb) { *why = "hdr and srgb modes cannot be enabled at the same time"; return nullptr; }
    if (color) {
        if (!albedo && !normal) return hdr ? "rt_hdr" : "rt_ldr";
        if (albedo && !normal) return hdr ? "rt_hdr_alb" : "rt_ldr_alb";
        if (albedo && normal) return cleanAux ? (hdr ? "rt_hdr_calb_cnrm" : "rt_ldr_calb_cnrm") : (hdr ? "rt_hdr_alb_nrm" : "rt_ldr_alb_nrm");
        *why = "unsupported combination of input features";
        return nullptr;
    }
    if (albedo && !normal) {
        if (hdr) { *why = "hdr mode is not supported for albedo filtering"; return nullptr; }
        *role = 1;
        return "rt_alb";
    }
    if (!albedo && normal) {
        if (hdr || srgb) { *why = "hdr and srgb modes are not supported for normal filtering"; return nullptr; }
        *role = 2;
        return "rt_nrm";
    }
    *why = albedo ? "unsupported combination of input features" : "input image not specified";
    return nullptr;
}

// a reference-counted handle; copies share the object
template <class T> class Ref {
public:
    Ref() : p(nullptr) {}
    explicit Ref(T *adopted) : p(adopted) {}
    Ref(const Ref &o) : p(o.p) { if (p) retain(p); }
    Ref(Ref &&o) noexcept : p(o.p) { o.p = nullptr; }
    Ref &operator=(const Ref &o) { if (o.p) retain(o.p); if (p) release(p); p = o.p; return *this; }
    Ref &operator=(Ref &&o) noexcept { if (this != &o) { if (p) release(p); p = o.p; o.p = nullptr; } return *this; }
    ~Ref() { if (p) release(p); }
    T *get() const { return p; }
private:
    T *p;
};

}  // namespace detail

class FilterRef {
public:
    FilterRef() {}
    explicit FilterRef(detail::Filter *adopted) : h(adopted) {}
    explicit operator bool() const { return h.get() != nullptr; }
    detail::Filter *getHandle() const { return h.get(); }

    void setImage(const char *name, void *ptr, Format format, size_t width, size_t height, size_t byteOffset = 0, size_t bytePixelStride = 0,
                  size_t byteRowStride = 0);
    void removeImage(const char *name);
    void setData(const char *name, void *ptr, size_t byteSize);       // "weights": a TZA blob, the caller's memory, read at commit
    void updateData(const char *name);                                // the blob's contents changed: the next commit builds again
    void removeData(const char *name);
    void set(const char *name, bool value);
    void set(const char *name, int value);
    void set(const char *name, float value);
    template <class T> T get(const char *name);
    void commit();
    void execute();

private:
    bool get1b(const char *name);
    int get1i(const char *name);
    float get1f(const char *name);
    detail::Ref<detail::Filter> h;
};
template <> inline bool FilterRef::get<bool>(const char *name) { return get1b(name); }
template <> inline int FilterRef::get<int>(const char *name) { return get1i(name); }
template <> inline float FilterRef::get<float>(const char *name) { return get1f(name); }

class DeviceRef {
public:
    DeviceRef() {}
    explicit DeviceRef(detail::Device *adopted) : h(adopted) {}
    explicit operator bool() const { return h.get() != nullptr; }
    detail::Device *getHandle() const { return h.get(); }

    void commit();
    Error getError();                                                 // the first error since the last getError, which this clears
    Error getError(const char *&outMessage);                          // outMessage: valid until the next call on this device / thread
    void setErrorFunction(ErrorFunction fn, void *userPtr = nullptr);
    void set(const char *name, bool value);
    void set(const char *name, int value);
    template <class T> T get(const char *name);
    FilterRef newFilter(const char *type);

private:
    bool get1b(const char *name);
    int get1i(const char *name);
    detail::Ref<detail::Device> h;
};
template <> inline bool DeviceRef::get<bool>(const char *name) { return get1b(name); }
template <> inline int DeviceRef::get<int>(const char *name) { return get1i(name); }

DeviceRef newDevice(DeviceType type = DeviceType::Default);

}  // namespace oidn
