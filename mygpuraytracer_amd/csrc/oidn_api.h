// oidn_api.h -- Open Image Denoise's C++ names over this library's network denoiser (ptx_nn_* of include/mi355x_pathtracer.h), so that
// a caller written against OIDN -- the reference's CPUdenoise(), apps/src/main.cpp:167-219: newDevice, newFilter("RT"), setImage x 3,
// commit, execute -- compiles and runs with this header in place of OIDN's.  Written in this project's words: the interface has OIDN's
// shape, the text is ours, and what stands behind it is ptx_nn_denoise_images_* (csrc/pt_nn_image.hip), whose descriptor setImage fills.
//
// Offered: DeviceType, Error, Format, Access; newDevice, DeviceRef, BufferRef, FilterRef with the calls below, the progress monitor
// among them; the "RT" filter and, on request, the "RTLightmap" filter -- the interface that OIDN's own oidnDenoise, oidnTest and
// oidnBenchmark are written against (INTEGRATION.md 1 has the recipe).  Not offered: the C API.  No weights ship: see Weights.
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
//   Format has OIDN's names and numbers (Float = 1 .. Float4 = 4, Half = 257 .. Half4 = 260), so that Format(int(dataType) + channels
//     - 1) means what it means there.  setImage takes any of them; commit accepts Float3 / Half3 images alone, with OIDN's messages.
//   Buffers: device.newBuffer(byteSize) owns host memory aligned to 128 bytes, newBuffer(ptr, byteSize) shares the caller's.  map hands
//     out getData() + offset (size 0: to the end), unmap does nothing: the memory is the host's.  setImage(name, buffer, ...) refuses
//     (InvalidArgument, "buffer region out of range") an image whose byte interval leaves the buffer, and the image keeps the buffer
//     alive.  With imagesOnDevice a buffer image is InvalidOperation: a buffer is host memory.
//   Progress: setProgressMonitorFunction(fn, userPtr) puts ptx_nn_set_progress' monitor on the filter's network for its executes (the
//     public header, "progress": 0 first, after every stage of every tile, exactly 1 last; the execute runs to completion).  fn
//     returning false cancels: execute leaves Error::Cancelled, "execution was cancelled", and the output untouched (host images).
//   Images of size 0: commit makes every check it makes otherwise, the weights included -- the blob is parsed by the host-only plan
//     (ptx_debug_nn_plan) -- but builds no network, and execute returns without error.  Such a filter needs no committed HIP device.
//   Device parameters: numThreads (int), setAffinity and verbose (bool or int) are accepted and read back, with no effect; version,
//     versionMajor, versionMinor, versionPatch read as 10402, 1, 4, 2: the interface restated here is OIDN 1.4.2's.
//   The RTLightmap filter (OIDN's RTLightmapFilter): images color and output; parameters directional (bool), maxMemoryMB, inputScale /
//     hdrScale, the read-only alignment and overlap; hdr, srgb, cleanAux, albedo and normal are "unknown filter parameter".  Weights:
//     the caller's "weights" data, else <dir>/rtlightmap_hdr.tza or, directional, <dir>/rtlightmap_dir.tza (detail::lightmapWeightsName).
//     execute runs ptx_nn_denoise_lightmap_host (or _device with imagesOnDevice).  It is offered to callers that ask: the device
//     parameter filterRTLightmap (bool, before device.commit()).  A translation unit compiled with OIDN_FILTER_RTLIGHTMAP defined --
//     OIDN's own CMake makes that definition PUBLIC for its consumers -- gets a newDevice that sets it: an inline function of an inline
//     namespace keyed by the macro, so translation units of both kinds link into one program without two definitions of one name.  The
//     exported oidn::newDevice(DeviceType) gives the device without it, for which newFilter("RTLightmap") stays null / InvalidArgument.
#pragma once
#include <stddef.h>

namespace oidn {

enum class DeviceType { Default, CPU };
enum class Error { None, Unknown, InvalidArgument, InvalidOperation, OutOfMemory, UnsupportedHardware, Cancelled };
enum class Format { Undefined = 0, Float = 1, Float2, Float3, Float4, Half = 257, Half2, Half3, Half4 };
enum class Access { Read, Write, ReadWrite, WriteDiscard };

typedef void (*ErrorFunction)(void *userPtr, Error code, const char *message);
typedef bool (*ProgressMonitorFunction)(void *userPtr, double n);     // false: cancel

// Extension: where the weight files are looked for (NULL or "": the environment variable MI355X_OIDN_WEIGHTS alone).  Process-wide.
void setWeightsDirectory(const char *dir);

namespace detail {

struct Device;
struct Filter;
struct Buffer;
void retain(Device *d);
void release(Device *d);
void retain(Filter *f);
void release(Filter *f);
void retain(Buffer *b);
void release(Buffer *b);

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

// The lightmap filter's weight table: rtlightmap_hdr, or rtlightmap_dir for the directional one.  Host only and inline, like weightsName.
inline const char *lightmapWeightsName(bool directional) { return directional ? "rtlightmap_dir" : "rtlightmap_hdr"; }

// bytes per channel and channels per pixel of a format; 0: Undefined or no format at all
inline size_t formatChannelSize(Format f) { return (int)f >= 1 && (int)f <= 4 ? 4 : (int)f >= 257 && (int)f <= 260 ? 2 : 0; }
inline size_t formatChannels(Format f) { return formatChannelSize(f) == 4 ? (size_t)f : formatChannelSize(f) == 2 ? (size_t)f - 256 : 0; }

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

class BufferRef {
public:
    BufferRef() {}
    explicit BufferRef(detail::Buffer *adopted) : h(adopted) {}
    explicit operator bool() const { return h.get() != nullptr; }
    detail::Buffer *getHandle() const { return h.get(); }

    void *getData() const;                                            // NULL for a null buffer or one of size 0
    size_t getSize() const;
    void *map(Access access = Access::ReadWrite, size_t byteOffset = 0, size_t byteSize = 0);      // byteSize 0: to the end
    void unmap(void *mappedPtr);

private:
    detail::Ref<detail::Buffer> h;
};

class FilterRef {
public:
    FilterRef() {}
    explicit FilterRef(detail::Filter *adopted) : h(adopted) {}
    explicit operator bool() const { return h.get() != nullptr; }
    detail::Filter *getHandle() const { return h.get(); }

    void setImage(const char *name, void *ptr, Format format, size_t width, size_t height, size_t byteOffset = 0, size_t bytePixelStride = 0,
                  size_t byteRowStride = 0);
    void setImage(const char *name, const BufferRef &buffer, Format format, size_t width, size_t height, size_t byteOffset = 0,
                  size_t bytePixelStride = 0, size_t byteRowStride = 0);
    void removeImage(const char *name);
    void setData(const char *name, void *ptr, size_t byteSize);       // "weights": a TZA blob, the caller's memory, read at commit
    void updateData(const char *name);                                // the blob's contents changed: the next commit builds again
    void removeData(const char *name);
    void set(const char *name, bool value);
    void set(const char *name, int value);
    void set(const char *name, float value);
    template <class T> T get(const char *name);
    void setProgressMonitorFunction(ProgressMonitorFunction fn, void *userPtr = nullptr);      // fn NULL: none
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
    FilterRef newFilter(const char *type) const;
    BufferRef newBuffer(size_t byteSize) const;                       // owned host memory, aligned to 128 bytes
    BufferRef newBuffer(void *ptr, size_t byteSize) const;            // the caller's memory, shared

private:
    bool get1b(const char *name);
    int get1i(const char *name);
    detail::Ref<detail::Device> h;
};
template <> inline bool DeviceRef::get<bool>(const char *name) { return get1b(name); }
template <> inline int DeviceRef::get<int>(const char *name) { return get1i(name); }

namespace detail {
DeviceRef newDevice(DeviceType type, bool filterRTLightmap);
}

#if defined(OIDN_FILTER_RTLIGHTMAP)
// this translation unit asked for the lightmap filter: its newDevice is another function than the exported one, under another name
inline namespace rtlightmap_offered {
inline DeviceRef newDevice(DeviceType type = DeviceType::Default) { return detail::newDevice(type, true); }
}
#else
DeviceRef newDevice(DeviceType type = DeviceType::Default);
#endif

}  // namespace oidn
