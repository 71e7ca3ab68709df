// oidn_api.cpp -- the veneer of oidn_api.h: OIDN's device and filter handles over ptx_nn and ptx_nn_denoise_images_*.  Host code; every
// device call is the C ABI's.  A veneer call runs under `guard`, which turns whatever is thrown inside into the device's error.
#include "oidn_api.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/mi355x_pathtracer.h"

namespace oidn {
namespace {

struct Failure {
    Error code;
    std::string message;
};

struct ErrorState {
    Error code = Error::None;
    std::string message, read;      // read: what the last getError handed out
};

thread_local ErrorState tl_error;   // of calls on null handles

std::mutex g_dir_mutex;
std::string g_weights_dir;

std::string weights_dir() {
    {
        std::lock_guard<std::mutex> lock(g_dir_mutex);
        if (!g_weights_dir.empty()) return g_weights_dir;
    }
    const char *env = getenv("MI355X_OIDN_WEIGHTS");
    return env ? env : "";
}

// a ptx return code as OIDN's error, with ptx_last_error's text
Failure ptx_failure(int rc, const char *during) {
    const std::string msg = std::string(during) + ": " + ptx_last_error();
    if (rc == PTX_ERR_NODEVICE) return {Error::UnsupportedHardware, msg};
    if (rc == PTX_ERR_IO) return {Error::InvalidOperation, msg};
    if (rc == PTX_ERR_INVALID) return {Error::InvalidArgument, msg};
    if (rc == PTX_ERR_CANCELLED) return {Error::Cancelled, "execution was cancelled"};
    if (rc == PTX_ERR_HIP && msg.find("out of memory") != std::string::npos) return {Error::OutOfMemory, msg};
    return {Error::Unknown, msg};
}

struct ImageParam {
    bool set = false;
    void *ptr = nullptr;
    detail::Ref<detail::Buffer> buffer;      // of an image set from a buffer: kept alive with the image
    Format format = Format::Undefined;
    size_t width = 0, height = 0, offset = 0, pixel_stride = 0, row_stride = 0;
};

int image_slot(const char *name) {
    static const char *const names[4] = {"color", "albedo", "normal", "output"};
    for (int k = 0; k < 4; k++)
        if (name && !strcmp(name, names[k])) return k;
    return -1;
}

}  // namespace

namespace detail {

struct Device {
    std::atomic<int> refs{1};
    std::mutex mutex;               // the error state and the settings
    ErrorState error;
    ErrorFunction fn = nullptr;
    void *user = nullptr;
    bool committed = false, images_on_device = false, lightmap = false;
    int ordinal = 0;
    int num_threads = 0, set_affinity = 1, verbose = 0;      // OIDN's CPU device's: kept and read back, no effect
};

struct Buffer {
    std::atomic<int> refs{1};
    Device *device = nullptr;       // retained
    void *ptr = nullptr;
    size_t size = 0;
    bool owned = false;
    ~Buffer() {
        if (owned) free(ptr);
        if (device) release(device);
    }
};

struct Filter {
    std::atomic<int> refs{1};
    Device *device = nullptr;       // retained
    ImageParam image[4];            // color, albedo, normal, output
    void *user_weights = nullptr;
    size_t user_weights_size = 0;
    unsigned long long weights_version = 0;
    bool lightmap = false, directional = false;      // the RTLightmap filter; its one bool
    ProgressMonitorFunction progress = nullptr;
    void *progress_user = nullptr;
    bool empty = false;                              // committed with images of size 0: no network, execute does nothing
    bool hdr = false, srgb = false, clean_aux = false;
    int max_memory_mb = 3000;
    float input_scale = NAN;
    bool dirty = true;
    // what the last commit made
    ptx_nn *nn = nullptr;
    int builds = 0, role = 0;
    ImageParam committed[4];
    struct Key {
        size_t width = 0, height = 0;
        int max_memory_mb = 0, inputs = 0;
        std::string file;
        void *user = nullptr;
        size_t user_size = 0;
        unsigned long long version = 0;
        bool operator==(const Key &o) const {
            return width == o.width && height == o.height && max_memory_mb == o.max_memory_mb && inputs == o.inputs && file == o.file &&
                   user == o.user && user_size == o.user_size && version == o.version;
        }
    } key;
    ~Filter() {
        if (nn) ptx_nn_destroy(nn);
        if (device) release(device);
    }
};

void retain(Device *d) { d->refs.fetch_add(1, std::memory_order_relaxed); }
void release(Device *d) { if (d->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete d; }
void retain(Filter *f) { f->refs.fetch_add(1, std::memory_order_relaxed); }
void release(Filter *f) { if (f->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete f; }
void retain(Buffer *b) { b->refs.fetch_add(1, std::memory_order_relaxed); }
void release(Buffer *b) { if (b->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete b; }

}  // namespace detail

namespace {

using detail::Buffer;
using detail::Device;
using detail::Filter;

// keeps the first error and tells the error function; d NULL: the thread's state
void report(Device *d, const Failure &f) {
    if (!d) {
        if (tl_error.code == Error::None) { tl_error.code = f.code; tl_error.message = f.message; }
        return;
    }
    ErrorFunction fn;
    void *user;
    {
        std::lock_guard<std::mutex> lock(d->mutex);
        if (d->error.code == Error::None) { d->error.code = f.code; d->error.message = f.message; }
        fn = d->fn; user = d->user;
    }
    if (fn) fn(user, f.code, f.message.c_str());
}

// body() with everything it throws turned into the device's error; only what the error function itself throws leaves
template <class Body> void guard(Device *d, Body body) {
    Failure failure{Error::None, ""};
    try {
        body();
        return;
    } catch (const Failure &f) {
        failure = f;
    } catch (const std::bad_alloc &) {
        failure = {Error::OutOfMemory, "out of memory"};
    } catch (const std::exception &e) {
        failure = {Error::Unknown, e.what()};
    } catch (...) {
        failure = {Error::Unknown, "unknown exception"};
    }
    report(d, failure);
}

const Failure NULL_HANDLE{Error::InvalidArgument, "invalid handle"};

ptx_nn_image descriptor(const ImageParam &im) {
    ptx_nn_image d;
    d.ptr = im.set ? im.ptr : nullptr;
    d.format = im.format == Format::Float3 ? PTX_NN_FORMAT_FLOAT3 : im.format == Format::Half3 ? PTX_NN_FORMAT_HALF3 : 0;
    d.byte_offset = im.offset; d.pixel_stride = im.pixel_stride; d.row_stride = im.row_stride;
    return d;
}

void read_file(const std::string &path, std::vector<unsigned char> &blob) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) throw Failure{Error::InvalidOperation, "cannot open the weight file " + path};
    unsigned char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + got);
    fclose(f);
}

void commit_filter(Filter *f) {
    Device *d = f->device;
    bool committed;
    int ordinal;
    {
        std::lock_guard<std::mutex> lock(d->mutex);
        committed = d->committed; ordinal = d->ordinal;
    }
    const ImageParam *im = f->image;
    // images of size 0 need no device: every other check is made, no network is built
    const bool empty = im[3].set && (im[3].width == 0 || im[3].height == 0);
    if (!committed && !empty) throw Failure{Error::InvalidOperation, "the device is not committed"};
    // unet.cpp:250-278
    if (!im[0].set && !im[1].set && !im[2].set) throw Failure{Error::InvalidOperation, "input image not specified"};
    if (!im[3].set) throw Failure{Error::InvalidOperation, "output image not specified"};
    Format input = Format::Undefined;
    int inputs = 0;
    for (int k = 0; k < 3; k++) {
        if (!im[k].set) continue;
        inputs++;
        if (im[k].format != Format::Float3 && im[k].format != Format::Half3) throw Failure{Error::InvalidOperation, "unsupported input image format"};
        if (input != Format::Undefined && im[k].format != input) throw Failure{Error::InvalidOperation, "unsupported input image format (mixed Float3 and Half3 inputs)"};
        input = im[k].format;
        if (im[k].width != im[3].width || im[k].height != im[3].height) throw Failure{Error::InvalidOperation, "image size mismatch"};
    }
    if (im[3].format != Format::Float3 && im[3].format != Format::Half3) throw Failure{Error::InvalidOperation, "unsupported output image format"};
    // unet.cpp:290-336
    int role = 0;
    const char *why = nullptr;
    const char *name = f->lightmap ? detail::lightmapWeightsName(f->directional)
                                   : detail::weightsName(im[0].set, im[1].set, im[2].set, f->hdr, f->srgb, f->clean_aux, &role, &why);
    if (!name) throw Failure{Error::InvalidOperation, why};
    Filter::Key key;
    key.width = im[3].width; key.height = im[3].height; key.max_memory_mb = f->max_memory_mb; key.inputs = inputs;
    if (f->user_weights) {
        key.user = f->user_weights; key.user_size = f->user_weights_size; key.version = f->weights_version;
    } else {
        const std::string dir = weights_dir();
        if (dir.empty())
            throw Failure{Error::InvalidOperation, std::string("no weights: none ship; set the \"weights\" data, or setWeightsDirectory() / MI355X_OIDN_WEIGHTS for ") + name + ".tza"};
        key.file = dir + "/" + name + ".tza";
    }
    if (empty || !f->nn || !(key == f->key)) {
        if (key.width > PTX_NN_MAX_FRAME || key.height > PTX_NN_MAX_FRAME) throw Failure{Error::InvalidOperation, "unsupported image size"};
        std::vector<unsigned char> file;
        const void *blob = f->user_weights;
        size_t bytes = f->user_weights_size;
        if (!f->user_weights) {
            read_file(key.file, file);
            blob = file.data(); bytes = file.size();
        }
        if (empty) {
            ptx_nn_info info;
            const int rc = ptx_debug_nn_plan(blob, bytes, &info);                 // host only: the blob is a network, or is refused as one
            if (rc != PTX_OK) throw Failure{Error::InvalidOperation, std::string("building the network: ") + ptx_last_error()};
            if (info.input_channels != 3 * inputs)
                throw Failure{Error::InvalidOperation, "building the network: the weights take " + std::to_string(info.input_channels) +
                                                           " input channels, the filter has " + std::to_string(inputs) + " input image(s)"};
            if (f->nn) ptx_nn_destroy(f->nn);
            f->nn = nullptr; f->key = Filter::Key();
            f->role = role; f->empty = true;
            for (int k = 0; k < 4; k++) f->committed[k] = im[k];
            f->dirty = false;
            return;
        }
        ptx_nn *made = nullptr;
        const int rc = ptx_nn_create_tiled(ordinal, (int)key.width, (int)key.height, blob, bytes, f->max_memory_mb, &made);
        if (rc != PTX_OK) {
            Failure fail = ptx_failure(rc, "building the network");
            if (rc == PTX_ERR_INVALID) fail.code = Error::InvalidOperation;      // a blob or a size the filter cannot run
            throw fail;
        }
        if (f->nn) ptx_nn_destroy(f->nn);
        f->nn = made; f->key = key; f->builds++;
    }
    f->role = role; f->empty = false;
    for (int k = 0; k < 4; k++) f->committed[k] = im[k];
    f->dirty = false;
}

// ptx_nn_progress_fn over the filter's bool monitor
int progress_trampoline(void *user, double n) {
    Filter *f = static_cast<Filter *>(user);
    return f->progress(f->progress_user, n) ? 1 : 0;
}

void execute_filter(Filter *f) {
    if (f->dirty || (!f->nn && !f->empty)) throw Failure{Error::InvalidOperation, "changes to the filter are not committed"};
    if (f->empty) return;
    bool on_device;
    {
        std::lock_guard<std::mutex> lock(f->device->mutex);
        on_device = f->device->images_on_device;
    }
    ptx_nn_image d[4];
    for (int k = 0; k < 4; k++) d[k] = descriptor(f->committed[k]);
    // a prefilter's single image stands where the colour does
    const ptx_nn_image *first = f->role == PTX_NN_ROLE_ALBEDO ? &d[1] : f->role == PTX_NN_ROLE_NORMAL ? &d[2] : &d[0];
    const ptx_nn_image *alb = f->role == PTX_NN_ROLE_COLOR && d[1].ptr ? &d[1] : nullptr;
    const ptx_nn_image *nrm = f->role == PTX_NN_ROLE_COLOR && d[2].ptr ? &d[2] : nullptr;
    ptx_nn_params p;
    ptx_default_nn_params(&p);
    p.hdr = f->hdr; p.srgb = f->srgb; p.input_scale = f->input_scale;
    int rc = ptx_nn_set_progress(f->nn, f->progress ? progress_trampoline : nullptr, f);
    if (rc != PTX_OK) throw ptx_failure(rc, "execute");
    if (on_device) {
        rc = f->lightmap ? ptx_nn_denoise_lightmap_device(f->nn, &d[0], &d[3], f->directional, f->input_scale, nullptr)
                         : ptx_nn_denoise_images_device(f->nn, first, alb, nrm, &d[3], 1.f, f->role, &p, nullptr);
        if (rc != PTX_OK) throw ptx_failure(rc, "execute");
        float scale;
        rc = ptx_nn_read_scale(f->nn, &scale);      // waits for the handle's event
        if (rc != PTX_OK) throw ptx_failure(rc, "execute");
    } else {
        rc = f->lightmap ? ptx_nn_denoise_lightmap_host(f->nn, &d[0], &d[3], f->directional, f->input_scale)
                         : ptx_nn_denoise_images_host(f->nn, first, alb, nrm, &d[3], 1.f, f->role, &p);
        if (rc != PTX_OK) throw ptx_failure(rc, "execute");
    }
}

}  // namespace

void setWeightsDirectory(const char *dir) {
    std::lock_guard<std::mutex> lock(g_dir_mutex);
    g_weights_dir = dir ? dir : "";
}

DeviceRef detail::newDevice(DeviceType type, bool filterRTLightmap) {
    (void)type;                      // Default and CPU alike: the one kind of device here is a HIP device, chosen at commit
    Device *d = new (std::nothrow) Device();
    if (!d) report(nullptr, {Error::OutOfMemory, "out of memory"});
    else d->lightmap = filterRTLightmap;
    return DeviceRef(d);
}

DeviceRef newDevice(DeviceType type) { return detail::newDevice(type, false); }

// ---- DeviceRef -------------------------------------------------------------------------------------------------------------------------
void DeviceRef::commit() {
    Device *d = h.get();
    guard(d, [&] {
        if (!d) throw NULL_HANDLE;
        const int count = ptx_device_count();
        std::unique_lock<std::mutex> lock(d->mutex);
        if (d->committed) throw Failure{Error::InvalidOperation, "device can be committed only once"};
        if (count < 1) throw Failure{Error::UnsupportedHardware, "no HIP device available: the network denoiser has no CPU path"};
        if (d->ordinal < 0 || d->ordinal >= count) throw Failure{Error::InvalidArgument, "deviceOrdinal is out of range"};
        d->committed = true;
    });
}

Error DeviceRef::getError() {
    const char *ignored;
    return getError(ignored);
}

Error DeviceRef::getError(const char *&outMessage) {
    Device *d = h.get();
    ErrorState *e = &tl_error;
    std::unique_lock<std::mutex> lock;
    if (d) {
        lock = std::unique_lock<std::mutex>(d->mutex);
        e = &d->error;
    }
    const Error code = e->code;
    e->read.swap(e->message);
    e->message.clear();
    e->code = Error::None;
    outMessage = code == Error::None ? nullptr : e->read.c_str();
    return code;
}

void DeviceRef::setErrorFunction(ErrorFunction fn, void *userPtr) {
    Device *d = h.get();
    if (!d) { report(nullptr, NULL_HANDLE); return; }
    std::lock_guard<std::mutex> lock(d->mutex);
    d->fn = fn; d->user = userPtr;
}

void DeviceRef::set(const char *name, bool value) {
    Device *d = h.get();
    guard(d, [&] {
        if (!d || !name) throw NULL_HANDLE;
        std::unique_lock<std::mutex> lock(d->mutex);
        if (d->committed) throw Failure{Error::InvalidOperation, "device parameters are set before commit"};
        if (!strcmp(name, "imagesOnDevice")) d->images_on_device = value;
        else if (!strcmp(name, "filterRTLightmap")) d->lightmap = value;
        else if (!strcmp(name, "setAffinity")) d->set_affinity = value;      // (OIDN's CPU device's: kept, without effect)
        else if (!strcmp(name, "verbose")) d->verbose = value;
    });
}

void DeviceRef::set(const char *name, int value) {
    Device *d = h.get();
    guard(d, [&] {
        if (!d || !name) throw NULL_HANDLE;
        std::unique_lock<std::mutex> lock(d->mutex);
        if (d->committed) throw Failure{Error::InvalidOperation, "device parameters are set before commit"};
        if (!strcmp(name, "deviceOrdinal")) d->ordinal = value;
        else if (!strcmp(name, "imagesOnDevice")) d->images_on_device = value != 0;
        else if (!strcmp(name, "filterRTLightmap")) d->lightmap = value != 0;
        else if (!strcmp(name, "numThreads")) d->num_threads = value;
        else if (!strcmp(name, "setAffinity")) d->set_affinity = value != 0;
        else if (!strcmp(name, "verbose")) d->verbose = value;
    });
}

bool DeviceRef::get1b(const char *name) { return get1i(name) != 0; }

int DeviceRef::get1i(const char *name) {
    Device *d = h.get();
    int value = 0;
    guard(d, [&] {
        if (!d || !name) throw NULL_HANDLE;
        std::unique_lock<std::mutex> lock(d->mutex);
        if (!strcmp(name, "imagesOnDevice")) value = d->images_on_device;
        else if (!strcmp(name, "deviceOrdinal")) value = d->ordinal;
        else if (!strcmp(name, "filterRTLightmap")) value = d->lightmap;
        else if (!strcmp(name, "numThreads")) value = d->num_threads;
        else if (!strcmp(name, "setAffinity")) value = d->set_affinity;
        else if (!strcmp(name, "verbose")) value = d->verbose;
        else if (!strcmp(name, "version")) value = 10402;                    // the interface restated here: OIDN 1.4.2's
        else if (!strcmp(name, "versionMajor")) value = 1;
        else if (!strcmp(name, "versionMinor")) value = 4;
        else if (!strcmp(name, "versionPatch")) value = 2;
        else throw Failure{Error::InvalidArgument, "unknown device parameter"};
    });
    return value;
}

FilterRef DeviceRef::newFilter(const char *type) const {
    Device *d = h.get();
    Filter *f = nullptr;
    guard(d, [&] {
        if (!d) throw NULL_HANDLE;
        bool lightmap_offered;
        {
            std::lock_guard<std::mutex> lock(d->mutex);
            lightmap_offered = d->lightmap;
        }
        const bool lightmap = type && !strcmp(type, "RTLightmap");
        if (lightmap && !lightmap_offered)
            throw Failure{Error::InvalidArgument, "unknown filter type (the RTLightmap filter is offered to a device with filterRTLightmap set)"};
        if (!type || (strcmp(type, "RT") && !lightmap)) throw Failure{Error::InvalidArgument, "unknown filter type (the RT filter is the one offered)"};
        f = new Filter();
        f->lightmap = lightmap;
        detail::retain(d);
        f->device = d;
    });
    return FilterRef(f);
}

BufferRef DeviceRef::newBuffer(size_t byteSize) const {
    Device *d = h.get();
    Buffer *b = nullptr;
    guard(d, [&] {
        if (!d) throw NULL_HANDLE;
        void *ptr = nullptr;
        if (byteSize) {
            const size_t rounded = (byteSize + 127) / 128 * 128;
            if (rounded < byteSize || !(ptr = aligned_alloc(128, rounded))) throw std::bad_alloc();
        }
        b = new (std::nothrow) Buffer();
        if (!b) { free(ptr); throw std::bad_alloc(); }
        b->ptr = ptr; b->size = byteSize; b->owned = true;
        detail::retain(d);
        b->device = d;
    });
    return BufferRef(b);
}

BufferRef DeviceRef::newBuffer(void *ptr, size_t byteSize) const {
    Device *d = h.get();
    Buffer *b = nullptr;
    guard(d, [&] {
        if (!d) throw NULL_HANDLE;
        if (!ptr && byteSize) throw Failure{Error::InvalidArgument, "buffer pointer null"};
        b = new Buffer();
        b->ptr = ptr; b->size = byteSize;
        detail::retain(d);
        b->device = d;
    });
    return BufferRef(b);
}

// ---- BufferRef -------------------------------------------------------------------------------------------------------------------------
void *BufferRef::getData() const { return h.get() ? h.get()->ptr : nullptr; }
size_t BufferRef::getSize() const { return h.get() ? h.get()->size : 0; }

void *BufferRef::map(Access access, size_t byteOffset, size_t byteSize) {
    (void)access;
    Buffer *b = h.get();
    void *at = nullptr;
    guard(b ? b->device : nullptr, [&] {
        if (!b) throw NULL_HANDLE;
        if (byteOffset > b->size || byteSize > b->size - byteOffset) throw Failure{Error::InvalidArgument, "buffer region out of range"};
        at = b->ptr ? static_cast<char *>(b->ptr) + byteOffset : nullptr;
    });
    return at;
}

void BufferRef::unmap(void *mappedPtr) {
    (void)mappedPtr;                 // host memory: nothing to write back
    if (!h.get()) report(nullptr, NULL_HANDLE);
}

// ---- FilterRef -------------------------------------------------------------------------------------------------------------------------
void FilterRef::setImage(const char *name, void *ptr, Format format, size_t width, size_t height, size_t byteOffset, size_t bytePixelStride,
                         size_t byteRowStride) {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f) throw NULL_HANDLE;
        const int k = image_slot(name);
        if (k < 0) throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        if (f->lightmap && (k == 1 || k == 2)) throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        ImageParam &im = f->image[k];
        im.set = ptr != nullptr;     // (a null pointer removes the image, as OIDN's does)
        im.buffer = detail::Ref<Buffer>();
        im.ptr = ptr; im.format = format; im.width = width; im.height = height;
        im.offset = byteOffset; im.pixel_stride = bytePixelStride; im.row_stride = byteRowStride;
        f->dirty = true;
    });
}

void FilterRef::setImage(const char *name, const BufferRef &buffer, Format format, size_t width, size_t height, size_t byteOffset,
                         size_t bytePixelStride, size_t byteRowStride) {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f) throw NULL_HANDLE;
        const int k = image_slot(name);
        if (k < 0 || (f->lightmap && (k == 1 || k == 2))) throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        Buffer *b = buffer.getHandle();
        if (!b) throw Failure{Error::InvalidArgument, "invalid handle"};
        {
            std::lock_guard<std::mutex> lock(f->device->mutex);
            if (f->device->images_on_device)
                throw Failure{Error::InvalidOperation, "a buffer is host memory: with imagesOnDevice set, images are device pointers"};
        }
        // the image's byte interval, from the buffer's start: [byteOffset, the last channel byte of the last pixel + 1)
        const size_t pixel = detail::formatChannels(format) * detail::formatChannelSize(format);
        if (!pixel) throw Failure{Error::InvalidArgument, "invalid image format"};
        const size_t ps = bytePixelStride ? bytePixelStride : pixel;
        const size_t rs = byteRowStride ? byteRowStride : width * ps;
        if (byteOffset > b->size) throw Failure{Error::InvalidArgument, "buffer region out of range"};
        if (width && height) {
            // (height - 1) * rs + (width - 1) * ps + pixel, refused where it overflows or leaves the buffer
            const size_t room = b->size - byteOffset;
            if (pixel > room || (width - 1) > (room - pixel) / ps) throw Failure{Error::InvalidArgument, "buffer region out of range"};
            const size_t row = (width - 1) * ps + pixel;
            if (height > 1 && (rs == 0 || (height - 1) > (room - row) / rs)) throw Failure{Error::InvalidArgument, "buffer region out of range"};
        }
        ImageParam &im = f->image[k];
        im.set = true;
        im.buffer = detail::Ref<Buffer>();
        detail::retain(b);
        im.buffer = detail::Ref<Buffer>(b);
        im.ptr = b->ptr; im.format = format; im.width = width; im.height = height;
        im.offset = byteOffset; im.pixel_stride = bytePixelStride; im.row_stride = byteRowStride;
        f->dirty = true;
    });
}

void FilterRef::setProgressMonitorFunction(ProgressMonitorFunction fn, void *userPtr) {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f) throw NULL_HANDLE;
        f->progress = fn; f->progress_user = fn ? userPtr : nullptr;      // read by execute: no commit needed
    });
}

void FilterRef::removeImage(const char *name) {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f) throw NULL_HANDLE;
        const int k = image_slot(name);
        if (k < 0) throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        f->image[k] = ImageParam();
        f->dirty = true;
    });
}

void FilterRef::setData(const char *name, void *ptr, size_t byteSize) {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f) throw NULL_HANDLE;
        if (!name || strcmp(name, "weights")) throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        f->user_weights = byteSize ? ptr : nullptr; f->user_weights_size = f->user_weights ? byteSize : 0;
        f->weights_version++;
        f->dirty = true;
    });
}

void FilterRef::updateData(const char *name) {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f) throw NULL_HANDLE;
        if (!name || strcmp(name, "weights")) throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        f->weights_version++;
        f->dirty = true;
    });
}

void FilterRef::removeData(const char *name) {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f) throw NULL_HANDLE;
        if (!name || strcmp(name, "weights")) throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        f->user_weights = nullptr; f->user_weights_size = 0;
        f->weights_version++;
        f->dirty = true;
    });
}

void FilterRef::set(const char *name, bool value) { set(name, (int)value); }

void FilterRef::set(const char *name, int value) {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f || !name) throw NULL_HANDLE;
        if (!strcmp(name, "maxMemoryMB")) f->max_memory_mb = value;
        else if (f->lightmap && !strcmp(name, "directional")) f->directional = value != 0;
        else if (f->lightmap) throw Failure{Error::InvalidArgument, "unknown filter parameter"};      // hdr, srgb, cleanAux: RTLightmapFilter::set1b has none
        else if (!strcmp(name, "hdr")) f->hdr = value != 0;
        else if (!strcmp(name, "srgb")) f->srgb = value != 0;
        else if (!strcmp(name, "cleanAux")) f->clean_aux = value != 0;
        else throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        f->dirty = true;
    });
}

void FilterRef::set(const char *name, float value) {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f || !name) throw NULL_HANDLE;
        if (!strcmp(name, "inputScale") || !strcmp(name, "hdrScale")) f->input_scale = value;
        else throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        f->dirty = true;
    });
}

bool FilterRef::get1b(const char *name) { return get1i(name) != 0; }

int FilterRef::get1i(const char *name) {
    Filter *f = h.get();
    int value = 0;
    guard(f ? f->device : nullptr, [&] {
        if (!f || !name) throw NULL_HANDLE;
        if (!strcmp(name, "maxMemoryMB")) value = f->max_memory_mb;
        else if (f->lightmap && !strcmp(name, "directional")) value = f->directional;
        else if (f->lightmap && (!strcmp(name, "hdr") || !strcmp(name, "srgb") || !strcmp(name, "cleanAux")))
            throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        else if (!strcmp(name, "hdr")) value = f->hdr;
        else if (!strcmp(name, "srgb")) value = f->srgb;
        else if (!strcmp(name, "cleanAux")) value = f->clean_aux;
        else if (!strcmp(name, "alignment")) value = PTX_NN_TILE_ALIGN;
        else if (!strcmp(name, "overlap")) value = PTX_NN_TILE_OVERLAP;
        else if (!strcmp(name, "networkBuilds")) value = f->builds;
        else throw Failure{Error::InvalidArgument, "unknown filter parameter"};
    });
    return value;
}

float FilterRef::get1f(const char *name) {
    Filter *f = h.get();
    float value = 0.f;
    guard(f ? f->device : nullptr, [&] {
        if (!f || !name) throw NULL_HANDLE;
        if (!strcmp(name, "inputScale") || !strcmp(name, "hdrScale")) value = f->input_scale;
        else if (!strcmp(name, "scale")) {
            if (!f->nn) throw Failure{Error::InvalidOperation, "no execute on this filter yet"};
            const int rc = ptx_nn_read_scale(f->nn, &value);
            if (rc != PTX_OK) throw ptx_failure(rc, "get scale");
        } else throw Failure{Error::InvalidArgument, "unknown filter parameter"};
    });
    return value;
}

void FilterRef::commit() {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f) throw NULL_HANDLE;
        commit_filter(f);
    });
}

void FilterRef::execute() {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f) throw NULL_HANDLE;
        execute_filter(f);
    });
}

}  // namespace oidn
