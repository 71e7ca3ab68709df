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
    if (rc == PTX_ERR_HIP && msg.find("out of memory") != std::string::npos) return {Error::OutOfMemory, msg};
    return {Error::Unknown, msg};
}

struct ImageParam {
    bool set = false;
    void *ptr = nullptr;
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
    bool committed = false, images_on_device = false;
    int ordinal = 0;
};

struct Filter {
    std::atomic<int> refs{1};
    Device *device = nullptr;       // retained
    ImageParam image[4];            // color, albedo, normal, output
    void *user_weights = nullptr;
    size_t user_weights_size = 0;
    unsigned long long weights_version = 0;
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

}  // namespace detail

namespace {

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
    if (!committed) throw Failure{Error::InvalidOperation, "the device is not committed"};
    const ImageParam *im = f->image;
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
    const char *name = detail::weightsName(im[0].set, im[1].set, im[2].set, f->hdr, f->srgb, f->clean_aux, &role, &why);
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
    if (!f->nn || !(key == f->key)) {
        if (key.width < 1 || key.height < 1 || key.width > PTX_NN_MAX_FRAME || key.height > PTX_NN_MAX_FRAME)
            throw Failure{Error::InvalidOperation, "unsupported image size"};
        std::vector<unsigned char> file;
        const void *blob = f->user_weights;
        size_t bytes = f->user_weights_size;
        if (!f->user_weights) {
            read_file(key.file, file);
            blob = file.data(); bytes = file.size();
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
    f->role = role;
    for (int k = 0; k < 4; k++) f->committed[k] = im[k];
    f->dirty = false;
}

void execute_filter(Filter *f) {
    if (f->dirty || !f->nn) throw Failure{Error::InvalidOperation, "changes to the filter are not committed"};
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
    if (on_device) {
        int rc = ptx_nn_denoise_images_device(f->nn, first, alb, nrm, &d[3], 1.f, f->role, &p, nullptr);
        if (rc != PTX_OK) throw ptx_failure(rc, "execute");
        float scale;
        rc = ptx_nn_read_scale(f->nn, &scale);      // waits for the handle's event
        if (rc != PTX_OK) throw ptx_failure(rc, "execute");
    } else {
        const int rc = ptx_nn_denoise_images_host(f->nn, first, alb, nrm, &d[3], 1.f, f->role, &p);
        if (rc != PTX_OK) throw ptx_failure(rc, "execute");
    }
}

}  // namespace

void setWeightsDirectory(const char *dir) {
    std::lock_guard<std::mutex> lock(g_dir_mutex);
    g_weights_dir = dir ? dir : "";
}

DeviceRef newDevice(DeviceType type) {
    (void)type;                      // Default and CPU alike: the one kind of device here is a HIP device, chosen at commit
    Device *d = new (std::nothrow) Device();
    if (!d) report(nullptr, {Error::OutOfMemory, "out of memory"});
    return DeviceRef(d);
}

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
        // (setAffinity, verbose and the like belong to OIDN's CPU device: accepted and without effect)
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
        else throw Failure{Error::InvalidArgument, "unknown device parameter"};
    });
    return value;
}

FilterRef DeviceRef::newFilter(const char *type) {
    Device *d = h.get();
    Filter *f = nullptr;
    guard(d, [&] {
        if (!d) throw NULL_HANDLE;
        if (!type || strcmp(type, "RT")) throw Failure{Error::InvalidArgument, "unknown filter type (the RT filter is the one offered)"};
        f = new Filter();
        detail::retain(d);
        f->device = d;
    });
    return FilterRef(f);
}

// ---- FilterRef -------------------------------------------------------------------------------------------------------------------------
void FilterRef::setImage(const char *name, void *ptr, Format format, size_t width, size_t height, size_t byteOffset, size_t bytePixelStride,
                         size_t byteRowStride) {
    Filter *f = h.get();
    guard(f ? f->device : nullptr, [&] {
        if (!f) throw NULL_HANDLE;
        const int k = image_slot(name);
        if (k < 0) throw Failure{Error::InvalidArgument, "unknown filter parameter"};
        ImageParam &im = f->image[k];
        im.set = ptr != nullptr;     // (a null pointer removes the image, as OIDN's does)
        im.ptr = ptr; im.format = format; im.width = width; im.height = height;
        im.offset = byteOffset; im.pixel_stride = bytePixelStride; im.row_stride = byteRowStride;
        f->dirty = true;
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
        if (!strcmp(name, "hdr")) f->hdr = value != 0;
        else if (!strcmp(name, "srgb")) f->srgb = value != 0;
        else if (!strcmp(name, "cleanAux")) f->clean_aux = value != 0;
        else if (!strcmp(name, "maxMemoryMB")) f->max_memory_mb = value;
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
        if (!strcmp(name, "hdr")) value = f->hdr;
        else if (!strcmp(name, "srgb")) value = f->srgb;
        else if (!strcmp(name, "cleanAux")) value = f->clean_aux;
        else if (!strcmp(name, "maxMemoryMB")) value = f->max_memory_mb;
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
