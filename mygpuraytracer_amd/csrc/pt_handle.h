// pt_handle.h -- what the host units build their state from: the ptx_last_error of a failed call and the checked HIP call (of every
// unit that calls HIP), the owned device array (DevBuf: the tracer's buffers, pt_tracer.h, and the handles'), the owned event and stream (OwnedEvent,
// OwnedStream: the tracer's and the handles') with the timed region made of two such events, and the base of the six post-processing
// handles (PtHandle: ptx_temporal and ptx_moments, pt_denoise.h; ptx_adaptive, pt_adaptive.h; ptx_display, pt_display.h; ptx_nn and
// ptx_nn_prefilter, pt_nn.h)
// with their one create and destroy path.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

#include "../../include/mi355x_pathtracer.h"

extern "C" void ptx_internal_set_error(const char *msg);
inline int pt_fail(int code, const std::string &msg) { ptx_internal_set_error(msg.c_str()); return code; }
#define PT_HC(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return pt_fail(PTX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

// An owned device array -- every device buffer of the tracer and of a handle, the scratch of the per-stage entry points -- freed when its
// owner goes, on every way out (a PT_HC that fails returns from the middle).  Each step hands back the hipError_t: ptx_create looks for
// out-of-memory.
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;                              // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    operator T *() const { return p; }
    hipError_t alloc(size_t count) { n = count; return hipMalloc(&p, sizeof(T) * count); }      // (once per buffer; contents undefined)
    hipError_t zero() { return hipMemset(p, 0, sizeof(T) * n); }
    hipError_t upload(const void *src, size_t count) { const hipError_t e = alloc(count); return e != hipSuccess ? e : hipMemcpy(p, src, sizeof(T) * count, hipMemcpyHostToDevice); }
    hipError_t upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
    hipError_t download(void *dst) const { return hipMemcpy(dst, p, sizeof(T) * n, hipMemcpyDeviceToHost); }
};

// The one owner of a HIP object that is a handle with a destroy call of its own -- an event, a stream.  Empty, made (`make`, `adopt`:
// destroyed when the owner goes, once) or a caller's (`borrow`: never destroyed).  `Destroy` is a parameter, so that a host-only check
// counts the calls of a fake one (tests/hip_owned_check.cpp).  Moves for a std::vector that grows; no copies.
template <class H, auto Destroy> struct Owned {
    H h{};
    bool own = false;
    Owned() = default;
    Owned(const Owned &) = delete; Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h(o.h), own(o.own) { o.h = H{}; o.own = false; }
    ~Owned() { reset(); }
    operator H() const { return h; }
    void adopt(H made) { reset(); h = made; own = true; }
    void borrow(H theirs) { reset(); h = theirs; }
    void reset() { if (own) (void)Destroy(h); h = H{}; own = false; }
    // what `create(&handle, args...)` makes; hands back its hipError_t, as DevBuf's steps do
    template <class Create, class... A> hipError_t make(Create create, A... args) { H made{}; const hipError_t e = create(&made, args...); if (e == hipSuccess) adopt(made); return e; }
};
struct OwnedEvent : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { return make(hipEventCreateWithFlags, flags); }
};
struct OwnedStream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags, int priority) { return make(hipStreamCreateWithPriority, flags, priority); }
};

// A timed region of one stream: begin() makes two events and records the first, end() records the second, waits for it and hands back
// the milliseconds between them.  Both events go with the region, on every way out.
struct TimedRegion {
    OwnedEvent e0, e1;
    hipStream_t st = nullptr;
    hipError_t begin(hipStream_t stream) { st = stream; hipError_t e = e0.create(); if (e == hipSuccess) e = e1.create(); return e != hipSuccess ? e : hipEventRecord(e0, st); }
    hipError_t end(float *ms) { hipError_t e = hipEventRecord(e1, st); if (e == hipSuccess) e = hipEventSynchronize(e1); return e != hipSuccess ? e : hipEventElapsedTime(ms, e0, e1); }
};

// A post-processing handle: made for one device and one frame size, its buffers DevBuf members of the struct that derives from this,
// and one event, which is its whole order with the streams it is used on.  Every call that enqueues work with the handle first makes
// its stream (or the host) wait for the handle's last work, and records the event behind its own.
struct PtHandle {
    int device = 0, w = 0, h = 0;
    OwnedEvent ev;                        // recorded after each call's work (on that call's stream); goes after the derived struct's buffers
    bool used = false;                    // ev was recorded
    PtHandle() = default;
    PtHandle(const PtHandle &) = delete; PtHandle &operator=(const PtHandle &) = delete;
    hipError_t wait_host() const { return used ? hipEventSynchronize(ev) : hipSuccess; }
    // what is enqueued on st next runs after the handle's last work, maybe on another stream
    hipError_t wait_stream(hipStream_t st) const { return used ? hipStreamWaitEvent(st, ev, 0) : hipSuccess; }
    // the handle's event behind what st holds so far, for the next call on the handle to wait for
    hipError_t record(hipStream_t st) {
        const hipError_t e = hipEventRecord(ev, st);
        if (e == hipSuccess) used = true;
        return e;
    }
};

// What ptx_<handle>_create (`fn`) refuses before anything is allocated, in this order: no `out`, a size that is no frame or above the
// unit's own cap of `max_pixels`, an ordinal below 0, no device at all (`noun`: the handle as that message names it), an ordinal at or
// above the device count.  PTX_OK: `device` is a device.
inline int pt_handle_create_problem(const char *fn, const char *noun, int device, int width, int height, long long max_pixels, const void *out) {
    const std::string name = fn;
    if (!out) return pt_fail(PTX_ERR_INVALID, name + ": out is NULL");
    if (width < 1 || height < 1 || (long long)width * height > max_pixels) return pt_fail(PTX_ERR_INVALID, name + ": bad frame size");
    if (device < 0) return pt_fail(PTX_ERR_INVALID, name + ": device ordinal out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return pt_fail(PTX_ERR_NODEVICE, std::string("no HIP device available; ") + noun + " has no CPU path");
    }
    if (device >= ndev) return pt_fail(PTX_ERR_INVALID, name + ": device ordinal out of range");
    return PTX_OK;
}

// ptx_<handle>_create: the checks above, then `alloc` on a handle that knows its device and size (it sets the device, allocates what
// is not left to a first use and creates the event).  *out is the handle, or NULL after every refusal and failure.
template <class H> int pt_handle_create(const char *fn, const char *noun, int device, int width, int height, long long max_pixels, H **out,
                                        int (*alloc)(H *)) {
    if (out) *out = nullptr;
    if (const int rc = pt_handle_create_problem(fn, noun, device, width, height, max_pixels, out)) return rc;
    H *x = new H();
    x->device = device; x->w = width; x->h = height;
    const int rc = alloc(x);
    if (rc != PTX_OK) { delete x; return rc; }
    *out = x;
    return PTX_OK;
}

// ptx_<handle>_destroy: after the handle's last work
template <class H> void pt_handle_destroy(H *x) {
    if (!x) return;
    (void)hipSetDevice(x->device);
    (void)x->wait_host();
    delete x;
}
