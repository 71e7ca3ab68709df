// pt_nn_image.hip -- the network denoiser on described images (ptx_nn_denoise_images_* of include/mi355x_pathtracer.h, "images"): float
// or half pixels at a byte offset with a byte pixel stride and a byte row stride, as OIDN's setImage describes them, and the result in
// place where the caller wants it there.  The networks are ptx_nn's (pt_nn.hip): their per-tile loop and convolutions run unchanged
// between the two end kernels here.  The descriptor's arithmetic is pt_nn_image.h's (host only); the definition is in the public
// header and restated by tests/nn_image_ref.py.
//
// Kernels (the network unit's flags, see the Makefile; -ffp-contract=off stays: every step is one IEEE fp32 operation, and the
// transfer functions are pt_nn_transfer.h's, so a packed float image gives k_nn_input's / k_nn_output's bits):
//   k_nn_image_input  : one thread per pixel of a tile's padded window: the colour (or, by role, the albedo or the normal image alone)
//       and the guides read through their descriptors, halves widened exactly, then k_nn_input's / k_nn_aux_input's steps into the
//       network's input, 16 fp16 channels per pixel (two 16-byte stores).  Thread 0 leaves the scale it used in d_scale.
//   k_nn_image_output : one thread per pixel of the rectangle a tile keeps: k_nn_output's / k_nn_aux_output's steps, then the three
//       channels written through the output's descriptor -- or into the in-place temporary, a packed float image.
//   k_nn_image_gather : one thread per pixel of the frame: the colour's three channels as floats into a W*H*3 buffer, for the meter.
//   k_nn_image_copy   : one thread per pixel of the frame: the in-place temporary through the output's descriptor.
// Loads: a 16-byte aligned float image with a pixel stride of 16 takes one 16-byte load per pixel, an 8-byte aligned half image with
// a pixel stride of 8 one 8-byte load (the fourth channel comes along and is dropped); every other layout one load per channel.
// Stores touch the three channels alone: three 4-byte stores, or for halves three 2-byte stores (a 4-byte and a 2-byte one where the
// pixels are 4-byte aligned).  A half is fp16_rne(v > 65504 ? 65504 : v).  No atomics, no LDS, no scratch.
// (The view, its loads and its stores are pt_nn_image_dev.h's, shared with pt_nn_lightmap.hip, which also launches the gather and the
// copy through the host functions at the end of this unit and stages host images through pt_nn_image_host_call.)
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>

#include "pt_nn.h"
#include "pt_nn_image.h"
#include "pt_nn_image_dev.h"
#include "pt_nn_transfer.h"
#include "pt_display.h"

namespace {

using namespace pt_nn_transfer;

constexpr int NT = 256;

struct ImgInputArgs {
    int w, h, wp, hp;                         // the window and its padded size
    int x0, y0;                               // the window's origin in the frame
    Img col, alb, nrm;                        // col: the role's image
    int role;
    float samples, scale;
    const float *scale_ptr;                   // NULL: `scale`
    float *scale_out;
    int mode, hdr;
    float norm;
    uint16_t *out;                            // [hp][wp][16] fp16
};

__global__ __launch_bounds__(NT) void k_nn_image_input(ImgInputArgs a) {
    const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
    const float s = a.scale_ptr ? *a.scale_ptr : a.scale;
    if (idx == 0) *a.scale_out = s;
    if (idx >= (size_t)a.wp * a.hp) return;
    const int y = (int)(idx / a.wp), x = (int)(idx - (size_t)y * a.wp);
    float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (x < a.w && y < a.h) {
        const size_t fx = (size_t)a.x0 + x, fy = (size_t)a.y0 + y;
        float in[3];
        load3(a.col, fx, fy, in);
#pragma unroll
        for (int c = 0; c < 3; c++)
            v[c] = a.role == PTX_NN_ROLE_NORMAL ? sanitise(in[c] * s, -1.f, 1.f) * 0.5f + 0.5f
                                                : transfer_forward(sanitise((in[c] / a.samples) * s, 0.f, a.hdr ? FLT_MAX : 1.f), a.mode, a.norm);
        if (a.alb.base) {
            load3(a.alb, fx, fy, in);
#pragma unroll
            for (int c = 0; c < 3; c++) v[3 + c] = sanitise(in[c], 0.f, 1.f);
        }
        if (a.nrm.base) {
            load3(a.nrm, fx, fy, in);
#pragma unroll
            for (int c = 0; c < 3; c++) v[6 + c] = sanitise(in[c], -1.f, 1.f) * 0.5f + 0.5f;
        }
    }
    half8 lo, hi = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 8; c++) lo[c] = (_Float16)v[c];
    hi[0] = (_Float16)v[8];
    half8 *o = reinterpret_cast<half8 *>(a.out) + 2 * idx;
    o[0] = lo; o[1] = hi;
}

struct ImgOutputArgs {
    int w, h, wp;                             // the rectangle kept; the tile's padded width
    int ix, iy;                               // where the rectangle begins in the tile's output
    int ox, oy;                               // ... and in the frame
    const float *net;                         // [hp][wp][4] fp32
    const float *scale;
    int role, mode, hdr;
    float xmax;
    Img out;
};

__global__ __launch_bounds__(NT) void k_nn_image_output(ImgOutputArgs a) {
    const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= (size_t)a.w * a.h) return;
    const int y = (int)(idx / a.w), x = (int)(idx - (size_t)y * a.w);
    const float s = *a.scale, inv = s != 0.f ? 1.f / s : 0.f;
    const float4 n = reinterpret_cast<const float4 *>(a.net)[((size_t)a.iy + y) * a.wp + a.ix + x];
    const float in[3] = {n.x, n.y, n.z};
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v = sanitise(in[c], 0.f, FLT_MAX);
        if (a.role == PTX_NN_ROLE_NORMAL) {
            v = v * 2.0f - 1.0f;
            v = fmaxf(v, -1.f);
            v = fminf(v, 1.f);
        } else {
            v = transfer_inverse(v, a.mode, a.xmax);
            if (!a.hdr) v = fminf(v, 1.f);
        }
        r[c] = v * inv;
    }
    store3(a.out, (size_t)a.ox + x, (size_t)a.oy + y, r);
}

struct ImgFrameArgs {
    int w, h;
    Img img;
    float *packed;                            // [h][w][3]
};

__global__ __launch_bounds__(NT) void k_nn_image_gather(ImgFrameArgs a) {
    const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= (size_t)a.w * a.h) return;
    const size_t y = idx / a.w, x = idx - y * a.w;
    float v[3];
    load3(a.img, x, y, v);
    a.packed[3 * idx] = v[0]; a.packed[3 * idx + 1] = v[1]; a.packed[3 * idx + 2] = v[2];
}

__global__ __launch_bounds__(NT) void k_nn_image_copy(ImgFrameArgs a) {
    const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= (size_t)a.w * a.h) return;
    const size_t y = idx / a.w, x = idx - y * a.w;
    const float v[3] = {a.packed[3 * idx], a.packed[3 * idx + 1], a.packed[3 * idx + 2]};
    store3(a.img, x, y, v);
}

template <class K, class A> int launch(K kernel, hipStream_t st, size_t n, const A &a) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, a);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

const char *const IMAGE_NAME[4] = {"colour", "albedo", "normal", "output"};
const char *const ROLE_NAME[3] = {"colour", "albedo", "normal"};

bool given(const ptx_nn_image *img) { return img && img->ptr; }

// What a call refuses without a device, in the public header's order: the params, the role's rules, the formats; then, with a handle,
// the images its network takes and each descriptor.  v[k]: the views of colour, albedo, normal, output.
int images_problem(const char *fn_, ptx_nn *n, const ptx_nn_image *const img[4], float samples, int role, const ptx_nn_params &p, PtNnImageView v[4]) {
    const std::string fn = fn_;
    if (const char *why = pt_nn_params_problem(p, samples)) return pt_fail(PTX_ERR_INVALID, fn + ": " + why);
    if (role != PTX_NN_ROLE_COLOR && role != PTX_NN_ROLE_ALBEDO && role != PTX_NN_ROLE_NORMAL)
        return pt_fail(PTX_ERR_INVALID, fn + ": role must be PTX_NN_ROLE_COLOR, PTX_NN_ROLE_ALBEDO or PTX_NN_ROLE_NORMAL");
    if (role != PTX_NN_ROLE_COLOR) {
        const std::string who = fn + ": the " + ROLE_NAME[role] + " role ";
        if (p.hdr) return pt_fail(PTX_ERR_INVALID, who + "is refused with hdr != 0 (a prefilter has no hdr mode)");
        if (samples != 1.f) return pt_fail(PTX_ERR_INVALID, who + "is refused with samples != 1 (the image is not an accumulation)");
        if (role == PTX_NN_ROLE_NORMAL && p.srgb) return pt_fail(PTX_ERR_INVALID, who + "is refused with srgb != 0 (a normal image has no transfer curve)");
        if (!isnan(p.input_scale) && !(p.input_scale > 0.f)) return pt_fail(PTX_ERR_INVALID, who + "needs an input_scale that is NaN (1) or > 0");
    }
    int input_format = 0;
    for (int k = 0; k < 4; k++) {
        if (!given(img[k])) continue;
        if (!pt_nn_image_channel(img[k]->format))
            return pt_fail(PTX_ERR_INVALID, fn + ": the " + IMAGE_NAME[k] + " image: unknown format " + std::to_string(img[k]->format) +
                                                " (PTX_NN_FORMAT_FLOAT3 = 1, PTX_NN_FORMAT_HALF3 = 2)");
        if (k == 3) break;
        if (input_format && img[k]->format != input_format)
            return pt_fail(PTX_ERR_INVALID, fn + ": mixed input formats: the " + IMAGE_NAME[k] + " image's differs from the colour image's "
                                                 "(the inputs are all Float3 or all Half3; the output may be either)");
        if (!input_format) input_format = img[k]->format;
    }
    if (!n || !given(img[0]) || !given(img[3])) return pt_fail(PTX_ERR_INVALID, fn + ": null handle, colour image or output image");
    if (role != PTX_NN_ROLE_COLOR && n->ic != 3)
        return pt_fail(PTX_ERR_INVALID, fn + ": the " + ROLE_NAME[role] + " role is refused on weights that take " + std::to_string(n->ic) +
                                            " input channels: it is a 3-input network's single image");
    if (given(img[1]) != (n->ic >= 6))
        return pt_fail(PTX_ERR_INVALID, fn + ": the weights take " + std::to_string(n->ic) + " input channels: albedo " + (n->ic >= 6 ? "is required" : "must be NULL"));
    if (given(img[2]) != (n->ic >= 9))
        return pt_fail(PTX_ERR_INVALID, fn + ": the weights take " + std::to_string(n->ic) + " input channels: normals " + (n->ic >= 9 ? "are required" : "must be NULL"));
    for (int k = 0; k < 4; k++) {
        v[k] = PtNnImageView();
        if (!given(img[k])) continue;
        const std::string why = pt_nn_image_view(n->w, n->h, *img[k], v[k]);
        if (!why.empty()) return pt_fail(PTX_ERR_INVALID, fn + ": the " + IMAGE_NAME[k] + " image: " + why);
    }
    return PTX_OK;
}

int mode_of(int role, const ptx_nn_params &p) { return role == PTX_NN_ROLE_NORMAL ? MODE_LINEAR : p.hdr ? MODE_PU : p.srgb ? MODE_LINEAR : MODE_SRGB; }

struct Ends { ImgInputArgs ia; ImgOutputArgs oa; };

// One denoise on st of checked views on the handle's device; the device is set.
int images_enqueue(ptx_nn *n, hipStream_t st, const PtNnImageView v[4], float samples, int role, const ptx_nn_params &p) {
    const bool automatic = isnan(p.input_scale) && p.hdr;
    if (automatic && !n->meter)
        if (const int rc = ptx_display_create(n->device, n->w, n->h, &n->meter)) {
            if (rc == PTX_ERR_INVALID && (n->w > PTX_NN_MAX_WIDTH || n->h > PTX_NN_MAX_HEIGHT))
                return pt_fail(rc, "the network denoiser's automatic hdr scale is refused at " + std::to_string(n->w) + " x " + std::to_string(n->h) +
                                       ": the display handle that meters the frame refuses this size (give ptx_nn_params.input_scale)");
            return rc;
        }
    // In place.  The output's interval meets no input's: every tile writes the output itself.  It meets one and there is one tile: the
    // same -- every read of the input stage (and of the gather) precedes every write of the output stage on the stream.  It meets one
    // and there are more tiles: a later tile's window would read what an earlier tile's result replaced, so the tiles write a packed
    // float temporary, which k_nn_image_copy moves through the output's descriptor after the last tile.
    const bool staged = pt_nn_image_staged(n, v);
    const size_t count = 3 * (size_t)n->w * n->h;
    const bool gather = automatic && !is_packed_float(v[0], n->w);
    PT_HC(n->wait_stream(st));
    if (staged && !n->d_image_tmp) PT_HC(n->d_image_tmp.alloc(count));      // (beside the activation scratch, outside max_memory_mb)
    if (gather && !n->d_image_gather) PT_HC(n->d_image_gather.alloc(count));

    Ends e;
    ImgInputArgs &ia = e.ia;
    ia.col = device_image(v[0]); ia.alb = device_image(v[1]); ia.nrm = device_image(v[2]);
    ia.role = role;
    ia.samples = samples; ia.scale = isnan(p.input_scale) ? 1.f : p.input_scale;
    ia.scale_ptr = nullptr;
    if (automatic) {
        const float *rgb = reinterpret_cast<const float *>(v[0].base);
        if (gather) {
            if (const int rc = pt_nn_image_gather_enqueue(st, n->w, n->h, v[0], n->d_image_gather)) return rc;
            rgb = n->d_image_gather;
        }
        if (const int rc = pt_display_meter_enqueue(n->meter, st, rgb, samples, 0.18f)) return rc;
        ia.scale_ptr = &n->meter->d_state.p->metered;
    }
    ia.scale_out = n->d_scale;
    ia.mode = mode_of(role, p); ia.hdr = p.hdr; ia.norm = pu_norm();
    ImgOutputArgs &oa = e.oa;
    oa.scale = n->d_scale; oa.role = role; oa.mode = ia.mode; oa.hdr = p.hdr; oa.xmax = pu_xmax();
    oa.out = device_image(staged ? packed_view(n->d_image_tmp, n->w) : v[3]);

    PtNnStages stages;
    stages.ctx = &e;
    stages.input = [](void *ctx, hipStream_t s, const ptx_nn_tile &T, int wp, int hp, uint16_t *net_in) {
        ImgInputArgs a = static_cast<Ends *>(ctx)->ia;
        a.w = T.w; a.h = T.h; a.wp = wp; a.hp = hp; a.x0 = T.x; a.y0 = T.y; a.out = net_in;
        return launch(k_nn_image_input, s, (size_t)wp * hp, a);
    };
    stages.output = [](void *ctx, hipStream_t s, const ptx_nn_tile &T, int wp, const float *net_out) {
        ImgOutputArgs a = static_cast<Ends *>(ctx)->oa;
        a.w = T.out_w; a.h = T.out_h; a.wp = wp; a.net = net_out;
        a.ix = T.out_x - T.x; a.iy = T.out_y - T.y; a.ox = T.out_x; a.oy = T.out_y;
        return launch(k_nn_image_output, s, (size_t)T.out_w * T.out_h, a);
    };
    if (const int rc = pt_nn_run_tiles(n, st, stages)) return rc;
    if (staged) {
        if (const int rc = pt_nn_image_copy_enqueue(st, n->w, n->h, n->d_image_tmp, v[3])) return rc;
        if (const int rc = pt_nn_progress_frame_unit(n, st)) return rc;
    }
    PT_HC(n->record(st));
    return PTX_OK;
}

ptx_nn_params params_or_default(const ptx_nn_params *given_params) {
    ptx_nn_params p;
    if (given_params) p = *given_params;
    else ptx_default_nn_params(&p);
    return p;
}

// a staging buffer of at least `bytes`; the handle's last work is over (the caller has waited)
hipError_t ensure(DevBuf<uint8_t> &b, size_t bytes) {
    if (b.p && b.n >= bytes) return hipSuccess;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.n = 0; }
    return b.alloc(bytes);
}

}  // namespace

int pt_nn_image_gather_enqueue(hipStream_t st, int w, int h, const PtNnImageView &img, float *packed) {
    ImgFrameArgs a;
    a.w = w; a.h = h; a.img = device_image(img); a.packed = packed;
    return launch(k_nn_image_gather, st, (size_t)w * h, a);
}

int pt_nn_image_copy_enqueue(hipStream_t st, int w, int h, const float *packed, const PtNnImageView &img) {
    ImgFrameArgs a;
    a.w = w; a.h = h; a.img = device_image(img); a.packed = const_cast<float *>(packed);
    return launch(k_nn_image_copy, st, (size_t)w * h, a);
}

bool pt_nn_image_staged(const ptx_nn *n, const PtNnImageView v[4]) {
    uintptr_t olo, ohi;
    pt_nn_image_interval(v[3], n->w, n->h, olo, ohi);
    bool meets = false;
    for (int k = 0; k < 3; k++) {
        if (!v[k].base) continue;
        uintptr_t lo, hi;
        pt_nn_image_interval(v[k], n->w, n->h, lo, hi);
        meets = meets || pt_nn_intervals_meet(olo, ohi, lo, hi);
    }
    return meets && n->tiling.count() > 1;
}

// the staging between pt_nn_image_host_call's first report and its end
static int host_call_staged(ptx_nn *n, const PtNnImageView v[4], int (*enqueue)(void *ctx, ptx_nn *n, const PtNnImageView d[4]), void *ctx) {
    // Each image's interval in a buffer of its own, but the inputs whose interval meets the output's: those go up with it, in one
    // buffer that spans them, so that images which share bytes in the caller's memory share them on the device.  A device address keeps
    // the host address's residue mod 16: the same alignment, the same loads and stores.
    uintptr_t lo[4] = {}, hi[4] = {};
    for (int k = 0; k < 4; k++)
        if (v[k].base) pt_nn_image_interval(v[k], n->w, n->h, lo[k], hi[k]);
    uintptr_t span_lo = lo[3], span_hi = hi[3];
    bool with_output[3] = {false, false, false};
    for (int k = 0; k < 3; k++)
        if (v[k].base && pt_nn_intervals_meet(lo[3], hi[3], lo[k], hi[k])) {
            with_output[k] = true;
            span_lo = std::min(span_lo, lo[k]); span_hi = std::max(span_hi, hi[k]);
        }
    PtNnImageView d[4];
    PT_HC(ensure(n->d_image_stage[3], (size_t)(span_hi - span_lo) + 16));
    uint8_t *span = n->d_image_stage[3].p + (span_lo & 15);
    PT_HC(hipMemcpy(span, reinterpret_cast<const void *>(span_lo), (size_t)(span_hi - span_lo), hipMemcpyHostToDevice));
    for (int k = 0; k < 4; k++) {
        d[k] = v[k];
        if (!v[k].base) continue;
        if (k == 3 || with_output[k]) {
            d[k].base = (uintptr_t)span + (v[k].base - span_lo);
            continue;
        }
        PT_HC(ensure(n->d_image_stage[k], (size_t)(hi[k] - lo[k]) + 16));
        uint8_t *at = n->d_image_stage[k].p + (lo[k] & 15);
        PT_HC(hipMemcpy(at, reinterpret_cast<const void *>(lo[k]), (size_t)(hi[k] - lo[k]), hipMemcpyHostToDevice));
        d[k].base = (uintptr_t)at;
    }
    if (const int rc = enqueue(ctx, n, d)) return rc;
    PT_HC(hipEventSynchronize(n->ev));
    PT_HC(hipMemcpy(reinterpret_cast<void *>(lo[3]), span + (lo[3] - span_lo), (size_t)(hi[3] - lo[3]), hipMemcpyDeviceToHost));
    return PTX_OK;
}

int pt_nn_image_host_call(const char *fn, ptx_nn *n, const PtNnImageView v[4], int (*enqueue)(void *ctx, ptx_nn *n, const PtNnImageView d[4]), void *ctx) {
    PT_HC(n->wait_host());
    bool mine;
    if (const int rc = pt_nn_progress_begin(fn, n, pt_nn_image_staged(n, v), &mine)) return rc;
    return pt_nn_progress_end(n, mine, host_call_staged(n, v, enqueue, ctx));
}

extern "C" {

size_t ptx_sizeof_nn_image(void) { return sizeof(ptx_nn_image); }

int ptx_debug_nn_image_problem(int width, int height, const ptx_nn_image *img, int is_output) {
    const std::string fn = "ptx_debug_nn_image_problem";
    if (width < 1 || height < 1 || width > PTX_NN_MAX_FRAME || height > PTX_NN_MAX_FRAME) return pt_fail(PTX_ERR_INVALID, fn + ": bad frame size");
    if (!img || !img->ptr) return pt_fail(PTX_ERR_INVALID, fn + ": no image (a NULL descriptor or ptr)");
    PtNnImageView v;
    const std::string why = pt_nn_image_view(width, height, *img, v);
    if (!why.empty()) return pt_fail(PTX_ERR_INVALID, fn + ": the " + (is_output ? "output" : "input") + " image: " + why);
    return PTX_OK;
}

int ptx_nn_denoise_images_device(ptx_nn *n, const ptx_nn_image *color, const ptx_nn_image *albedo, const ptx_nn_image *normal,
                                 const ptx_nn_image *output, float samples, int role, const ptx_nn_params *params, void *stream) {
    const ptx_nn_params p = params_or_default(params);
    const ptx_nn_image *const img[4] = {color, albedo, normal, output};
    PtNnImageView v[4];
    if (const int rc = images_problem("ptx_nn_denoise_images_device", n, img, samples, role, p, v)) return rc;
    PT_HC(hipSetDevice(n->device));
    bool mine;
    if (const int rc = pt_nn_progress_begin("ptx_nn_denoise_images_device", n, pt_nn_image_staged(n, v), &mine)) return rc;
    return pt_nn_progress_end(n, mine, images_enqueue(n, (hipStream_t)stream, v, samples, role, p));
}

int ptx_nn_denoise_images_host(ptx_nn *n, const ptx_nn_image *color, const ptx_nn_image *albedo, const ptx_nn_image *normal,
                               const ptx_nn_image *output, float samples, int role, const ptx_nn_params *params) {
    const ptx_nn_params p = params_or_default(params);
    const ptx_nn_image *const img[4] = {color, albedo, normal, output};
    PtNnImageView v[4];
    if (const int rc = images_problem("ptx_nn_denoise_images_host", n, img, samples, role, p, v)) return rc;
    PT_HC(hipSetDevice(n->device));
    struct Call { float samples; int role; ptx_nn_params p; } c = {samples, role, p};
    return pt_nn_image_host_call("ptx_nn_denoise_images_host", n, v, [](void *ctx, ptx_nn *h, const PtNnImageView d[4]) {
        const Call &k = *static_cast<Call *>(ctx);
        return images_enqueue(h, nullptr, d, k.samples, k.role, k.p);
    }, &c);
}

}  // extern "C"
