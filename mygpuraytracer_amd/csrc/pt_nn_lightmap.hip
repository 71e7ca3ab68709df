// pt_nn_lightmap.hip -- OIDN's RTLightmap filter on the device (ptx_nn_denoise_lightmap_* of include/mi355x_pathtracer.h, "lightmap"): a
// 3-input network of ptx_nn (pt_nn.hip) between the two end kernels here, on described images (pt_nn_image.h) with pt_nn_image.hip's
// rules, staging and in-place behaviour.  The per-tile loop and the convolutions run unchanged (pt_nn_run_tiles); the gather for the
// meter and the in-place copy-out are pt_nn_image.hip's kernels, launched through its host functions (pt_nn_image_dev.h).  The
// definition is in the public header and restated by tests/nn_lightmap_ref.py.
//
// Kernels (the network unit's flags, see the Makefile; -ffp-contract=off stays: every step is one IEEE fp32 operation, logf and expf the
// correctly rounded ones, see logf_rn / expf_rn):
//   k_nn_lightmap_input  : one thread per pixel of a tile's padded window: the colour read through its descriptor, halves widened
//       exactly, then HDR: logf(clamp(v * s, 0, FLT_MAX) + 1) * norm, or directional: clamp(v * s, -1, 1) * 0.5 + 0.5 -- the normal
//       role's steps of k_nn_image_input -- into the network's input, 16 fp16 channels per pixel (two 16-byte stores), 3 of them used.
//       Thread 0 leaves the scale it used in d_scale.
//   k_nn_lightmap_output : one thread per pixel of the rectangle a tile keeps: HDR: (expf(clamp(x, 0, FLT_MAX) * xmax) - 1) / s, or
//       directional: the normal role's steps of k_nn_image_output; then the three channels through the output's descriptor -- or into
//       the in-place temporary, a packed float image.
// The Log functions are this unit's own: pt_nn_transfer.h's transfer_forward / transfer_inverse are not touched.  Loads and stores are
// pt_nn_image_dev.h's.  No atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string>

#include "pt_nn.h"
#include "pt_nn_image.h"
#include "pt_nn_image_dev.h"
#include "pt_nn_lightmap.h"
#include "pt_nn_transfer.h"
#include "pt_display.h"

namespace {

using pt_nn_transfer::sanitise;

constexpr int NT = 256;

// logf and expf as IEEE 754 recommends them, correctly rounded: formed in double and rounded once.  The library's logf / expf are good
// to an ulp, which is not enough here: near 0 the inverse is expf(a) - 1 with expf(a) just above 1, so an ulp of expf is 2^-23 absolute in
// the result whatever its size, twice the 2^-24 that the rounding of the correctly rounded value costs (and that the tests allow).  The
// restatement forms them the same way, so it gives these bits.  Per pixel six such calls; the sixteen convolutions dwarf them.
__device__ __forceinline__ float logf_rn(float v) { return (float)log((double)v); }
__device__ __forceinline__ float expf_rn(float v) { return (float)exp((double)v); }

// OIDN's Log transfer function (core/color.ispc, LogTransferFunc) with its normalisation: four fp32 operations each way
__device__ __forceinline__ float log_forward(float y, float norm) { return logf_rn(y + 1.f) * norm; }
__device__ __forceinline__ float log_inverse(float x, float xmax) { return expf_rn(x * xmax) - 1.f; }

struct LmInputArgs {
    int w, h, wp, hp;                         // the window and its padded size
    int x0, y0;                               // the window's origin in the frame
    Img col;
    int directional;
    float scale;
    const float *scale_ptr;                   // NULL: `scale`
    float *scale_out;
    float norm;
    uint16_t *out;                            // [hp][wp][16] fp16
};

__global__ __launch_bounds__(NT) void k_nn_lightmap_input(LmInputArgs a) {
    const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
    const float s = a.scale_ptr ? *a.scale_ptr : a.scale;
    if (idx == 0) *a.scale_out = s;
    if (idx >= (size_t)a.wp * a.hp) return;
    const int y = (int)(idx / a.wp), x = (int)(idx - (size_t)y * a.wp);
    float v[3] = {0.f, 0.f, 0.f};
    if (x < a.w && y < a.h) {
        float in[3];
        load3(a.col, (size_t)a.x0 + x, (size_t)a.y0 + y, in);
#pragma unroll
        for (int c = 0; c < 3; c++)
            v[c] = a.directional ? sanitise(in[c] * s, -1.f, 1.f) * 0.5f + 0.5f : log_forward(sanitise(in[c] * s, 0.f, FLT_MAX), a.norm);
    }
    half8 lo = {0, 0, 0, 0, 0, 0, 0, 0};
    const half8 hi = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; c++) lo[c] = (_Float16)v[c];
    half8 *o = reinterpret_cast<half8 *>(a.out) + 2 * idx;
    o[0] = lo; o[1] = hi;
}

struct LmOutputArgs {
    int w, h, wp;                             // the rectangle kept; the tile's padded width
    int ix, iy;                               // where the rectangle begins in the tile's output
    int ox, oy;                               // ... and in the frame
    const float *net;                         // [hp][wp][4] fp32
    const float *scale;
    int directional;
    float xmax;
    Img out;
};

__global__ __launch_bounds__(NT) void k_nn_lightmap_output(LmOutputArgs a) {
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
        if (a.directional) {
            v = v * 2.0f - 1.0f;
            v = fmaxf(v, -1.f);
            v = fminf(v, 1.f);
        } else {
            v = log_inverse(v, a.xmax);
        }
        r[c] = v * inv;
    }
    store3(a.out, (size_t)a.ox + x, (size_t)a.oy + y, r);
}

template <class K, class A> int launch(K kernel, hipStream_t st, size_t n, const A &a) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, a);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

bool given(const ptx_nn_image *img) { return img && img->ptr; }

// What a call refuses, in the public header's order: without a device the two scalars and the formats; then, with a handle, the blob's
// input count and each descriptor.  v: the views of colour, -, -, output (pt_nn_image.hip's order).
int lightmap_problem(const char *fn_, ptx_nn *n, const ptx_nn_image *color, const ptx_nn_image *output, int directional, float input_scale,
                     PtNnImageView v[4]) {
    const std::string fn = fn_;
    if (const char *why = pt_nn_lightmap::args_problem(directional, input_scale)) return pt_fail(PTX_ERR_INVALID, fn + ": " + why);
    const ptx_nn_image *const img[2] = {color, output};
    const char *const name[2] = {"colour", "output"};
    for (int k = 0; k < 2; k++)
        if (given(img[k]) && !pt_nn_image_channel(img[k]->format))
            return pt_fail(PTX_ERR_INVALID, fn + ": the " + name[k] + " image: unknown format " + std::to_string(img[k]->format) +
                                                " (PTX_NN_FORMAT_FLOAT3 = 1, PTX_NN_FORMAT_HALF3 = 2)");
    if (!n || !given(color) || !given(output)) return pt_fail(PTX_ERR_INVALID, fn + ": null handle, colour image or output image");
    if (n->ic != 3)
        return pt_fail(PTX_ERR_INVALID, fn + ": the weights take " + std::to_string(n->ic) + " input channels: a lightmap network takes the colour alone (3)");
    for (int k = 0; k < 4; k++) v[k] = PtNnImageView();
    for (int k = 0; k < 2; k++) {
        const std::string why = pt_nn_image_view(n->w, n->h, *img[k], v[k ? 3 : 0]);
        if (!why.empty()) return pt_fail(PTX_ERR_INVALID, fn + ": the " + name[k] + " image: " + why);
    }
    return PTX_OK;
}

struct Ends { LmInputArgs ia; LmOutputArgs oa; };

// One denoise on st of checked views on the handle's device; the device is set.  pt_nn_image.hip's images_enqueue with this unit's ends.
int lightmap_enqueue(ptx_nn *n, hipStream_t st, const PtNnImageView v[4], int directional, float input_scale) {
    const bool automatic = isnan(input_scale) && !directional;
    if (automatic && !n->meter)
        if (const int rc = ptx_display_create(n->device, n->w, n->h, &n->meter)) {
            if (rc == PTX_ERR_INVALID && (n->w > PTX_NN_MAX_WIDTH || n->h > PTX_NN_MAX_HEIGHT))
                return pt_fail(rc, "the lightmap filter's automatic scale is refused at " + std::to_string(n->w) + " x " + std::to_string(n->h) +
                                       ": the display handle that meters the frame refuses this size (give input_scale)");
            return rc;
        }
    const bool staged = pt_nn_image_staged(n, v);                              // in place under several tiles: see pt_nn_image.hip
    const size_t count = 3 * (size_t)n->w * n->h;
    const bool gather = automatic && !is_packed_float(v[0], n->w);
    PT_HC(n->wait_stream(st));
    if (staged && !n->d_image_tmp) PT_HC(n->d_image_tmp.alloc(count));
    if (gather && !n->d_image_gather) PT_HC(n->d_image_gather.alloc(count));

    Ends e;
    LmInputArgs &ia = e.ia;
    ia.col = device_image(v[0]);
    ia.directional = directional;
    ia.scale = isnan(input_scale) ? 1.f : input_scale;
    ia.scale_ptr = nullptr;
    if (automatic) {
        const float *rgb = reinterpret_cast<const float *>(v[0].base);
        if (gather) {
            if (const int rc = pt_nn_image_gather_enqueue(st, n->w, n->h, v[0], n->d_image_gather)) return rc;
            rgb = n->d_image_gather;
        }
        if (const int rc = pt_display_meter_enqueue(n->meter, st, rgb, 1.f, 0.18f)) return rc;
        ia.scale_ptr = &n->meter->d_state.p->metered;
    }
    ia.scale_out = n->d_scale;
    ia.norm = pt_nn_lightmap::log_norm();
    LmOutputArgs &oa = e.oa;
    oa.scale = n->d_scale; oa.directional = directional; oa.xmax = pt_nn_lightmap::log_xmax();
    oa.out = device_image(staged ? packed_view(n->d_image_tmp, n->w) : v[3]);

    PtNnStages stages;
    stages.ctx = &e;
    stages.input = [](void *ctx, hipStream_t s, const ptx_nn_tile &T, int wp, int hp, uint16_t *net_in) {
        LmInputArgs a = static_cast<Ends *>(ctx)->ia;
        a.w = T.w; a.h = T.h; a.wp = wp; a.hp = hp; a.x0 = T.x; a.y0 = T.y; a.out = net_in;
        return launch(k_nn_lightmap_input, s, (size_t)wp * hp, a);
    };
    stages.output = [](void *ctx, hipStream_t s, const ptx_nn_tile &T, int wp, const float *net_out) {
        LmOutputArgs a = static_cast<Ends *>(ctx)->oa;
        a.w = T.out_w; a.h = T.out_h; a.wp = wp; a.net = net_out;
        a.ix = T.out_x - T.x; a.iy = T.out_y - T.y; a.ox = T.out_x; a.oy = T.out_y;
        return launch(k_nn_lightmap_output, s, (size_t)T.out_w * T.out_h, a);
    };
    if (const int rc = pt_nn_run_tiles(n, st, stages)) return rc;
    if (staged) {
        if (const int rc = pt_nn_image_copy_enqueue(st, n->w, n->h, n->d_image_tmp, v[3])) return rc;
        if (const int rc = pt_nn_progress_frame_unit(n, st)) return rc;
    }
    PT_HC(n->record(st));
    return PTX_OK;
}

}  // namespace

extern "C" {

void ptx_debug_nn_lightmap_constants(float *xmax, float *norm) {
    if (xmax) *xmax = pt_nn_lightmap::log_xmax();
    if (norm) *norm = pt_nn_lightmap::log_norm();
}

int ptx_nn_denoise_lightmap_device(ptx_nn *n, const ptx_nn_image *color, const ptx_nn_image *output, int directional, float input_scale,
                                   void *stream) {
    PtNnImageView v[4];
    if (const int rc = lightmap_problem("ptx_nn_denoise_lightmap_device", n, color, output, directional, input_scale, v)) return rc;
    PT_HC(hipSetDevice(n->device));
    bool mine;
    if (const int rc = pt_nn_progress_begin("ptx_nn_denoise_lightmap_device", n, pt_nn_image_staged(n, v), &mine)) return rc;
    return pt_nn_progress_end(n, mine, lightmap_enqueue(n, (hipStream_t)stream, v, directional, input_scale));
}

int ptx_nn_denoise_lightmap_host(ptx_nn *n, const ptx_nn_image *color, const ptx_nn_image *output, int directional, float input_scale) {
    PtNnImageView v[4];
    if (const int rc = lightmap_problem("ptx_nn_denoise_lightmap_host", n, color, output, directional, input_scale, v)) return rc;
    PT_HC(hipSetDevice(n->device));
    struct Call { int directional; float input_scale; } c = {directional, input_scale};
    return pt_nn_image_host_call("ptx_nn_denoise_lightmap_host", n, v, [](void *ctx, ptx_nn *h, const PtNnImageView d[4]) {
        const Call &k = *static_cast<Call *>(ctx);
        return lightmap_enqueue(h, nullptr, d, k.directional, k.input_scale);
    }, &c);
}

}  // extern "C"
