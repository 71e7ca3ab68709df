// pt_nn_aux.hip -- the network denoiser's prefilter of its guides (ptx_nn_prefilter_* of include/mi355x_pathtracer.h; OIDN's cleanAux):
// an albedo image and a normal image each denoised alone by a 3-input network of the caller's (OIDN's rt_alb / rt_nrm weight files),
// the results kept on the device for the main network.  ptx_denoise_nn_prefiltered is pt_post.hip's: it needs the tracer's buffers.
// The networks are ptx_nn's (pt_nn.hip): their per-tile loop and convolutions run unchanged between the two kernels here, both
// networks in the one scratch this handle owns (pt_nn.h).  The arithmetic is defined in the public header and restated by
// tests/unet_aux_ref.py.
//
// Kernels (the network unit's flags, see the Makefile; -ffp-contract=off stays: every step below is one IEEE fp32 operation):
//   k_nn_aux_input  : one thread per pixel of a tile's padded window: one image with a pixel stride of 3 or 4 floats (4: the tracer's
//       G-buffer records, one 16-byte load) sanitised and transformed into channels 0 .. 2 of the network's input, 16 fp16 channels per
//       pixel (two 16-byte stores), the rest and everything right of and below the window zero.
//         albedo: (v / 1) * scale; NaN -> 0; clamp to [0, 1]; the sRGB curve, or nothing (k_nn_input's colour, hdr 0, samples 1)
//         normal: v * scale; NaN -> 0; clamp to [-1, 1]; * 0.5 + 0.5
//   k_nn_aux_output : one thread per pixel of the rectangle a tile keeps: dec_conv0's three fp32 channels into three floats.
//         albedo: k_nn_output with hdr 0
//         normal: NaN -> 0; clamp to [0, FLT_MAX]; * 2 - 1; max(., -1); min(., 1); times 1 / scale (0 when scale is 0)
// The scale is a launch argument: there is no meter.  No atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "pt_nn.h"
#include "pt_nn_transfer.h"

namespace {

using namespace pt_nn_transfer;

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

constexpr int NT = 256;

struct AuxInputArgs {
    int w, h, wp, hp;                         // the window and its padded size
    int x0, y0, W;                            // the window's origin in the frame, the frame's row stride in pixels
    const float *img;                         // [H][W][stride]
    int stride, kind, mode;
    float scale;
    uint16_t *out;                            // [hp][wp][16] fp16
    float *raw;                               // NULL, or [h][w][3] fp32 before the rounding (ptx_kat_nn_transfer_aux)
};

__global__ __launch_bounds__(NT) void k_nn_aux_input(AuxInputArgs a) {
    const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= (size_t)a.wp * a.hp) return;
    const int y = (int)(idx / a.wp), x = (int)(idx - (size_t)y * a.wp);
    float v[3] = {0.f, 0.f, 0.f};
    if (x < a.w && y < a.h) {
        const size_t p = ((size_t)a.y0 + y) * a.W + a.x0 + x;
        float in[3];
        if (a.stride == 4) {
            const float4 r = reinterpret_cast<const float4 *>(a.img)[p];
            in[0] = r.x; in[1] = r.y; in[2] = r.z;
        } else {
            for (int c = 0; c < 3; c++) in[c] = a.img[3 * p + c];
        }
        for (int c = 0; c < 3; c++)
            v[c] = a.kind == PTX_NN_AUX_NORMAL ? sanitise(in[c] * a.scale, -1.f, 1.f) * 0.5f + 0.5f
                                               : transfer_forward(sanitise((in[c] / 1.0f) * a.scale, 0.f, 1.f), a.mode, 0.f);
        if (a.raw) for (int c = 0; c < 3; c++) a.raw[3 * ((size_t)y * a.w + x) + c] = v[c];
    }
    half8 lo = {0, 0, 0, 0, 0, 0, 0, 0};
    const half8 hi = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 3; c++) lo[c] = (_Float16)v[c];
    half8 *o = reinterpret_cast<half8 *>(a.out) + 2 * idx;
    o[0] = lo; o[1] = hi;
}

struct AuxOutputArgs {
    int w, h, wp;                             // the rectangle kept; the tile's padded width
    int ix, iy;                               // where the rectangle begins in the tile's output
    int ox, oy, W;                            // ... and in the frame; the frame's row stride in pixels
    const float *net;                         // [hp][wp][4] fp32
    int kind, mode;
    float scale;
    float *out;                               // [H][W][3]
};

__global__ __launch_bounds__(NT) void k_nn_aux_output(AuxOutputArgs a) {
    const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= (size_t)a.w * a.h) return;
    const int y = (int)(idx / a.w), x = (int)(idx - (size_t)y * a.w);
    const float s = a.scale, inv = s != 0.f ? 1.f / s : 0.f;
    const float4 n = reinterpret_cast<const float4 *>(a.net)[((size_t)a.iy + y) * a.wp + a.ix + x];
    const size_t p = ((size_t)a.oy + y) * a.W + a.ox + x;
    const float in[3] = {n.x, n.y, n.z};
    for (int c = 0; c < 3; c++) {
        float v = sanitise(in[c], 0.f, FLT_MAX);
        if (a.kind == PTX_NN_AUX_NORMAL) {
            v = v * 2.0f - 1.0f;
            v = fmaxf(v, -1.f);
        } else {
            v = transfer_inverse(v, a.mode, 0.f);
        }
        v = fminf(v, 1.f);
        a.out[3 * p + c] = v * inv;
    }
}

int pad16(int c) { return (c + 15) / 16 * 16; }

int launch_input(hipStream_t st, const AuxInputArgs &a) {
    const size_t n = (size_t)a.wp * a.hp;
    hipLaunchKernelGGL(k_nn_aux_input, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, a);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

int launch_output(hipStream_t st, const AuxOutputArgs &a) {
    const size_t n = (size_t)a.w * a.h;
    hipLaunchKernelGGL(k_nn_aux_output, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, a);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

int mode_of(int kind, int srgb) { return kind == PTX_NN_AUX_NORMAL || srgb ? MODE_LINEAR : MODE_SRGB; }
float scale_of(float input_scale) { return isnan(input_scale) ? 1.f : input_scale; }

// the blobs' plans and the refusals that need no device; has[k]: blob k was given
int blobs_problem(const char *fn, const void *const tza[2], const size_t bytes[2], int width, int height, int max_memory_mb, PtNnPlan plan[2], bool has[2]) {
    static const char *const what[2] = {"albedo", "normal"};
    if (!tza[0] && !tza[1]) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": no weights: the albedo blob, the normal blob or both are needed");
    for (int k = 0; k < 2; k++) {
        has[k] = tza[k] != nullptr;
        if (!has[k]) continue;
        if (const int rc = pt_nn_blob_problem(fn, tza[k], bytes[k], width, height, max_memory_mb, plan[k])) return rc;
        if (plan[k].ic != 3)
            return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": the " + what[k] + " weights take " + std::to_string(plan[k].ic) +
                                                " input channels: a prefilter network takes the image alone ('enc_conv0.weight' with 3)");
    }
    return PTX_OK;
}

struct AllocArgs { const PtNnPlan *plan; const bool *has; int max_memory_mb; };
thread_local const AllocArgs *tl_args = nullptr;      // ptx_nn_prefilter_create's, for alloc_prefilter (pt_handle_create hands over the handle alone)

int alloc_prefilter(ptx_nn_prefilter *pf) {
    const AllocArgs &A = *tl_args;
    const int limit = A.max_memory_mb < 0 ? 0 : A.max_memory_mb;
    size_t total = 0;
    for (int k = 0; k < 2; k++)
        if (A.has[k]) {
            const PtNnTiling t = pt_nn_tiling(A.plan[k], pf->w, pf->h, limit);
            total = std::max(total, pt_nn_scratch(A.plan[k], t.tile_width, t.tile_height).total);
        }
    PT_HC(hipSetDevice(pf->device));
    PT_HC(pf->d_scratch.alloc(total));
    for (int k = 0; k < 2; k++)
        if (A.has[k]) {
            if (const int rc = pt_nn_create_shared("ptx_nn_prefilter_create", pf->device, pf->w, pf->h, A.plan[k], A.max_memory_mb, pf->d_scratch, &pf->net[k])) return rc;
            if (pf->net[k]->scratch_bytes > total) return pt_fail(PTX_ERR_INVALID, "ptx_nn_prefilter_create: a network's plan exceeds the shared scratch");
            PT_HC(pf->d_clean[k].alloc(3 * (size_t)pf->w * pf->h));
            PT_HC(pf->d_clean[k].zero());
        }
    PT_HC(pf->ev.create(hipEventDisableTiming));
    return PTX_OK;
}

struct Ends { AuxInputArgs ia; AuxOutputArgs oa; };

int run_net(ptx_nn *net, hipStream_t st, Ends &e) {
    PtNnStages stages;
    stages.ctx = &e;
    stages.input = [](void *ctx, hipStream_t s, const ptx_nn_tile &T, int wp, int hp, uint16_t *net_in) {
        AuxInputArgs a = static_cast<Ends *>(ctx)->ia;
        a.w = T.w; a.h = T.h; a.wp = wp; a.hp = hp; a.x0 = T.x; a.y0 = T.y; a.out = net_in;
        return launch_input(s, a);
    };
    stages.output = [](void *ctx, hipStream_t s, const ptx_nn_tile &T, int wp, const float *net_out) {
        AuxOutputArgs a = static_cast<Ends *>(ctx)->oa;
        a.w = T.out_w; a.h = T.out_h; a.wp = wp; a.net = net_out;
        a.ix = T.out_x - T.x; a.iy = T.out_y - T.y; a.ox = T.out_x; a.oy = T.out_y;
        return launch_output(s, a);
    };
    return pt_nn_run_tiles(net, st, stages);
}

ptx_nn_prefilter_params params_or_default(const ptx_nn_prefilter_params *given) {
    ptx_nn_prefilter_params p;
    if (given) p = *given;
    else ptx_default_nn_prefilter_params(&p);
    return p;
}

// the byte ranges [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

ptx_nn_prefilter::~ptx_nn_prefilter() {
    for (ptx_nn *n : net) pt_handle_destroy(n);      // (they do not own the scratch: d_scratch goes after them, with the other members)
}

const char *pt_nn_prefilter_params_problem(const ptx_nn_prefilter_params &p) {
    if (p.srgb != 0 && p.srgb != 1) return "ptx_nn_prefilter_params.srgb must be 0 or 1";
    if (!isnan(p.input_scale) && (!(p.input_scale > 0.f) || isinf(p.input_scale))) return "ptx_nn_prefilter_params.input_scale must be NaN (1) or finite and > 0";
    return nullptr;
}

int pt_nn_prefilter_enqueue(ptx_nn_prefilter *pf, hipStream_t st, int mask, const float *alb, int alb_stride, const float *nrm, int nrm_stride,
                            const ptx_nn_prefilter_params &p) {
    const float *img[2] = {alb, nrm};
    const int stride[2] = {alb_stride, nrm_stride};
    PT_HC(pf->wait_stream(st));
    for (int k = 0; k < 2; k++) {
        if (!(mask >> k & 1)) continue;
        const int kind = k == 0 ? PTX_NN_AUX_ALBEDO : PTX_NN_AUX_NORMAL;
        Ends e;
        e.ia.W = pf->w; e.ia.img = img[k]; e.ia.stride = stride[k]; e.ia.kind = kind; e.ia.mode = mode_of(kind, p.srgb);
        e.ia.scale = scale_of(p.input_scale); e.ia.raw = nullptr;
        e.oa.W = pf->w; e.oa.kind = kind; e.oa.mode = e.ia.mode; e.oa.scale = e.ia.scale; e.oa.out = pf->d_clean[k];
        if (const int rc = run_net(pf->net[k], st, e)) return rc;
    }
    PT_HC(pf->record(st));
    pf->runs++;
    return PTX_OK;
}

extern "C" {

void ptx_default_nn_prefilter_params(ptx_nn_prefilter_params *p) {
    if (!p) return;
    p->srgb = 0;
    p->input_scale = NAN;
}

size_t ptx_sizeof_nn_prefilter_params(void) { return sizeof(ptx_nn_prefilter_params); }
size_t ptx_sizeof_nn_prefilter_info(void) { return sizeof(ptx_nn_prefilter_info); }

int ptx_debug_nn_prefilter_problem(const void *alb_tza, size_t alb_bytes, const void *nrm_tza, size_t nrm_bytes, const ptx_nn_prefilter_params *params) {
    const ptx_nn_prefilter_params p = params_or_default(params);
    if (const char *why = pt_nn_prefilter_params_problem(p)) return pt_fail(PTX_ERR_INVALID, why);
    const void *const tza[2] = {alb_tza, nrm_tza};
    const size_t bytes[2] = {alb_bytes, nrm_bytes};
    PtNnPlan plan[2];
    bool has[2];
    return blobs_problem("ptx_debug_nn_prefilter_problem", tza, bytes, 1, 1, -1, plan, has);
}

int ptx_nn_prefilter_create(int device, int width, int height, const void *alb_tza, size_t alb_bytes, const void *nrm_tza, size_t nrm_bytes,
                            int max_memory_mb, ptx_nn_prefilter **out) {
    if (out) *out = nullptr;
    const void *const tza[2] = {alb_tza, nrm_tza};
    const size_t bytes[2] = {alb_bytes, nrm_bytes};
    PtNnPlan plan[2];
    bool has[2];
    if (const int rc = blobs_problem("ptx_nn_prefilter_create", tza, bytes, width, height, max_memory_mb, plan, has)) return rc;
    const AllocArgs args = {plan, has, max_memory_mb};
    tl_args = &args;
    const long long cap = max_memory_mb < 0 ? (long long)PTX_NN_MAX_WIDTH * PTX_NN_MAX_HEIGHT : (long long)PTX_NN_MAX_FRAME * PTX_NN_MAX_FRAME;
    const int rc = pt_handle_create("ptx_nn_prefilter_create", "the network denoiser", device, width, height, cap, out, alloc_prefilter);
    tl_args = nullptr;
    return rc;
}

int ptx_nn_prefilter_create_from_files(int device, int width, int height, const char *alb_path, const char *nrm_path, int max_memory_mb,
                                       ptx_nn_prefilter **out) {
    if (out) *out = nullptr;
    const char *fn = "ptx_nn_prefilter_create_from_files";
    std::vector<uint8_t> blob[2];
    if (alb_path) if (const int rc = pt_nn_read_file(fn, alb_path, blob[0])) return rc;
    if (nrm_path) if (const int rc = pt_nn_read_file(fn, nrm_path, blob[1])) return rc;
    return ptx_nn_prefilter_create(device, width, height, alb_path ? blob[0].data() : nullptr, blob[0].size(), nrm_path ? blob[1].data() : nullptr,
                                   blob[1].size(), max_memory_mb, out);
}

void ptx_nn_prefilter_destroy(ptx_nn_prefilter *pf) { pt_handle_destroy(pf); }

int ptx_nn_prefilter_get_info(ptx_nn_prefilter *pf, ptx_nn_prefilter_info *out) {
    if (!pf || !out) return pt_fail(PTX_ERR_INVALID, "ptx_nn_prefilter_get_info: null handle or info");
    *out = ptx_nn_prefilter_info();
    out->width = pf->w; out->height = pf->h;
    out->has_albedo = pf->net[0] != nullptr; out->has_normal = pf->net[1] != nullptr;
    if (pf->net[0]) if (const int rc = ptx_nn_get_info(pf->net[0], &out->albedo)) return rc;
    if (pf->net[1]) if (const int rc = ptx_nn_get_info(pf->net[1], &out->normal)) return rc;
    out->scratch_bytes = pf->d_scratch.n;
    out->runs = pf->runs;
    return PTX_OK;
}

int ptx_nn_prefilter_invalidate(ptx_nn_prefilter *pf) {
    if (!pf) return pt_fail(PTX_ERR_INVALID, "ptx_nn_prefilter_invalidate: null handle");
    pf->cache_serial = 0; pf->cache_mask = 0;
    return PTX_OK;
}

int ptx_nn_prefilter_run_device(ptx_nn_prefilter *pf, const float *device_alb, int alb_stride, const float *device_nrm, int nrm_stride,
                                const ptx_nn_prefilter_params *params, void *stream) {
    const char *fn = "ptx_nn_prefilter_run_device";
    const ptx_nn_prefilter_params p = params_or_default(params);
    if (const char *why = pt_nn_prefilter_params_problem(p)) return pt_fail(PTX_ERR_INVALID, why);
    if (!pf) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": null handle");
    const float *img[2] = {device_alb, device_nrm};
    const int stride[2] = {alb_stride, nrm_stride};
    static const char *const what[2] = {"albedo", "normal"};
    for (int k = 0; k < 2; k++) {
        if ((img[k] != nullptr) != (pf->net[k] != nullptr))
            return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": the " + what[k] + " image " +
                                                (pf->net[k] ? "is required: the handle has a network for it" : "must be NULL: the handle has no network for it"));
        if (!img[k]) continue;
        if (stride[k] != 3 && stride[k] != 4) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": the " + what[k] + " image's stride must be 3 or 4 floats per pixel");
        if (stride[k] == 4 && ((uintptr_t)img[k] & 15)) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": an image with a stride of 4 floats must be 16-byte aligned");
        for (int j = 0; j < 2; j++)
            if (pf->net[j] && ranges_overlap(img[k], sizeof(float) * stride[k] * (size_t)pf->w * pf->h, pf->d_clean[j].p, sizeof(float) * pf->d_clean[j].n))
                return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": an image may not overlap the handle's clean images in memory");
    }
    PT_HC(hipSetDevice(pf->device));
    pf->cache_serial = 0; pf->cache_mask = 0;
    return pt_nn_prefilter_enqueue(pf, (hipStream_t)stream, (pf->net[0] ? 1 : 0) | (pf->net[1] ? 2 : 0), device_alb, alb_stride, device_nrm, nrm_stride, p);
}

int ptx_nn_prefilter_device_clean(ptx_nn_prefilter *pf, const float **alb3, const float **nrm3) {
    if (!pf) return pt_fail(PTX_ERR_INVALID, "ptx_nn_prefilter_device_clean: null handle");
    if (alb3) *alb3 = pf->net[0] ? pf->d_clean[0].p : nullptr;
    if (nrm3) *nrm3 = pf->net[1] ? pf->d_clean[1].p : nullptr;
    return PTX_OK;
}

int ptx_nn_prefilter_read(ptx_nn_prefilter *pf, float *alb3, float *nrm3) {
    if (!pf) return pt_fail(PTX_ERR_INVALID, "ptx_nn_prefilter_read: null handle");
    if (!pf->used) return pt_fail(PTX_ERR_INVALID, "ptx_nn_prefilter_read: no run on this handle yet");
    float *host[2] = {alb3, nrm3};
    for (int k = 0; k < 2; k++)
        if (host[k] && !pf->net[k]) return pt_fail(PTX_ERR_INVALID, std::string("ptx_nn_prefilter_read: the handle has no ") + (k ? "normal" : "albedo") + " network");
    PT_HC(hipSetDevice(pf->device));
    PT_HC(hipEventSynchronize(pf->ev));
    for (int k = 0; k < 2; k++)
        if (host[k]) PT_HC(pf->d_clean[k].download(host[k]));
    return PTX_OK;
}

int ptx_nn_prefilter_run_host(ptx_nn_prefilter *pf, const float *alb3, const float *nrm3, const ptx_nn_prefilter_params *params, float *out_alb3,
                              float *out_nrm3) {
    if (!pf) return pt_fail(PTX_ERR_INVALID, "ptx_nn_prefilter_run_host: null handle");
    const size_t count = 3 * (size_t)pf->w * pf->h;
    PT_HC(hipSetDevice(pf->device));
    PT_HC(pf->wait_host());
    const float *host[2] = {alb3, nrm3};
    for (int k = 0; k < 2; k++) {
        if (!host[k]) continue;
        if (!pf->d_stage[k]) PT_HC(pf->d_stage[k].alloc(count));
        PT_HC(hipMemcpy(pf->d_stage[k], host[k], sizeof(float) * count, hipMemcpyHostToDevice));
    }
    if (const int rc = ptx_nn_prefilter_run_device(pf, alb3 ? pf->d_stage[0].p : nullptr, 3, nrm3 ? pf->d_stage[1].p : nullptr, 3, params, nullptr)) return rc;
    return ptx_nn_prefilter_read(pf, pf->net[0] ? out_alb3 : nullptr, pf->net[1] ? out_nrm3 : nullptr);
}

int ptx_kat_nn_transfer_aux(int device, int w, int h, int kind, const float *in3, int srgb, float scale, int inverse, float *out3) {
    const char *fn = "ptx_kat_nn_transfer_aux";
    if (w < 1 || h < 1 || w > PTX_NN_MAX_WIDTH || h > PTX_NN_MAX_HEIGHT) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": bad frame size");
    if (!in3 || !out3) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": null array");
    if (kind != PTX_NN_AUX_ALBEDO && kind != PTX_NN_AUX_NORMAL) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": kind must be PTX_NN_AUX_ALBEDO or PTX_NN_AUX_NORMAL");
    if (srgb != 0 && srgb != 1) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": srgb must be 0 or 1");
    if (srgb && kind == PTX_NN_AUX_NORMAL) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": srgb is the albedo's: a normal image has no transfer curve");
    if (isnan(scale) || !(scale >= 0.f) || isinf(scale)) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": scale must be finite and >= 0");
    if (const int rc = pt_nn_device_problem(fn, device)) return rc;
    PT_HC(hipSetDevice(device));
    const int wp = pad16(w), hp = pad16(h);
    const size_t px = (size_t)w * h, pxp = (size_t)wp * hp;
    DevBuf<float> d_img, d_out, d_net;
    DevBuf<uint16_t> d_in;
    PT_HC(d_out.alloc(3 * px));
    if (!inverse) {
        PT_HC(d_img.upload(in3, 3 * px));
        PT_HC(d_in.alloc(pxp * 16));
        AuxInputArgs ia;
        ia.w = w; ia.h = h; ia.wp = wp; ia.hp = hp; ia.x0 = ia.y0 = 0; ia.W = w;
        ia.img = d_img; ia.stride = 3; ia.kind = kind; ia.mode = mode_of(kind, srgb); ia.scale = scale;
        ia.out = d_in; ia.raw = d_out;
        if (const int rc = launch_input(nullptr, ia)) return rc;
    } else {
        std::vector<float> net(4 * pxp, 0.f);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) memcpy(&net[4 * ((size_t)y * wp + x)], in3 + 3 * ((size_t)y * w + x), 3 * sizeof(float));
        PT_HC(d_net.upload(net));
        AuxOutputArgs oa;
        oa.w = w; oa.h = h; oa.wp = wp; oa.ix = oa.iy = oa.ox = oa.oy = 0; oa.W = w; oa.net = d_net;
        oa.kind = kind; oa.mode = mode_of(kind, srgb); oa.scale = scale; oa.out = d_out;
        if (const int rc = launch_output(nullptr, oa)) return rc;
    }
    PT_HC(hipDeviceSynchronize());
    PT_HC(d_out.download(out3));
    return PTX_OK;
}

}  // extern "C"
