// pt_display.hip -- the display transform (ptx_display_* of include/mi355x_pathtracer.h): a scene-referred fp32 frame -> automatic
// exposure from block luminances, a tone curve, the sRGB transfer, 8-bit codes.  ptx_display_tracer is pt_engine.hip's: it needs the
// tracer's buffers and stream.  State layout in pt_display.h; the rule itself is defined in the public header and restated in float64 by
// tests/display_ref.py.
//
// Kernels (fp32, exact arithmetic: the Makefile's common flags, -ffp-contract=off included, so numpy in float32 reproduces the quantiser
// bit for bit from z):
//   k_display_blocks : one workgroup of 256 per block of the meter's grid (at most 23 x 23 pixels; its bounds from a table of the host's).  Thread t adds the luminances of the
//       block's pixels t, t + 256, t + 512 (block-linear order) in fp32, a wave adds its lanes by shuffles of fixed shape, thread 0 adds
//       the four waves' sums from LDS in wave order: the same bits on every run.  12 B read per pixel, one plain 4-byte vector store per block.
//   k_display_meter  : one workgroup of 1024.  Thread t adds log2f(L) over blocks t, t + 1024, ... in that order, in DOUBLE (at 3840 x 2160
//       there are 32 400 terms of magnitude up to 27: an fp32 running sum would be off by percent), then a tree of fixed shape in LDS.
//       Thread 0 forms the metered exposure, adapts the applied one (in double) and stores the state record.  No float atomics anywhere.
//   k_display_map<VEC, KEEP> : VEC: one thread maps four consecutive pixels -- three 16-byte loads, one 16-byte store of four uchar4, and
//       with KEEP three 16-byte stores of z; the last W*H mod 4 pixels go through scalar code in the threads behind.  !VEC: one thread per
//       pixel, for a caller's pointer that is not 16-byte aligned.  The applied exposure is read from the state record.  The uchar4
//       written is the quantisation of exactly the fp32 z that KEEP stores.  Plain vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include <algorithm>
#include <string>
#include <vector>

#include "pt_display.h"

namespace {

constexpr int NT = 256, WAVE = 64, NWAVES = NT / WAVE;
constexpr int NTM = 1024;                 // k_display_meter's one workgroup
// The upper clamp of a sanitised channel.  This is OIDN's HDR_Y_MAX (the largest half float), not its pos_max (the largest float): a
// block sums up to 529 luminances in fp32, and 529 * 65504 cannot overflow where 529 * FLT_MAX would.
constexpr float C_MAX = 65504.f;
constexpr float L_MIN = 1e-8f;            // blocks at or below this luminance do not vote (OIDN: core/color.ispc, getAvgLuminance)

// step 1: rgb / samples by an IEEE division as k_pbo does it, NaN -> 0, clamped to [0, C_MAX]
__device__ __forceinline__ float sanitise(float v, float samples) {
    const float c = v / samples;
    return c != c ? 0.f : fminf(fmaxf(c, 0.f), C_MAX);
}

// grid = (WK, HK); begin = the HK + 1 row and WK + 1 column boundaries of the block grid, tabulated by the host (pt_display_begins)
__global__ __launch_bounds__(NT) void k_display_blocks(int w, int hk, float samples, const int *__restrict__ begin,
                                                       const float *__restrict__ rgb, float *__restrict__ blocks) {
    __shared__ float s_wave[NWAVES];
    const int i = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
    const int b = i * gridDim.x + j;
    const int r0 = begin[i], r1 = begin[i + 1], c0 = begin[hk + 1 + j], c1 = begin[hk + 2 + j];
    const int bw = c1 - c0, n = bw * (r1 - r0);
    float sum = 0.f;
    for (int k = tid; k < n; k += NT) {
        const int dy = k / bw, dx = k - dy * bw;
        const float *pix = rgb + 3 * ((size_t)(r0 + dy) * w + (c0 + dx));
        // the project's one luminance (pt_denoise.h: Rec. 709), not OIDN's slightly different weights: every variance, error and
        // exposure of this library is one of the same quantity
        sum = sum + pt_luminance(sanitise(pix[0], samples), sanitise(pix[1], samples), sanitise(pix[2], samples));
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) sum = sum + __shfl_down(sum, off, WAVE);
    if ((tid & (WAVE - 1)) == 0) s_wave[tid / WAVE] = sum;
    __syncthreads();
    if (tid == 0) blocks[b] = (((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3]) / (float)n;
}

__device__ __forceinline__ void vote(float L, double &sum, int &cnt) {
    if (L > L_MIN) { sum = sum + (double)log2f(L); cnt++; }
}

__global__ __launch_bounds__(NTM) void k_display_meter(int nblocks, const float *__restrict__ blocks, float key, float adapt, int fresh,
                                                       PtDisplayState *state) {
    __shared__ double s_sum[NTM];
    __shared__ int s_cnt[NTM];
    const int tid = threadIdx.x;
    double sum = 0.0;
    int cnt = 0;
    // thread t takes blocks t, t + NTM, t + 2 NTM, ... in that order; four loads are in flight before the first is used (the loop is
    // a chain of memory latencies otherwise: 32 400 blocks at 3840 x 2160)
    for (int k = tid; k < nblocks; k += 4 * NTM) {
        const float L0 = blocks[k];
        const float L1 = k + NTM < nblocks ? blocks[k + NTM] : 0.f;
        const float L2 = k + 2 * NTM < nblocks ? blocks[k + 2 * NTM] : 0.f;
        const float L3 = k + 3 * NTM < nblocks ? blocks[k + 3 * NTM] : 0.f;
        vote(L0, sum, cnt); vote(L1, sum, cnt); vote(L2, sum, cnt); vote(L3, sum, cnt);
    }
    s_sum[tid] = sum; s_cnt[tid] = cnt;
    __syncthreads();
    for (int s = NTM / 2; s > 0; s >>= 1) {
        if (tid < s) { s_sum[tid] = s_sum[tid] + s_sum[tid + s]; s_cnt[tid] += s_cnt[tid + s]; }
        __syncthreads();
    }
    if (tid != 0) return;
    const int used = s_cnt[0];
    const double m = used ? s_sum[0] / (double)used : 0.0;
    const double metered = used ? (double)key / exp2(m) : 1.0;       // no block to vote (a frame below 8 pixels, a black frame): 1
    const double lm = log2(metered);
    PtDisplayState st = *state;
    const bool jump = fresh || adapt >= 1.f;                         // the first metered frame, or no inertia: applied = metered
    const double la = jump ? lm : st.log2_applied + (double)adapt * (lm - st.log2_applied);
    st.log2_applied = la;
    st.metered = (float)metered;
    st.applied = jump ? (float)metered : (float)exp2(la);
    st.log2_mean = (float)m;
    st.blocks_used = used;
    st.blocks_total = nblocks;
    st.reserved = 0;
    st.frames = fresh ? 1 : st.frames + 1;
    *state = st;
}

struct MapArgs {
    float samples, exposure, white;
    int tone, transfer, quantize, dither;
    int w;
};

// (2 B + 1) / 128 of the 8 x 8 Bayer matrix B: exact in fp32.  B interleaves the bits of x ^ y and y, most significant pair from bit 0.
__device__ __forceinline__ float bayer_threshold(int x, int y) {
    const int a = (x ^ y) & 7, c = y & 7;
    const int B = ((a & 1) << 5) | ((c & 1) << 4) | ((a & 2) << 2) | ((c & 2) << 1) | ((a & 4) >> 1) | ((c & 4) >> 2);
    return (float)(2 * B + 1) / 128.f;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ float aces(float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); }

// Beyond what fp32 holds.  x = c E reaches 65504 * FLT_MAX, and a curve written as the rule writes it then divides inf by inf: both
// products of aces() overflow from x of about 1.2e19, Reinhard is inf * inf / inf at x = inf, and clamp01 takes the NaN to 0 -- a
// saturated channel came out black.  The two curves are kept the real numbers' curves in different ways, because ACES is a function
// of one channel and Reinhard of the ratios between three:
//   ACES     : x is held to X_CAP = 2^60 inside the curve.  The clamped curve is exactly 1 from x = 7.25 on, the largest product at
//       the cap is 2^121, and no bit below the cap changes.  A select, not fminf: a NaN (0 * inf when applied * exposure overflowed)
//       stays one and clamps to 0 as before.
//   Reinhard : no channel is capped -- that would change x / L.  From L = 2^60 on, 1 + L is L to 2^-60, so
//       y = x / L + x / white^2, and both terms are formed from c, where E cancels or can be multiplied in last:
//       c / l(c) + ((c / white) * E) / white.  Below that L, x and L are finite and the rule's own expression stands, but for
//       1 + L / white^2 = inf (a white below about 1e-19 beside any light), where x * inf would be 1 even for a channel of 1e-40
//       whose y = x / white^2 is below 1: there the same quotient is taken with the large factor last.
// tests/test_display_grid_cpu.py restates all of it in numpy float32 on non-grey pixels.
constexpr float X_CAP = 0x1p60f;
constexpr float F_MAX = 3.402823466e38f;

// (the power through the hardware's log2 / exp2, about an ulp each: y is a normal number in (0.003, 1] here, and the result is held to
// 1e-4 of the float64 restatement, not to libm's last bit; powf is a long routine, three times per pixel)
__device__ __forceinline__ float transfer_srgb(float y) {
    return y <= 0.0031308f ? 12.92f * y : 1.055f * __builtin_amdgcn_exp2f(__log2f(y) * (1.f / 2.4f)) - 0.055f;
}

__device__ __forceinline__ unsigned quantise(float z, const MapArgs &a, float threshold) {
    if (!a.quantize) return (unsigned)(int)((double)z * 255.0);      // the reference's truncation (k_pbo)
    return (unsigned)(int)(z * 255.f + threshold);
}

// steps 1, 4 - 7 on one pixel: z into zr, zg, zb, the uchar4 (alpha 0) as the return value's four bytes
__device__ __forceinline__ unsigned map_pixel(float r, float g, float b, float E, const MapArgs &a, int pixel, float &zr, float &zg, float &zb) {
    const float cr = sanitise(r, a.samples), cg = sanitise(g, a.samples), cb = sanitise(b, a.samples);
    const float xr = cr * E, xg = cg * E, xb = cb * E;
    float yr = xr, yg = xg, yb = xb;
    if (a.tone == PTX_TONE_REINHARD) {
        const float L = pt_luminance(xr, xg, xb);
        const float w2 = a.white * a.white;
        const float num = 1.f + L / w2, den = 1.f + L;
        if (!(L < X_CAP)) {
            const float Lc = pt_luminance(cr, cg, cb);
            yr = cr / Lc + cr / a.white * E / a.white; yg = cg / Lc + cg / a.white * E / a.white; yb = cb / Lc + cb / a.white * E / a.white;
        } else if (num > F_MAX) {
            // (x / (1 + L), left out, is below 2^-128 of what stays; white^2 = 0: x / 0 = inf and 0 / 0 = NaN clamp to 1 and 0, as they should)
            const float s = L / den;
            yr = xr / w2 * s; yg = xg / w2 * s; yb = xb / w2 * s;
        } else {
            yr = xr * num / den; yg = xg * num / den; yb = xb * num / den;
        }
    } else if (a.tone == PTX_TONE_ACES) {
        yr = aces(xr > X_CAP ? X_CAP : xr); yg = aces(xg > X_CAP ? X_CAP : xg); yb = aces(xb > X_CAP ? X_CAP : xb);
    }
    yr = clamp01(yr); yg = clamp01(yg); yb = clamp01(yb);
    if (a.transfer == PTX_TRANSFER_SRGB) { yr = transfer_srgb(yr); yg = transfer_srgb(yg); yb = transfer_srgb(yb); }
    zr = yr; zg = yg; zb = yb;
    float threshold = 0.5f;
    if (a.dither) {
        const int y = pixel / a.w;
        threshold = bayer_threshold(pixel - y * a.w, y);
    }
    return quantise(zr, a, threshold) | (quantise(zg, a, threshold) << 8) | (quantise(zb, a, threshold) << 16);
}

template <bool VEC, bool KEEP>
__global__ __launch_bounds__(NT) void k_display_map(int n, MapArgs a, const PtDisplayState *__restrict__ state, const float *__restrict__ rgb,
                                                    unsigned *__restrict__ out, float *__restrict__ zout) {
    const int t = blockIdx.x * NT + threadIdx.x;
    const float E = state ? state->applied * a.exposure : a.exposure;
    const int quads = VEC ? n / 4 : 0;
    if (VEC && t < quads) {
        const float4 *in = reinterpret_cast<const float4 *>(rgb) + 3 * (size_t)t;
        const float4 A = in[0], B = in[1], Cq = in[2];
        float4 za, zb, zc;
        uint4 o;
        o.x = map_pixel(A.x, A.y, A.z, E, a, 4 * t, za.x, za.y, za.z);
        o.y = map_pixel(A.w, B.x, B.y, E, a, 4 * t + 1, za.w, zb.x, zb.y);
        o.z = map_pixel(B.z, B.w, Cq.x, E, a, 4 * t + 2, zb.z, zb.w, zc.x);
        o.w = map_pixel(Cq.y, Cq.z, Cq.w, E, a, 4 * t + 3, zc.y, zc.z, zc.w);
        reinterpret_cast<uint4 *>(out)[t] = o;
        if (KEEP) {
            float4 *zo = reinterpret_cast<float4 *>(zout) + 3 * (size_t)t;
            zo[0] = za; zo[1] = zb; zo[2] = zc;
        }
        return;
    }
    const int p = 4 * quads + (t - quads);           // the tail of the vector form; every pixel of the scalar one
    if (p >= n) return;
    float zr, zg, zb;
    out[p] = map_pixel(rgb[3 * (size_t)p], rgb[3 * (size_t)p + 1], rgb[3 * (size_t)p + 2], E, a, p, zr, zg, zb);
    if (KEEP) { zout[3 * (size_t)p] = zr; zout[3 * (size_t)p + 1] = zg; zout[3 * (size_t)p + 2] = zb; }
}

int alloc_display(ptx_display *d) {
    const size_t n = (size_t)d->w * d->h;
    pt_display_grid(d->w, d->h, &d->hk, &d->wk);
    if (d->hk == 0 || d->wk == 0) d->hk = d->wk = 0;
    PT_HC(hipSetDevice(d->device));
    PT_HC(d->d_blocks.alloc(std::max<size_t>((size_t)d->hk * d->wk, 1)));
    std::vector<int32_t> begin((size_t)d->hk + d->wk + 2, 0);
    pt_display_begins(d->w, d->h, d->hk, d->wk, begin.data(), begin.data() + d->hk + 1);
    PT_HC(d->d_begin.upload(begin));
    PT_HC(d->d_state.alloc(1));
    PT_HC(d->d_state.zero());
    PT_HC(d->d_codes.alloc(n));
    PT_HC(d->ev.create(hipEventDisableTiming));
    return PTX_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <bool VEC>
void launch_map(hipStream_t st, int n, const MapArgs &a, const PtDisplayState *state, const float *rgb, unsigned *out, float *zout) {
    const int threads = VEC ? n / 4 + n % 4 : n;
    const dim3 grid((unsigned)((threads + NT - 1) / NT));
    if (zout) hipLaunchKernelGGL((k_display_map<VEC, true>), grid, dim3(NT), 0, st, n, a, state, rgb, out, zout);
    else hipLaunchKernelGGL((k_display_map<VEC, false>), grid, dim3(NT), 0, st, n, a, state, rgb, out, zout);
}

}  // namespace

// integer arithmetic as OIDN's getAutoexposure (core/color.cpp:62-65)
void pt_display_begins(int w, int h, int hk, int wk, int32_t *row_begin, int32_t *col_begin) {
    if (row_begin) for (int i = 0; i <= hk && hk > 0; i++) row_begin[i] = (int32_t)((long long)i * h / hk);
    if (col_begin) for (int j = 0; j <= wk && wk > 0; j++) col_begin[j] = (int32_t)((long long)j * w / wk);
}

const char *pt_display_params_problem(const ptx_display_params &p, float samples) {
    if (p.meter != PTX_METER_MANUAL && p.meter != PTX_METER_BLOCKS) return "ptx_display_params.meter must be PTX_METER_MANUAL or PTX_METER_BLOCKS";
    if (p.tone != PTX_TONE_CLAMP && p.tone != PTX_TONE_REINHARD && p.tone != PTX_TONE_ACES)
        return "ptx_display_params.tone must be PTX_TONE_CLAMP, PTX_TONE_REINHARD or PTX_TONE_ACES";
    if (p.transfer != PTX_TRANSFER_LINEAR && p.transfer != PTX_TRANSFER_SRGB)
        return "ptx_display_params.transfer must be PTX_TRANSFER_LINEAR or PTX_TRANSFER_SRGB";
    if (p.quantize != 0 && p.quantize != 1) return "ptx_display_params.quantize must be 0 (truncate) or 1 (round)";
    if (p.dither != 0 && p.dither != 1) return "ptx_display_params.dither must be 0 or 1";
    if (p.keep_float != 0 && p.keep_float != 1) return "ptx_display_params.keep_float must be 0 or 1";
    if (!(p.exposure > 0.f) || isinf(p.exposure)) return "ptx_display_params.exposure must be finite and positive";
    if (!(p.key > 0.f) || isinf(p.key)) return "ptx_display_params.key must be finite and positive";
    if (!(p.white > 0.f) || isinf(p.white)) return "ptx_display_params.white must be finite and positive";
    if (!(p.adapt > 0.f) || p.adapt > 1.f) return "ptx_display_params.adapt must be in (0, 1]";
    if (!(samples > 0.f) || isinf(samples)) return "the display transform's divisor (samples) must be finite and positive";
    return nullptr;
}

int pt_display_enqueue(ptx_display *d, hipStream_t st, const float *rgb, float samples, const ptx_display_params &p, void *device_uchar4) {
    const int n = d->w * d->h, nblocks = d->hk * d->wk;
    if (p.keep_float && !d->d_float) PT_HC(d->d_float.alloc(3 * (size_t)n));      // 12 B per pixel, only for who asks
    PT_HC(d->wait_stream(st));                                       // the handle's last work, maybe on another stream
    const bool blocks = p.meter == PTX_METER_BLOCKS;
    if (blocks) {
        if (nblocks > 0) {
            hipLaunchKernelGGL(k_display_blocks, dim3((unsigned)d->wk, (unsigned)d->hk), dim3(NT), 0, st, d->w, d->hk, samples,
                               (const int *)d->d_begin, rgb, d->d_blocks);
            PT_HC(hipGetLastError());
        }
        hipLaunchKernelGGL(k_display_meter, dim3(1), dim3(NTM), 0, st, nblocks, (const float *)d->d_blocks, p.key, p.adapt, d->fresh ? 1 : 0,
                           d->d_state);
        PT_HC(hipGetLastError());
        d->fresh = false;
        d->metered = true;
    }
    MapArgs a;
    a.samples = samples; a.exposure = p.exposure; a.white = p.white;
    a.tone = p.tone; a.transfer = p.transfer; a.quantize = p.quantize; a.dither = p.quantize && p.dither ? 1 : 0;
    a.w = d->w;
    unsigned *out = reinterpret_cast<unsigned *>(device_uchar4 ? device_uchar4 : (void *)d->d_codes);
    float *zout = p.keep_float ? d->d_float.p : nullptr;
    const PtDisplayState *state = blocks ? d->d_state.p : nullptr;
    if (aligned16(rgb) && aligned16(out)) launch_map<true>(st, n, a, state, rgb, out, zout);
    else launch_map<false>(st, n, a, state, rgb, out, zout);         // a caller's pointer off the 16-byte grid: the per-pixel form
    PT_HC(hipGetLastError());
    PT_HC(d->record(st));
    d->codes_own = device_uchar4 == nullptr;
    d->float_valid = p.keep_float != 0;
    return PTX_OK;
}

// The meter alone, for the network denoiser's automatic scale (pt_nn.hip): steps 1 and 2 at `key`, adapt 1, so state->metered is the
// frame's.  The handle is the caller's own and never shown: it orders it, and neither the event nor the flags of a display call move.
int pt_display_meter_enqueue(ptx_display *d, hipStream_t st, const float *rgb, float samples, float key) {
    const int nblocks = d->hk * d->wk;
    if (nblocks > 0) {
        hipLaunchKernelGGL(k_display_blocks, dim3((unsigned)d->wk, (unsigned)d->hk), dim3(NT), 0, st, d->w, d->hk, samples,
                           (const int *)d->d_begin, rgb, d->d_blocks);
        PT_HC(hipGetLastError());
    }
    hipLaunchKernelGGL(k_display_meter, dim3(1), dim3(NTM), 0, st, nblocks, (const float *)d->d_blocks, key, 1.f, 1, d->d_state);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

extern "C" {

void ptx_default_display_params(ptx_display_params *p) {
    if (!p) return;
    p->meter = PTX_METER_BLOCKS;
    p->exposure = 1.f;
    p->key = 0.18f;            // OIDN's key (core/color.cpp, getAutoexposure)
    p->adapt = 1.f;
    p->tone = PTX_TONE_ACES;
    p->white = 4.f;
    p->transfer = PTX_TRANSFER_SRGB;
    p->quantize = 1;
    p->dither = 0;
    p->keep_float = 0;
}

size_t ptx_sizeof_display_params(void) { return sizeof(ptx_display_params); }
size_t ptx_sizeof_display_status(void) { return sizeof(ptx_display_status); }

int ptx_debug_display_blocks(int w, int h, int *hk, int *wk, int32_t *row_begin, int32_t *col_begin) {
    if (w < 1 || h < 1 || !hk || !wk) return pt_fail(PTX_ERR_INVALID, "ptx_debug_display_blocks: bad frame size or NULL hk / wk");
    pt_display_grid(w, h, hk, wk);
    if (*hk == 0 || *wk == 0) { *hk = *wk = 0; return PTX_OK; }     // below 8 pixels either way: no block
    pt_display_begins(w, h, *hk, *wk, row_begin, col_begin);
    return PTX_OK;
}

int ptx_display_create(int device, int width, int height, ptx_display **out) {
    return pt_handle_create("ptx_display_create", "the display handle", device, width, height, INT_MAX / 4, out, alloc_display);
}

void ptx_display_destroy(ptx_display *d) { pt_handle_destroy(d); }

int ptx_display_reset(ptx_display *d) {
    if (!d) return pt_fail(PTX_ERR_INVALID, "ptx_display_reset: null display handle");
    d->fresh = true;           // (the state record is only written behind this: the next metered frame overwrites it, and waits for the last)
    d->metered = false;
    return PTX_OK;
}

int ptx_display_device(ptx_display *d, const float *device_rgb, float samples, const ptx_display_params *params, void *device_uchar4, void *stream) {
    ptx_display_params p;
    if (params) p = *params;
    else ptx_default_display_params(&p);
    if (const char *why = pt_display_params_problem(p, samples)) return pt_fail(PTX_ERR_INVALID, why);
    if (!d || !device_rgb) return pt_fail(PTX_ERR_INVALID, "ptx_display_device: null display handle or frame");
    PT_HC(hipSetDevice(d->device));
    return pt_display_enqueue(d, (hipStream_t)stream, device_rgb, samples, p, device_uchar4);
}

int ptx_display_host(ptx_display *d, const float *host_rgb, float samples, const ptx_display_params *params, uint8_t *host_rgba) {
    ptx_display_params p;
    if (params) p = *params;
    else ptx_default_display_params(&p);
    if (const char *why = pt_display_params_problem(p, samples)) return pt_fail(PTX_ERR_INVALID, why);
    if (!d || !host_rgb) return pt_fail(PTX_ERR_INVALID, "ptx_display_host: null display handle or frame");
    const size_t n = (size_t)d->w * d->h;
    PT_HC(hipSetDevice(d->device));
    PT_HC(d->wait_host());
    if (!d->d_stage) PT_HC(d->d_stage.alloc(3 * n));
    PT_HC(hipMemcpy(d->d_stage, host_rgb, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
    if (const int rc = pt_display_enqueue(d, nullptr, d->d_stage, samples, p, nullptr)) return rc;
    PT_HC(hipEventSynchronize(d->ev));
    if (host_rgba) PT_HC(hipMemcpy(host_rgba, d->d_codes, 4 * n, hipMemcpyDeviceToHost));
    return PTX_OK;
}

int ptx_display_read(ptx_display *d, float *rgb3, uint8_t *rgba4) {
    if (!d) return pt_fail(PTX_ERR_INVALID, "ptx_display_read: null display handle");
    if (!d->used) return pt_fail(PTX_ERR_INVALID, "ptx_display_read: no display call on this handle yet");
    if (rgb3 && !d->float_valid) return pt_fail(PTX_ERR_INVALID, "ptx_display_read: the float frame exists only after a call with keep_float = 1");
    if (rgba4 && !d->codes_own)
        return pt_fail(PTX_ERR_INVALID, "ptx_display_read: the last call wrote its codes into the caller's buffer, not the handle's");
    const size_t n = (size_t)d->w * d->h;
    PT_HC(hipSetDevice(d->device));
    PT_HC(hipEventSynchronize(d->ev));
    if (rgb3) PT_HC(hipMemcpy(rgb3, d->d_float, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
    if (rgba4) PT_HC(hipMemcpy(rgba4, d->d_codes, 4 * n, hipMemcpyDeviceToHost));
    return PTX_OK;
}

int ptx_display_read_blocks(ptx_display *d, float *block_lum) {
    if (!d || !block_lum) return pt_fail(PTX_ERR_INVALID, "ptx_display_read_blocks: null display handle or array");
    if (!d->metered) return pt_fail(PTX_ERR_INVALID, "ptx_display_read_blocks: no metered frame on this handle since create / reset");
    const size_t nblocks = (size_t)d->hk * d->wk;
    if (!nblocks) return PTX_OK;
    PT_HC(hipSetDevice(d->device));
    PT_HC(hipEventSynchronize(d->ev));
    PT_HC(hipMemcpy(block_lum, d->d_blocks, sizeof(float) * nblocks, hipMemcpyDeviceToHost));
    return PTX_OK;
}

int ptx_display_get_status(ptx_display *d, ptx_display_status *out) {
    if (!d || !out) return pt_fail(PTX_ERR_INVALID, "ptx_display_get_status: null display handle or status");
    *out = ptx_display_status();
    out->metered = out->applied = 1.f;                   // before the first metered frame: exposure 1, nothing seen
    out->blocks_total = d->hk * d->wk;
    if (!d->metered) return PTX_OK;
    PtDisplayState s;
    PT_HC(hipSetDevice(d->device));
    PT_HC(hipEventSynchronize(d->ev));
    PT_HC(hipMemcpy(&s, d->d_state, sizeof s, hipMemcpyDeviceToHost));
    out->metered = s.metered; out->applied = s.applied; out->log2_mean = s.log2_mean;
    out->blocks_used = s.blocks_used; out->blocks_total = s.blocks_total;
    out->frames = s.frames;
    return PTX_OK;
}

}  // extern "C"
