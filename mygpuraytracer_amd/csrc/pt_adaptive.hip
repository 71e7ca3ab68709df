// pt_adaptive.hip -- adaptive sampling by tiles (ptx_adaptive_* of include/mi355x_pathtracer.h): per-tile sample counts, the tile error
// from the batch-means moments (pt_moments.hip), the decision which tiles go on, and the frame normalised by per-tile counts.  The
// tracer is not touched here: ptx_adaptive_add / _select / _resolve and ptx_denoise_adaptive are pt_engine.hip's (they need its
// accumulation buffer, its stream, its tile mask and its G-buffer) and enqueue the kernels below.  State layout in pt_adaptive.h.
//
// Kernels:
//   k_tile_mask        : one thread per tile, the tracer's table of visible geoms ANDed with the flags (pt_engine.hip enqueues it: that
//       unit holds the tracer's own kernels and nothing else).
//   k_adaptive_advance : one thread per tile, the counts of the tiles that were rendered and the (k, W') table of the tiled moments add.
//   k_adaptive_select  : one workgroup per tile.  Per pixel k_moments_summary's rel; the workgroup's sum of rel^2 in double through a
//       tree of fixed shape in LDS; e_T = sqrt(sum / n_T), the decision.  No atomics: the same bits on every run.
//   k_adaptive_status  : one workgroup; thread t takes a contiguous run of tiles in index order, then the same tree.  Integers only but
//       for the largest e_T, a maximum.
//   k_adaptive_resolve : one thread per pixel, acc / samples of its tile.
//   k_adaptive_prep    : the variance-guided filter's prep on a frame of unequal counts (ptx_denoise_adaptive): k_moments_prep with the
//       divisor and W of the pixel's tile, and the resolve's store.  One thread per pixel on the filter's grid of 64 x 4 pixels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include <string.h>
#include <string>
#include <vector>

#include "pt_adaptive.h"

namespace {

constexpr int NT = 256;
constexpr float LR = 0.2126f, LG = 0.7152f, LB = 0.0722f;   // pt_luminance's weights

// (src may be keep itself: every thread reads its element before it writes it)
__global__ __launch_bounds__(NT) void k_tile_mask(int ntiles, const uint8_t *src, uint8_t *keep, const uint32_t *__restrict__ base,
                                                  uint32_t *__restrict__ eff) {
    const int tile = blockIdx.x * NT + threadIdx.x;
    if (tile >= ntiles) return;
    const uint8_t a = src[tile] != 0 ? 1 : 0;
    keep[tile] = a;
    eff[tile] = a ? base[tile] : 0u;
}

__global__ __launch_bounds__(NT) void k_adaptive_advance(int ntiles, int k, const uint8_t *__restrict__ active, int32_t *__restrict__ samples,
                                                         int32_t *__restrict__ batches, float2 *__restrict__ kt) {
    const int tile = blockIdx.x * NT + threadIdx.x;
    if (tile >= ntiles) return;
    int32_t s = samples[tile];
    float fk = 0.f;
    if (active[tile]) {
        s += k; fk = (float)k;
        samples[tile] = s;
        batches[tile] = batches[tile] + 1;
    }
    kt[tile] = make_float2(fk, (float)s);
}

__global__ __launch_bounds__(NT) void k_adaptive_select(int w, int npix, int pairs, int tile_px, float floor_l, float target, int min_batches,
                                                        int max_samples, const float4 *__restrict__ snap, const float4 *__restrict__ mean,
                                                        const float4 *__restrict__ ma, const float2 *__restrict__ mb2,
                                                        const int32_t *__restrict__ samples, const int32_t *__restrict__ batches,
                                                        float *__restrict__ err, int32_t *__restrict__ nest, uint8_t *__restrict__ active) {
    __shared__ double s_sum[NT];
    __shared__ int s_cnt[NT];
    const int tile = blockIdx.x, tid = threadIdx.x;
    const long long p0 = (long long)tile * tile_px;
    const int n_t = (int)min((long long)tile_px, (long long)npix - p0);
    double sum = 0.0;
    int cnt = 0;
    for (int i = tid; i < n_t; i += NT) {
        const size_t p = (size_t)(p0 + i);
        const float4 mu = mean[p];
        if (mu.w >= 2.f) {                               // (k_moments_summary's rel, operation for operation)
            const int y = (int)(p / (size_t)w), x = (int)(p - (size_t)y * w);
            const float2 b = mb2[(size_t)y * pairs * 2 + x];
            const float q = fmaxf(quad_form(LR, LG, LB, ma[p], b.x, b.y, mu.w), 0.f);
            const float rel = sqrtf(q / snap[p].w) / fmaxf(pt_luminance(mu.x, mu.y, mu.z), floor_l);
            sum += (double)rel * rel;
            cnt++;
        }
    }
    s_sum[tid] = sum; s_cnt[tid] = cnt;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) { s_sum[tid] += s_sum[tid + s]; s_cnt[tid] += s_cnt[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        const float e = s_cnt[0] ? (float)sqrt(s_sum[0] / (double)n_t) : 0.f;
        err[tile] = e;
        nest[tile] = s_cnt[0];
        active[tile] = (samples[tile] < max_samples && (batches[tile] < min_batches || e > target)) ? 1 : 0;
    }
}

struct Tally {
    long long samples_total, pixels_active;
    int tiles_active, smin, smax;
    float worst;
};

__device__ __forceinline__ void tally_add(Tally &a, const Tally &b) {
    a.samples_total += b.samples_total; a.pixels_active += b.pixels_active; a.tiles_active += b.tiles_active;
    a.smin = min(a.smin, b.smin); a.smax = max(a.smax, b.smax); a.worst = fmaxf(a.worst, b.worst);
}

__global__ __launch_bounds__(NT) void k_adaptive_status(int ntiles, int npix, int tile_px, int rounds, const int32_t *__restrict__ samples,
                                                        const float *__restrict__ err, const int32_t *__restrict__ nest,
                                                        const uint8_t *__restrict__ active, ptx_adaptive_status *__restrict__ out) {
    __shared__ Tally s_t[NT];
    const int tid = threadIdx.x;
    const int run = (ntiles + NT - 1) / NT;
    Tally v = {0ll, 0ll, 0, INT_MAX, 0, 0.f};
    for (int i = tid * run; i < min((tid + 1) * run, ntiles); i++) {
        const int n_t = (int)min((long long)tile_px, (long long)npix - (long long)i * tile_px);
        const int s = samples[i];
        Tally o = {(long long)s * n_t, active[i] ? (long long)n_t : 0ll, active[i] ? 1 : 0, s, s, nest[i] > 0 ? err[i] : 0.f};
        tally_add(v, o);
    }
    s_t[tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) tally_add(s_t[tid], s_t[tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        const Tally t = s_t[0];
        ptx_adaptive_status o;
        o.samples_total = t.samples_total; o.pixels_active = t.pixels_active; o.tiles = ntiles; o.tiles_active = t.tiles_active;
        o.samples_min = t.smin; o.samples_max = t.smax; o.worst_error = t.worst; o.rounds = rounds;
        *out = o;
    }
}

__global__ __launch_bounds__(NT) void k_adaptive_resolve(int npix, int tile_px, const float *__restrict__ acc, const int32_t *__restrict__ samples,
                                                         float *__restrict__ frame) {
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= npix) return;
    const int s = samples[p / tile_px];
    const float n = (float)s;
    const size_t i = 3 * (size_t)p;
    frame[i] = s > 0 ? acc[i] / n : 0.f; frame[i + 1] = s > 0 ? acc[i + 1] / n : 0.f; frame[i + 2] = s > 0 ? acc[i + 2] / n : 0.f;
}

// k_moments_prep (pt_moments.hip) with the divisor of the pixel's tile, operation for operation: c = float4(acc / s (demodulated on hit
// pixels), v), v = max(g^T C g, 0) / W on hit pixels with B >= min_batches, -1 on the other hit pixels, 0 on miss pixels; and the
// un-demodulated acc / s into frame (k_adaptive_resolve's store).  s = samples[tile] > 0 for every tile (ptx_denoise_adaptive checks
// the host's mirror), and W = float(s): the state's snap.w holds the same number, which is therefore not read.  One thread per pixel
// of the 64 x 4 grid, so a wave is one row segment and samples[] changes at most once inside it.  No LDS, no atomics.
__global__ __launch_bounds__(PT_BX * PT_BY) void k_adaptive_prep(int w, int h, int pairs, int tile_px, const float *__restrict__ rgb,
                                                                 const int32_t *__restrict__ samples, const float4 *__restrict__ nh,
                                                                 const float4 *__restrict__ alb, int demod, const float4 *__restrict__ mean,
                                                                 const float4 *__restrict__ ma, const float2 *__restrict__ mb2,
                                                                 float min_batches, float4 *__restrict__ c, float *__restrict__ frame) {
    const int x = blockIdx.x * PT_BX + threadIdx.x, y = blockIdx.y * PT_BY + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float spp = (float)samples[p / (size_t)tile_px];
    float r = rgb[3 * p] / spp, g = rgb[3 * p + 1] / spp, b = rgb[3 * p + 2] / spp;
    frame[3 * p] = r; frame[3 * p + 1] = g; frame[3 * p + 2] = b;
    float v = 0.f;
    if (nh[p].w != 0.f) {
        float g0 = LR, g1 = LG, g2 = LB;
        if (demod) {
            const float4 a = alb[p];
            const float f0 = fmaxf(a.x, 1e-3f), f1 = fmaxf(a.y, 1e-3f), f2 = fmaxf(a.z, 1e-3f);
            r = r / f0; g = g / f1; b = b / f2;
            g0 = g0 / f0; g1 = g1 / f1; g2 = g2 / f2;
        }
        const float B = mean[p].w;
        v = -1.f;
        if (B >= min_batches) {
            const float2 m2 = mb2[(size_t)y * pairs * 2 + x];
            v = fmaxf(quad_form(g0, g1, g2, ma[p], m2.x, m2.y, B), 0.f) / spp;
        }
    }
    c[p] = make_float4(r, g, b, v);
}

// everything as after create, on the null stream, synchronously
int clear_adaptive(ptx_adaptive *a) {
    const size_t nt = (size_t)a->ntiles;
    PT_HC(a->d_samples.zero()); PT_HC(a->d_batches.zero());
    PT_HC(a->d_nest.zero()); PT_HC(a->d_err.zero());
    PT_HC(a->d_kt.zero());
    PT_HC(hipMemset(a->d_out, 0, sizeof(ptx_adaptive_status)));
    PT_HC(hipMemset(a->d_active(), 1, nt));
    PT_HC(a->d_frame.zero());
    PT_HC(hipDeviceSynchronize());
    a->h_active.assign(nt, 1); a->h_samples.assign(nt, 0); a->h_k.assign(nt, 0);
    a->rounds = 0;
    return PTX_OK;
}

int alloc_adaptive(ptx_adaptive *a) {
    a->ntiles = pt_moments_tiles(a->w, a->h);
    const size_t nt = (size_t)a->ntiles, bytes = sizeof(ptx_adaptive_status) + nt;
    PT_HC(hipSetDevice(a->device));
    PT_HC(a->d_samples.alloc(nt)); PT_HC(a->d_batches.alloc(nt));
    PT_HC(a->d_nest.alloc(nt)); PT_HC(a->d_err.alloc(nt));
    PT_HC(a->d_kt.alloc(nt));
    PT_HC(a->d_out.alloc(bytes));
    PT_HC(hipHostMalloc(&a->h_out, bytes, hipHostMallocDefault));
    PT_HC(a->d_frame.alloc(3 * (size_t)a->w * a->h));
    PT_HC(a->ev.create(hipEventDisableTiming));
    return clear_adaptive(a);
}

}  // namespace

const char *pt_adaptive_params_problem(const ptx_adaptive_params &p) {
    if (!(p.target > 0.f) || isinf(p.target)) return "ptx_adaptive_params.target must be finite and positive";
    if (!(p.floor > 0.f) || isinf(p.floor)) return "ptx_adaptive_params.floor must be finite and positive";
    if (p.min_batches < 2) return "ptx_adaptive_params.min_batches must be >= 2";
    if (p.max_samples < 1) return "ptx_adaptive_params.max_samples must be >= 1";
    return nullptr;
}

hipError_t pt_tile_mask_enqueue(hipStream_t st, int ntiles, const uint8_t *flags, uint8_t *keep, const uint32_t *base, uint32_t *eff) {
    hipLaunchKernelGGL(k_tile_mask, dim3((unsigned)((ntiles + NT - 1) / NT)), dim3(NT), 0, st, ntiles, flags, keep, base, eff);
    return hipGetLastError();
}

hipError_t pt_adaptive_advance_enqueue(hipStream_t st, const ptx_adaptive &a, int k) {
    hipLaunchKernelGGL(k_adaptive_advance, dim3((unsigned)((a.ntiles + NT - 1) / NT)), dim3(NT), 0, st, a.ntiles, k, (const uint8_t *)a.d_active(),
                       a.d_samples, a.d_batches, a.d_kt);
    return hipGetLastError();
}

hipError_t pt_adaptive_select_enqueue(hipStream_t st, const ptx_adaptive &a, const PtMomentsState &s, const ptx_adaptive_params &p, int rounds) {
    const int npix = a.w * a.h;
    hipLaunchKernelGGL(k_adaptive_select, dim3((unsigned)a.ntiles), dim3(NT), 0, st, a.w, npix, pt_moments_pairs(a.w), ptx_tile_pixels(), p.floor,
                       p.target, p.min_batches, p.max_samples, (const float4 *)s.snap, (const float4 *)s.mean, (const float4 *)s.ma,
                       reinterpret_cast<const float2 *>(s.mb), (const int32_t *)a.d_samples, (const int32_t *)a.d_batches, a.d_err, a.d_nest,
                       a.d_active());
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_adaptive_status, dim3(1), dim3(NT), 0, st, a.ntiles, npix, ptx_tile_pixels(), rounds, (const int32_t *)a.d_samples,
                       (const float *)a.d_err, (const int32_t *)a.d_nest, (const uint8_t *)a.d_active(),
                       reinterpret_cast<ptx_adaptive_status *>(a.d_out.p));
    return hipGetLastError();
}

hipError_t pt_adaptive_resolve_enqueue(hipStream_t st, const ptx_adaptive &a, const float *acc) {
    const int npix = a.w * a.h;
    hipLaunchKernelGGL(k_adaptive_resolve, dim3((unsigned)((npix + NT - 1) / NT)), dim3(NT), 0, st, npix, ptx_tile_pixels(), acc,
                       (const int32_t *)a.d_samples, a.d_frame);
    return hipGetLastError();
}

hipError_t pt_adaptive_prep_enqueue(hipStream_t st, const ptx_adaptive &a, const float *acc, const float4 *nh, const float4 *alb, int demod,
                                    const PtMomentsState &s, int min_batches, float4 *c) {
    hipLaunchKernelGGL(k_adaptive_prep, pt_pixel_grid(a.w, a.h), dim3(PT_BX, PT_BY), 0, st, a.w, a.h, pt_moments_pairs(a.w), ptx_tile_pixels(), acc,
                       (const int32_t *)a.d_samples, nh, alb, demod, (const float4 *)s.mean, (const float4 *)s.ma,
                       reinterpret_cast<const float2 *>(s.mb), (float)min_batches, c, a.d_frame);
    return hipGetLastError();
}

extern "C" {

void ptx_default_adaptive_params(ptx_adaptive_params *p) {
    if (!p) return;
    p->target = 0.02f;         // stated, not tuned
    p->floor = 0.05f;          // ptx_moments_params.floor's
    p->min_batches = 4;
    p->max_samples = 1 << 20;
}

size_t ptx_sizeof_adaptive_params(void) { return sizeof(ptx_adaptive_params); }
size_t ptx_sizeof_adaptive_status(void) { return sizeof(ptx_adaptive_status); }

int ptx_adaptive_create(int device, int width, int height, ptx_adaptive **out) {
    return pt_handle_create("ptx_adaptive_create", "the adaptive handle", device, width, height, INT_MAX / 4, out, alloc_adaptive);
}

void ptx_adaptive_destroy(ptx_adaptive *a) { pt_handle_destroy(a); }

int ptx_adaptive_reset(ptx_adaptive *a) {
    if (!a) return pt_fail(PTX_ERR_INVALID, "ptx_adaptive_reset: null adaptive handle");
    PT_HC(hipSetDevice(a->device));
    PT_HC(a->wait_host());
    return clear_adaptive(a);
}

int ptx_adaptive_read(ptx_adaptive *a, float *mean_rgb, int32_t *samples_per_pixel, float *tile_error, uint8_t *tile_active) {
    if (!a) return pt_fail(PTX_ERR_INVALID, "ptx_adaptive_read: null adaptive handle");
    const size_t n = (size_t)a->w * a->h, nt = (size_t)a->ntiles;
    PT_HC(hipSetDevice(a->device));
    PT_HC(a->wait_host());
    if (mean_rgb) PT_HC(hipMemcpy(mean_rgb, a->d_frame, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
    if (tile_error) PT_HC(hipMemcpy(tile_error, a->d_err, sizeof(float) * nt, hipMemcpyDeviceToHost));
    if (tile_active) PT_HC(hipMemcpy(tile_active, a->d_active(), nt, hipMemcpyDeviceToHost));
    if (samples_per_pixel) {
        std::vector<int32_t> s(nt);
        PT_HC(hipMemcpy(s.data(), a->d_samples, sizeof(int32_t) * nt, hipMemcpyDeviceToHost));
        const size_t tp = (size_t)ptx_tile_pixels();
        for (size_t p = 0; p < n; p++) samples_per_pixel[p] = s[p / tp];
    }
    return PTX_OK;
}

float *ptx_adaptive_device_frame(ptx_adaptive *a) { return a ? a->d_frame : nullptr; }
int ptx_adaptive_num_tiles(const ptx_adaptive *a) { return a ? a->ntiles : 0; }

}  // extern "C"
