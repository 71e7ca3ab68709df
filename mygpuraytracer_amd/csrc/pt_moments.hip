// pt_moments.hip -- per-pixel sample moments by the method of batch means (ptx_moments_* of include/mi355x_pathtracer.h): the
// per-sample covariance of a pixel's radiance from successive states of the accumulation buffer alone, a frame-level error summary
// reduced on the device, and the a-trous filter's prep with the measured variance.  ptx_moments_add and ptx_denoise_measured are
// pt_engine.hip's: they need the tracer's accumulation buffer, stream and G-buffer.  State layout in pt_denoise.h.
//
// Kernels (all fp32 per pixel, exact arithmetic, one thread per pixel, workgroups of 64 x 4 pixels as the filter's):
//   k_moments_add     : West's weighted update of mean and scatter matrix by the batch between the snapshot and the frame, new snapshot.
//       12 B read from the frame, 56 B read and 56 B written of state per pixel (124 B), in 16-byte loads and stores only: the pair
//       (rb, gb) shares a float4 with the row neighbour's; the even lane moves it and the odd lane's half crosses by a DPP quad
//       permutation.  No atomics, no LDS, no scratch.
//   k_moments_summary : stage one, the per-pixel relative standard error of the luminance and a workgroup's sums of it (a fixed-order
//       tree in LDS, sums in double) into one partial per workgroup.
//   k_moments_total   : stage two, one workgroup: thread t sums a contiguous run of partials in index order, then the same tree.  No
//       float atomics anywhere, so the summary is the same bits on every run.
//   k_moments_prep    : k_atrous_prep with v = g^T C g / W from the state (a kernel of its own: pt_denoise.hip's are not touched).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include <algorithm>
#include <string>
#include <vector>

#include "pt_denoise.h"

namespace {

constexpr int BX = PT_BX, BY = PT_BY, NT = BX * BY;
constexpr float LR = 0.2126f, LG = 0.7152f, LB = 0.0722f;   // pt_luminance's weights

// the value of lane ^ 1 (quad_perm [1, 0, 3, 2]); every lane of the wave must be active
__device__ __forceinline__ float pair_swap(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}

__global__ __launch_bounds__(NT) void k_moments_add(int w, int h, int pairs, float k, float total, int fresh, const float *__restrict__ rgb,
                                                    float4 *__restrict__ snap, float4 *__restrict__ mean, float4 *__restrict__ ma,
                                                    float4 *__restrict__ mb) {
    const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
    const bool inside = x < w && y < h;                  // (no early return: the lanes outside still serve pair_swap)
    const bool even = (threadIdx.x & 1) == 0;
    const size_t p = (size_t)y * w + x, pb = (size_t)y * pairs + (x >> 1);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), mu = s, A = s, Bq = s;
    if (inside) {
        a0 = rgb[3 * p]; a1 = rgb[3 * p + 1]; a2 = rgb[3 * p + 2];
        if (!fresh) {
            s = snap[p]; mu = mean[p]; A = ma[p];
            if (even) Bq = mb[pb];
        }
    }
    const float orb = pair_swap(Bq.z), ogb = pair_swap(Bq.w);     // the odd lane's (rb, gb), held by its even neighbour
    float rb = even ? Bq.x : orb, gb = even ? Bq.y : ogb;
    // d = x - mean with mean = snap / W (the weighted mean of the batch means IS the buffer over its samples), so
    // d = D / (k W), D = W acc - W' snap, and the scatter term k d (x - mean')^T = D D^T / (k W W').  D is formed from the two buffers by
    // exact products (the fma returns a product's rounding error), so it is right to an ulp of ITSELF however close the batch mean is to
    // the running one; through x = fl(acc - snap) / k and a stored mean it would carry an ulp of the colour.  This needs the unit's
    // -ffp-contract=off: p1 - p2 contracted into fma(acc, wo, -p2) is no longer the difference the two residuals complete.  Held to
    // (B + 8) 2^-23 sqrt(C_ii C_jj) by tests/test_gpu_moments_grid.py down to a relative noise of 1e-6 and up to W' = 2^24.
    const float wo = total - k;
    if (wo > 0.f) {
        const float kw = k * wo, den = kw * total, r = k / total;
        float D[3];
        const float acc[3] = {a0, a1, a2}, old[3] = {s.x, s.y, s.z};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float p1 = acc[c] * wo, p2 = old[c] * total;
            D[c] = (p1 - p2) + (__fmaf_rn(acc[c], wo, -p1) - __fmaf_rn(old[c], total, -p2));
        }
        mu.x = mu.x + r * (D[0] / kw); mu.y = mu.y + r * (D[1] / kw); mu.z = mu.z + r * (D[2] / kw);
        A.x = A.x + (D[0] * D[0]) / den; A.y = A.y + (D[1] * D[1]) / den; A.z = A.z + (D[2] * D[2]) / den; A.w = A.w + (D[0] * D[1]) / den;
        rb = rb + (D[0] * D[2]) / den; gb = gb + (D[1] * D[2]) / den;
    } else {                                             // the first add: one batch, no scatter yet (s, mu, A, rb, gb are zeros)
        mu.x = a0 / k; mu.y = a1 / k; mu.z = a2 / k;
    }
    mu.w = mu.w + 1.f;
    const float nrb = pair_swap(rb), ngb = pair_swap(gb);         // the neighbour's (zeros from a lane outside the frame)
    if (!inside) return;
    snap[p] = make_float4(a0, a1, a2, total);
    mean[p] = mu;
    ma[p] = A;
    if (even) mb[pb] = make_float4(rb, gb, nrb, ngb);
}

// k_moments_add with k and W' of the pixel's tile (kt[(y w + x) / tile_px]): the same arithmetic on the pixels of a tile that advances.
// A tile with k == 0 is idle: its pixels are not stored (fresh: stored as zeros), and their half of a shared (rb, gb) record goes back
// with the bits it came with -- a record whose two pixels are both idle is not stored at all.
__global__ __launch_bounds__(NT) void k_moments_add_tiled(int w, int h, int pairs, int tile_px, const float2 *__restrict__ kt, int fresh,
                                                          const float *__restrict__ rgb, float4 *__restrict__ snap, float4 *__restrict__ mean,
                                                          float4 *__restrict__ ma, float4 *__restrict__ mb) {
    const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
    const bool inside = x < w && y < h;                  // (no early return: the lanes outside still serve pair_swap)
    const bool even = (threadIdx.x & 1) == 0;
    const size_t p = (size_t)y * w + x, pb = (size_t)y * pairs + (x >> 1);
    float k = 0.f, total = 0.f;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), mu = s, A = s, Bq = s;
    if (inside) {
        const float2 t = kt[p / (size_t)tile_px];
        k = t.x; total = t.y;
        if (k > 0.f) { a0 = rgb[3 * p]; a1 = rgb[3 * p + 1]; a2 = rgb[3 * p + 2]; }
        if (!fresh) {
            if (k > 0.f) { s = snap[p]; mu = mean[p]; A = ma[p]; }
            if (even) Bq = mb[pb];
        }
    }
    const bool live = k > 0.f;
    const float orb = pair_swap(Bq.z), ogb = pair_swap(Bq.w);     // the odd lane's (rb, gb), held by its even neighbour
    float rb = even ? Bq.x : orb, gb = even ? Bq.y : ogb;
    if (live) {
        const float wo = total - k;
        if (wo > 0.f) {                                  // (k_moments_add's update, operation for operation)
            const float kw = k * wo, den = kw * total, r = k / total;
            float D[3];
            const float acc[3] = {a0, a1, a2}, old[3] = {s.x, s.y, s.z};
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float p1 = acc[c] * wo, p2 = old[c] * total;
                D[c] = (p1 - p2) + (__fmaf_rn(acc[c], wo, -p1) - __fmaf_rn(old[c], total, -p2));
            }
            mu.x = mu.x + r * (D[0] / kw); mu.y = mu.y + r * (D[1] / kw); mu.z = mu.z + r * (D[2] / kw);
            A.x = A.x + (D[0] * D[0]) / den; A.y = A.y + (D[1] * D[1]) / den; A.z = A.z + (D[2] * D[2]) / den; A.w = A.w + (D[0] * D[1]) / den;
            rb = rb + (D[0] * D[2]) / den; gb = gb + (D[1] * D[2]) / den;
        } else {                                         // the tile's first add: one batch, no scatter yet
            mu.x = a0 / k; mu.y = a1 / k; mu.z = a2 / k;
        }
        mu.w = mu.w + 1.f;
    }
    const float nrb = pair_swap(rb), ngb = pair_swap(gb);         // the neighbour's (zeros from a lane outside the frame)
    const bool nlive = pair_swap(live ? 1.f : 0.f) != 0.f;
    if (!inside) return;
    if (live || fresh) {
        snap[p] = live ? make_float4(a0, a1, a2, total) : s;      // (an idle pixel of a fresh handle: s, mu, A are zeros)
        mean[p] = mu;
        ma[p] = A;
    }
    if (even && (live || nlive || fresh)) mb[pb] = make_float4(rb, gb, nrb, ngb);
}

__device__ __forceinline__ void partial_add(PtMomentsPartial &a, const PtMomentsPartial &b) {
    a.sum_rel += b.sum_rel; a.sum_rel2 += b.sum_rel2; a.sum_q += b.sum_q;
    a.max_rel = fmax(a.max_rel, b.max_rel);
    a.n += b.n; a.over += b.over;
}

// the workgroup's total in thread 0's v: a tree of fixed shape
__device__ __forceinline__ void block_total(PtMomentsPartial &v, int tid) {
    __shared__ PtMomentsPartial s_p[NT];
    s_p[tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) partial_add(s_p[tid], s_p[tid + s]);
        __syncthreads();
    }
    v = s_p[0];
}

__global__ __launch_bounds__(NT) void k_moments_summary(int w, int h, int pairs, float floor_l, float threshold, const float4 *__restrict__ snap,
                                                        const float4 *__restrict__ mean, const float4 *__restrict__ ma,
                                                        const float2 *__restrict__ mb2, PtMomentsPartial *__restrict__ part) {
    const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
    const int tid = threadIdx.y * BX + threadIdx.x;
    PtMomentsPartial v = {0.0, 0.0, 0.0, 0.0, 0ull, 0ull};
    if (x < w && y < h) {
        const size_t p = (size_t)y * w + x;
        const float4 mu = mean[p];
        if (mu.w >= 2.f) {
            const float2 b = mb2[(size_t)y * pairs * 2 + x];
            const float q = fmaxf(quad_form(LR, LG, LB, ma[p], b.x, b.y, mu.w), 0.f);
            const float rel = sqrtf(q / snap[p].w) / fmaxf(pt_luminance(mu.x, mu.y, mu.z), floor_l);
            v.sum_rel = rel; v.sum_rel2 = (double)rel * rel; v.max_rel = rel; v.sum_q = q;
            v.n = 1ull; v.over = rel > threshold ? 1ull : 0ull;
        }
    }
    block_total(v, tid);
    if (tid == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = v;
}

// part[npart] = the sum of part[0 .. npart)
__global__ __launch_bounds__(NT) void k_moments_total(int npart, PtMomentsPartial *part) {
    const int tid = threadIdx.x;
    const int run = (npart + NT - 1) / NT;
    PtMomentsPartial v = {0.0, 0.0, 0.0, 0.0, 0ull, 0ull};
    for (int i = tid * run; i < min((tid + 1) * run, npart); i++) partial_add(v, part[i]);
    block_total(v, tid);
    if (tid == 0) part[npart] = v;
}

__global__ __launch_bounds__(NT) void k_moments_prep(int w, int h, int pairs, const float *__restrict__ rgb, float spp, const float4 *__restrict__ nh,
                                                     const float4 *__restrict__ alb, int demod, const float4 *__restrict__ snap,
                                                     const float4 *__restrict__ mean, const float4 *__restrict__ ma,
                                                     const float2 *__restrict__ mb2, float min_batches, float4 *__restrict__ c) {
    const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    float r = rgb[3 * p] / spp, g = rgb[3 * p + 1] / spp, b = rgb[3 * p + 2] / spp;      // = k_atrous_prep
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
            v = fmaxf(quad_form(g0, g1, g2, ma[p], m2.x, m2.y, B), 0.f) / snap[p].w;
        }
    }
    c[p] = make_float4(r, g, b, v);
}

int alloc_moments(ptx_moments *m) {
    const size_t n = (size_t)m->w * m->h;
    const dim3 grid = pt_pixel_grid(m->w, m->h);
    PT_HC(hipSetDevice(m->device));
    PT_HC(m->d_snap.alloc(n)); PT_HC(m->d_mean.alloc(n));
    PT_HC(m->d_ma.alloc(n));
    PT_HC(m->d_mb.alloc((size_t)pt_moments_pairs(m->w) * m->h));
    m->st.snap = m->d_snap; m->st.mean = m->d_mean; m->st.ma = m->d_ma; m->st.mb = m->d_mb;
    PT_HC(m->d_part.alloc((size_t)grid.x * grid.y + 1));
    PT_HC(m->ev.create(hipEventDisableTiming));
    return PTX_OK;
}

}  // namespace

const char *pt_moments_params_problem(const ptx_moments_params &p) {
    if (!(p.floor > 0.f) || isinf(p.floor)) return "ptx_moments_params.floor must be finite and positive";
    if (!(p.threshold >= 0.f) || isinf(p.threshold)) return "ptx_moments_params.threshold must be finite and not negative";
    return nullptr;
}

hipError_t pt_moments_add_enqueue(hipStream_t st, int w, int h, const float *rgb, float k, float total, int fresh, const PtMomentsState &s) {
    hipLaunchKernelGGL(k_moments_add, pt_pixel_grid(w, h), dim3(BX, BY), 0, st, w, h, pt_moments_pairs(w), k, total, fresh, rgb, s.snap, s.mean,
                       s.ma, s.mb);
    return hipGetLastError();
}

hipError_t pt_moments_prep_enqueue(hipStream_t st, int w, int h, const float *rgb, float spp, const float4 *nh, const float4 *alb, int demod,
                                   const PtMomentsState &s, int min_batches, float4 *c) {
    hipLaunchKernelGGL(k_moments_prep, pt_pixel_grid(w, h), dim3(BX, BY), 0, st, w, h, pt_moments_pairs(w), rgb, spp, nh, alb, demod,
                       (const float4 *)s.snap, (const float4 *)s.mean, (const float4 *)s.ma, reinterpret_cast<const float2 *>(s.mb),
                       (float)min_batches, c);
    return hipGetLastError();
}

int pt_moments_add_tiled(ptx_moments *m, hipStream_t st, const float *rgb, const float2 *d_kt, const int32_t *host_k) {
    const int ntiles = pt_moments_tiles(m->w, m->h);
    bool any = false;
    for (int i = 0; i < ntiles && !any; i++) any = host_k[i] > 0;
    if (!any) return PTX_OK;
    hipLaunchKernelGGL(k_moments_add_tiled, pt_pixel_grid(m->w, m->h), dim3(BX, BY), 0, st, m->w, m->h, pt_moments_pairs(m->w), ptx_tile_pixels(),
                       d_kt, m->samples == 0 ? 1 : 0, rgb, m->st.snap, m->st.mean, m->st.ma, m->st.mb);
    PT_HC(hipGetLastError());
    if (m->tile_samples.empty()) {                       // the first tiled add: every tile stands where the handle stands
        m->tile_samples.assign((size_t)ntiles, m->samples);
        m->tile_batches.assign((size_t)ntiles, m->batches);
    }
    m->tiled = true;
    for (int i = 0; i < ntiles; i++) {
        if (host_k[i] <= 0) continue;
        m->tile_samples[(size_t)i] += host_k[i];
        m->tile_batches[(size_t)i]++;
        m->samples = std::max(m->samples, m->tile_samples[(size_t)i]);
        m->batches = std::max(m->batches, m->tile_batches[(size_t)i]);
    }
    return PTX_OK;
}

extern "C" {

void ptx_default_moments_params(ptx_moments_params *p) {
    if (!p) return;
    p->floor = 0.05f;          // stated, not tuned
    p->threshold = 0.05f;
}

size_t ptx_sizeof_moments_params(void) { return sizeof(ptx_moments_params); }
size_t ptx_sizeof_moments_summary(void) { return sizeof(ptx_moments_summary); }

int ptx_moments_create(int device, int width, int height, ptx_moments **out) {
    return pt_handle_create("ptx_moments_create", "the moments handle", device, width, height, INT_MAX / 4, out, alloc_moments);
}

void ptx_moments_destroy(ptx_moments *m) { pt_handle_destroy(m); }

int ptx_moments_reset(ptx_moments *m) {
    if (!m) return pt_fail(PTX_ERR_INVALID, "ptx_moments_reset: null moments handle");
    m->samples = 0;            // (the buffers are only read behind this: the next add takes them as zeros, and waits for the last)
    m->batches = 0;
    m->tiled = false;
    m->tile_samples.clear(); m->tile_batches.clear();
    return PTX_OK;
}

int ptx_moments_add_host(ptx_moments *m, const float *host_rgb_sum, int64_t samples_total) {
    if (samples_total < 1) return pt_fail(PTX_ERR_INVALID, "ptx_moments_add_host: samples_total must be >= 1");
    if (!m || !host_rgb_sum) return pt_fail(PTX_ERR_INVALID, "ptx_moments_add_host: null moments handle or frame");
    if (samples_total <= m->samples)
        return pt_fail(PTX_ERR_INVALID, "ptx_moments_add_host: samples_total " + std::to_string(samples_total) + " does not exceed the last add's " +
                                            std::to_string(m->samples));
    if (m->tiled) return pt_fail(PTX_ERR_INVALID, "ptx_moments_add_host: this handle has had a tiled add; its tiles hold different sample counts until ptx_moments_reset");
    if (samples_total > (1 << 24))                       // (W and k are held as floats: exact to 2^24)
        return pt_fail(PTX_ERR_INVALID, "ptx_moments_add_host: samples_total " + std::to_string(samples_total) + " is above 2^24");
    const size_t n = (size_t)m->w * m->h;
    PT_HC(hipSetDevice(m->device));
    PT_HC(m->wait_host());
    if (!m->d_stage) PT_HC(m->d_stage.alloc(3 * n));
    PT_HC(hipMemcpy(m->d_stage, host_rgb_sum, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
    PT_HC(pt_moments_add_enqueue(nullptr, m->w, m->h, m->d_stage, (float)(samples_total - m->samples), (float)samples_total, m->samples == 0, m->st));
    PT_HC(m->record(nullptr));
    m->samples = samples_total;
    m->batches++;
    PT_HC(hipEventSynchronize(m->ev));
    return PTX_OK;
}

int ptx_moments_add_host_tiled(ptx_moments *m, const float *host_rgb_sum, const int64_t *tile_samples_total, int ntiles) {
    if (!m || !host_rgb_sum || !tile_samples_total) return pt_fail(PTX_ERR_INVALID, "ptx_moments_add_host_tiled: null moments handle, frame or table");
    if (ntiles != pt_moments_tiles(m->w, m->h))
        return pt_fail(PTX_ERR_INVALID, "ptx_moments_add_host_tiled: ntiles " + std::to_string(ntiles) + " is not the frame's " +
                                            std::to_string(pt_moments_tiles(m->w, m->h)));
    std::vector<float2> kt((size_t)ntiles);
    std::vector<int32_t> hk((size_t)ntiles);
    for (int i = 0; i < ntiles; i++) {
        const long long last = m->tile_samples.empty() ? m->samples : m->tile_samples[(size_t)i], now = tile_samples_total[i];
        if (now < last || now - last > (1 << 24) || now > (1 << 24))      // (W and k are held as floats: exact to 2^24)
            return pt_fail(PTX_ERR_INVALID, "ptx_moments_add_host_tiled: tile " + std::to_string(i) + "'s total " + std::to_string(now) +
                                                (now < last ? " is below its last add's " + std::to_string(last) : std::string(" is above 2^24")));
        hk[(size_t)i] = (int32_t)(now - last);
        kt[(size_t)i] = make_float2((float)(now - last), (float)now);
    }
    const size_t n = (size_t)m->w * m->h;
    PT_HC(hipSetDevice(m->device));
    PT_HC(m->wait_host());
    if (!m->d_stage) PT_HC(m->d_stage.alloc(3 * n));
    if (!m->d_tile_kt) PT_HC(m->d_tile_kt.alloc((size_t)ntiles));
    PT_HC(hipMemcpy(m->d_stage, host_rgb_sum, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
    PT_HC(hipMemcpy(m->d_tile_kt, kt.data(), sizeof(float2) * (size_t)ntiles, hipMemcpyHostToDevice));
    if (const int rc = pt_moments_add_tiled(m, nullptr, m->d_stage, m->d_tile_kt, hk.data())) return rc;
    PT_HC(m->record(nullptr));
    PT_HC(hipEventSynchronize(m->ev));
    return PTX_OK;
}

int ptx_moments_read(ptx_moments *m, float *mean3, float *cov6, int32_t *batches1, int64_t *samples_out) {
    if (!m) return pt_fail(PTX_ERR_INVALID, "ptx_moments_read: null moments handle");
    if (samples_out) *samples_out = m->samples;
    const size_t n = (size_t)m->w * m->h, pairs = (size_t)pt_moments_pairs(m->w);
    if (m->samples == 0) {                               // fresh: everything reads as zero
        for (size_t i = 0; i < n; i++) {
            if (mean3) mean3[3 * i] = mean3[3 * i + 1] = mean3[3 * i + 2] = 0.f;
            if (cov6) for (int j = 0; j < 6; j++) cov6[6 * i + j] = 0.f;
            if (batches1) batches1[i] = 0;
        }
        return PTX_OK;
    }
    PT_HC(hipSetDevice(m->device));
    PT_HC(hipEventSynchronize(m->ev));
    std::vector<float4> mu(n), A, Bq;
    PT_HC(hipMemcpy(mu.data(), m->st.mean, sizeof(float4) * n, hipMemcpyDeviceToHost));
    if (cov6) {
        A.resize(n); Bq.resize(pairs * m->h);
        PT_HC(hipMemcpy(A.data(), m->st.ma, sizeof(float4) * n, hipMemcpyDeviceToHost));
        PT_HC(hipMemcpy(Bq.data(), m->st.mb, sizeof(float4) * pairs * m->h, hipMemcpyDeviceToHost));
    }
    for (int y = 0; y < m->h; y++)
        for (int x = 0; x < m->w; x++) {
            const size_t i = (size_t)y * m->w + x;
            const float B = mu[i].w;
            if (mean3) { mean3[3 * i] = mu[i].x; mean3[3 * i + 1] = mu[i].y; mean3[3 * i + 2] = mu[i].z; }
            if (batches1) batches1[i] = (int32_t)B;
            if (cov6) {
                const float4 q = Bq[(size_t)y * pairs + (x >> 1)];
                const float v[6] = {A[i].x, A[i].y, A[i].z, A[i].w, (x & 1) ? q.z : q.x, (x & 1) ? q.w : q.y};
                for (int j = 0; j < 6; j++) cov6[6 * i + j] = B >= 2.f ? v[j] / (B - 1.f) : 0.f;
            }
        }
    return PTX_OK;
}

int ptx_moments_read_samples(ptx_moments *m, int32_t *samples1) {
    if (!m || !samples1) return pt_fail(PTX_ERR_INVALID, "ptx_moments_read_samples: null moments handle or array");
    const size_t n = (size_t)m->w * m->h;
    if (m->samples == 0) {                               // fresh: everything reads as zero
        for (size_t i = 0; i < n; i++) samples1[i] = 0;
        return PTX_OK;
    }
    PT_HC(hipSetDevice(m->device));
    PT_HC(hipEventSynchronize(m->ev));
    std::vector<float4> s(n);
    PT_HC(hipMemcpy(s.data(), m->st.snap, sizeof(float4) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) samples1[i] = (int32_t)s[i].w;
    return PTX_OK;
}

int ptx_moments_summarize(ptx_moments *m, const ptx_moments_params *params, ptx_moments_summary *out) {
    ptx_moments_params p;
    if (params) p = *params;
    else ptx_default_moments_params(&p);
    if (const char *why = pt_moments_params_problem(p)) return pt_fail(PTX_ERR_INVALID, why);
    if (!m || !out) return pt_fail(PTX_ERR_INVALID, "ptx_moments_summarize: null moments handle or summary");
    *out = ptx_moments_summary();
    out->samples = m->samples;
    out->batches = m->batches;
    if (m->batches < 2) return PTX_OK;                   // no pixel has an estimate yet
    PT_HC(hipSetDevice(m->device));
    PT_HC(hipEventSynchronize(m->ev));
    const dim3 grid = pt_pixel_grid(m->w, m->h);
    const int npart = (int)(grid.x * grid.y);
    hipLaunchKernelGGL(k_moments_summary, grid, dim3(BX, BY), 0, nullptr, m->w, m->h, pt_moments_pairs(m->w), p.floor, p.threshold,
                       (const float4 *)m->st.snap, (const float4 *)m->st.mean, (const float4 *)m->st.ma,
                       reinterpret_cast<const float2 *>(m->st.mb), m->d_part);
    PT_HC(hipGetLastError());
    hipLaunchKernelGGL(k_moments_total, dim3(1), dim3(NT), 0, nullptr, npart, m->d_part);
    PT_HC(hipGetLastError());
    PtMomentsPartial t;
    PT_HC(hipMemcpyAsync(&t, m->d_part + npart, sizeof t, hipMemcpyDeviceToHost, nullptr));
    PT_HC(hipStreamSynchronize(nullptr));
    out->pixels = (int64_t)t.n;
    out->pixels_over = (int64_t)t.over;
    if (t.n) {
        out->mean_rel_se = t.sum_rel / (double)t.n;
        out->rms_rel_se = sqrt(t.sum_rel2 / (double)t.n);
        out->max_rel_se = t.max_rel;
        out->mean_variance = t.sum_q / (double)t.n;
    }
    return PTX_OK;
}

}  // extern "C"
