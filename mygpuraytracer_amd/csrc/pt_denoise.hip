// pt_denoise.hip -- edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) and its variance guidance (the
// middle of SVGF, Schied et al., HPG 2017: a per-pixel estimate of the variance of the filter's input, a luminance weight normalised by
// it, and its propagation through the passes) for the denoiser entry points of include/mi355x_pathtracer.h.  The G-buffer that guides
// it is written by k_gbuffer in pt_engine.hip, the temporal side of the variance estimate by k_reproject_variance (pt_temporal.hip);
// this file only filters.
//
// Kernels (all fp32, exact arithmetic, plain vector loads and stores, layouts in pt_denoise.h):
//   k_atrous_prep / k_variance_prep_state : the float4(rgb, v) colour buffer, from rgb / spp (/ max(albedo, 1e-3) on hit pixels when
//       demodulating) or from a temporal state
//   k_variance_spatial  : the windowed estimate for the pixels marked v < 0.  A workgroup none of whose pixels is marked leaves after
//       one load per lane and one barrier (after a camera step almost every pixel has history); otherwise it stages its 64 x 4 tile
//       plus an apron of r (normal + hit, position + luminance, ids: 40 B per pixel) in LDS once, and the waves with a marked pixel read
//       their 2 x (2r+1)^2 taps from there.  Two sweeps (mean, then squared deviations): sum w l^2 / sum w - lbar^2 cancels in fp32.
//   k_atrous_pass<VAR, LAST> : one 5x5 a-trous pass at step 2^i; the last pass writes W*H*3 floats, multiplied back by the albedo
//       factor.  The VAR instances weigh by luminance and carry v; their 3 x 3 prefilter of v reads neighbours at distance 1 while the
//       taps are at distance 2^i, so the tile's v plus a one-pixel apron goes through LDS (1.6 KB) -- cheaper than a pass of its own (a
//       launch and W*H*4 B each way per pass) and the nine values are shared by the tile's neighbours.  The plain instances have no LDS.
// One thread per pixel, workgroups of 64 x 4 pixels (a wave is one 64-pixel row segment: every tap it reads is 1 KB contiguous).  Each
// pass reads its own pixel's 48 B of records from HBM and the other 24 taps' through the caches.  The three edge-stopping weights are
// evaluated as ONE exponential, exp2(-(|dc|^2 kc + |dn|^2 kn + |dx|^2 kx)), or exp2(-(|dl| kl + ...)) with the per-pixel kl of the
// variance guidance, with the per-pass constants (log2 e folded in) computed on the host in double -- the same product as the three
// factors of the definition.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include <string>
#include <utility>
#include <vector>

#include "pt_denoise.h"

namespace {

constexpr int BX = PT_BX, BY = PT_BY;
constexpr int RMAX = 3;                                  // ptx_variance_params.spatial_radius <= 3
constexpr int SPATIAL_TILE = (BX + 2 * RMAX) * (BY + 2 * RMAX);      // 700 pixels: 28,000 B of LDS per workgroup

__global__ __launch_bounds__(256) void k_atrous_prep(int n, const float *__restrict__ rgb, float spp, const float4 *__restrict__ nh,
                                                     const float4 *__restrict__ alb, int demod, int variance,
                                                     const float *__restrict__ var1, float4 *__restrict__ c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r = rgb[3 * (size_t)i] / spp, g = rgb[3 * (size_t)i + 1] / spp, b = rgb[3 * (size_t)i + 2] / spp;
    const bool hit = (demod || variance) && nh[i].w != 0.f;
    if (demod && hit) {
        const float4 a = alb[i];
        r = r / fmaxf(a.x, 1e-3f); g = g / fmaxf(a.y, 1e-3f); b = b / fmaxf(a.z, 1e-3f);
    }
    c[i] = make_float4(r, g, b, variance && hit ? (var1 ? fmaxf(var1[i], 0.f) : -1.f) : 0.f);
}

__global__ __launch_bounds__(256) void k_variance_prep_state(int n, const float4 *__restrict__ nh, const float4 *__restrict__ xn,
                                                             const float4 *__restrict__ dd, float4 *__restrict__ c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 d = dd[i];
    c[i] = make_float4(d.x, d.y, d.z, nh[i].w != 0.f ? d.w / xn[i].w : 0.f);
}

// cv is the float4(rgb, v) buffer as floats: every workgroup reads floats 0..2 of its tile's and apron's pixels and writes float 3 of its
// own marked pixels, so no address is read by one workgroup and written by another.
__global__ __launch_bounds__(BX * BY) void k_variance_spatial(int w, int h, int r, float kn, float kx, const float4 *__restrict__ nh,
                                                              const float4 *__restrict__ xn, const int2 *__restrict__ ids,
                                                              int count_from_xn, float *cv) {
    __shared__ float4 s_nh[SPATIAL_TILE];                // normal xyz, hit
    __shared__ float4 s_xl[SPATIAL_TILE];                // position xyz, luminance
    __shared__ int2 s_id[SPATIAL_TILE];
    const int x0 = blockIdx.x * BX, y0 = blockIdx.y * BY;
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    const bool inside = x < w && y < h;
    const int p = y * w + x;
    const bool need = inside && cv[4 * (size_t)p + 3] < 0.f;
    if (!__syncthreads_or(need)) return;                 // nothing to estimate in this tile
    const int tw = BX + 2 * r, th = BY + 2 * r;
    for (int i = threadIdx.y * BX + threadIdx.x; i < tw * th; i += BX * BY) {
        const int ty = i / tw, tx = i - ty * tw;
        const int gx = min(max(x0 - r + tx, 0), w - 1), gy = min(max(y0 - r + ty, 0), h - 1);      // taps clamped to the frame
        const size_t q = (size_t)gy * w + gx;
        const float4 xq = xn[q];
        s_nh[i] = nh[q];
        s_xl[i] = make_float4(xq.x, xq.y, xq.z, pt_luminance(cv[4 * q], cv[4 * q + 1], cv[4 * q + 2]));
        s_id[i] = ids ? ids[q] : make_int2(0, 0);
    }
    __syncthreads();
    if (!need) return;
    const int ci = ((int)threadIdx.y + r) * tw + (int)threadIdx.x + r;
    const float4 np = s_nh[ci], xp = s_xl[ci];
    const int2 id = s_id[ci];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, lbar = 0.f;
    for (int sweep = 0; sweep < 2; sweep++) {
        for (int j = -r; j <= r; j++) {
            for (int i = -r; i <= r; i++) {
                const int t = ci + j * tw + i;
                const float4 nq = s_nh[t];
                const int2 iq = s_id[t];
                if (nq.w == 0.f || iq.x != id.x || iq.y != id.y) continue;
                const float4 xq = s_xl[t];
                const float n0 = np.x - nq.x, n1 = np.y - nq.y, n2 = np.z - nq.z;
                const float d0 = xp.x - xq.x, d1 = xp.y - xq.y, d2 = xp.z - xq.z;
                const float wt = exp2f(-((n0 * n0 + n1 * n1 + n2 * n2) * kn + (d0 * d0 + d1 * d1 + d2 * d2) * kx));
                if (sweep == 0) { s0 += wt; s1 += wt * xq.w; }
                else { const float d = xq.w - lbar; s2 += wt * d * d; }
            }
        }
        lbar = s1 / s0;                                  // s0 >= 1: the centre tap
    }
    cv[4 * (size_t)p + 3] = (count_from_xn ? xn[p].w : 1.f) * (s2 / s0);
}

// vp (VAR only): phi_luminance, epsilon and prefilter of the variance guidance; var_in / var_out (VAR only, may be NULL): v0 / the last v
template <bool VAR, bool LAST>
__global__ __launch_bounds__(BX * BY) void k_atrous_pass(int w, int h, int step, float kc, float kn, float kx, const ptx_variance_params vp,
                                                         const float4 *__restrict__ nh, const float4 *__restrict__ xt,
                                                         const float4 *__restrict__ cin, float4 *__restrict__ cout,
                                                         const float4 *__restrict__ alb, int demod, float *__restrict__ out,
                                                         float *__restrict__ var_in, float *__restrict__ var_out) {
    __shared__ float s_v[(BY + 2) * (BX + 2)];           // VAR: v of the tile and a one-pixel apron, -1 on miss pixels
    const int x0 = blockIdx.x * BX, y0 = blockIdx.y * BY;
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (VAR && vp.prefilter) {
        for (int i = threadIdx.y * BX + threadIdx.x; i < (BY + 2) * (BX + 2); i += BX * BY) {
            const int ty = i / (BX + 2), tx = i - ty * (BX + 2);
            const int gx = min(max(x0 - 1 + tx, 0), w - 1), gy = min(max(y0 - 1 + ty, 0), h - 1);
            const size_t q = (size_t)gy * w + gx;
            s_v[i] = nh[q].w != 0.f ? cin[q].w : -1.f;
        }
        __syncthreads();
    }
    if (x >= w || y >= h) return;
    const int p = y * w + x;
    const float4 np = nh[p], cp = cin[p];
    float4 res = make_float4(cp.x, cp.y, cp.z, 0.f);     // miss pixels pass through, with v = 0
    if (np.w != 0.f) {
        float kl = 0.f, lp = 0.f;                        // VAR: the luminance weight's per-pixel constant and the centre's luminance
        if (VAR) {
            float g = cp.w;
            if (vp.prefilter) {
                const float k[3] = {0.25f, 0.5f, 0.25f};
                float gs = 0.f, ks = 0.f;
#pragma unroll
                for (int j = 0; j < 3; j++) {
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        const float v = s_v[((int)threadIdx.y + j) * (BX + 2) + (int)threadIdx.x + i];
                        if (v < 0.f) continue;
                        gs += k[i] * k[j] * v; ks += k[i] * k[j];
                    }
                }
                g = gs / ks;                             // ks >= 1/4: the centre tap
            }
            kl = 1.4426950408889634f / (vp.phi_luminance * sqrtf(g) + vp.epsilon);
            lp = pt_luminance(cp.x, cp.y, cp.z);
        }
        const float4 xp = xt[p];
        const float b[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
        float sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f, sw = 0.f;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const int yy = min(max(y + (j - 2) * step, 0), h - 1);
#pragma unroll
            for (int i = 0; i < 5; i++) {
                const int xx = min(max(x + (i - 2) * step, 0), w - 1);
                const int q = yy * w + xx;
                const float4 nq = nh[q];
                if (nq.w == 0.f) continue;                   // a miss tap weighs 0
                const float4 cq = cin[q], xq = xt[q];
                float ec;                                    // the colour term of the exponent: |dl| kl or |dc|^2 kc
                if (VAR) {
                    ec = fabsf(lp - pt_luminance(cq.x, cq.y, cq.z)) * kl;
                } else {
                    const float c0 = cp.x - cq.x, c1 = cp.y - cq.y, c2 = cp.z - cq.z;
                    ec = (c0 * c0 + c1 * c1 + c2 * c2) * kc;
                }
                const float n0 = np.x - nq.x, n1 = np.y - nq.y, n2 = np.z - nq.z;
                const float d0 = xp.x - xq.x, d1 = xp.y - xq.y, d2 = xp.z - xq.z;
                const float dn2 = n0 * n0 + n1 * n1 + n2 * n2, dx2 = d0 * d0 + d1 * d1 + d2 * d2;
                const float wt = b[i] * b[j] * exp2f(-(ec + dn2 * kn + dx2 * kx));
                sr += wt * cq.x; sg += wt * cq.y; sb += wt * cq.z; sw += wt;
                if (VAR) sv += wt * wt * cq.w;
            }
        }
        res = make_float4(sr / sw, sg / sw, sb / sw, VAR ? sv / (sw * sw) : 0.f);    // sw >= 9/64: the centre tap
    }
    if (VAR && var_in) var_in[p] = cp.w;
    if (LAST) {
        if (VAR && var_out) var_out[p] = res.w;
        if (demod && np.w != 0.f) {
            const float4 a = alb[p];
            res.x = res.x * fmaxf(a.x, 1e-3f); res.y = res.y * fmaxf(a.y, 1e-3f); res.z = res.z * fmaxf(a.z, 1e-3f);
        }
        out[3 * (size_t)p] = res.x; out[3 * (size_t)p + 1] = res.y; out[3 * (size_t)p + 2] = res.z;
    } else {
        cout[p] = res;
    }
}

// The two ptx_denoise_buffers* entry points: arguments checked under the caller's name `fn`, float3 -> float4 staging, upload, the
// filter on the null stream, download.  variance == false: the plain filter (ids2, var1, vparams and out_var1 are not looked at).
int denoise_buffers(const char *fn, bool variance, int device, int w, int h, const float *rgb, const float *alb3, const float *nrm3,
                    const float *pos3, const uint8_t *hit, const int32_t *ids2, const float *var1, const ptx_denoise_params *dparams,
                    const ptx_variance_params *vparams, float *out_rgb, float *out_var1) {
    const std::string name = fn;
    ptx_denoise_params dp;
    ptx_variance_params vp;
    if (dparams) dp = *dparams;
    else ptx_default_denoise_params(&dp);
    if (vparams) vp = *vparams;
    else ptx_default_variance_params(&vp);
    if (w < 1 || h < 1 || (long long)w * h > INT_MAX / (variance ? 4 : 3)) return pt_fail(PTX_ERR_INVALID, name + ": bad frame size");
    if (!rgb || !nrm3 || !pos3 || !hit || !out_rgb) return pt_fail(PTX_ERR_INVALID, name + ": rgb, nrm3, pos3, hit and out_rgb are required");
    if (dp.demodulate && !alb3) return pt_fail(PTX_ERR_INVALID, name + ": demodulation needs alb3");
    if (const char *why = pt_denoise_params_problem(dp)) return pt_fail(PTX_ERR_INVALID, why);
    if (const char *why = variance ? pt_variance_params_problem(vp) : nullptr) return pt_fail(PTX_ERR_INVALID, why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return pt_fail(PTX_ERR_NODEVICE, "no HIP device available; the denoiser has no CPU path");
    }
    if (device < 0 || device >= ndev) return pt_fail(PTX_ERR_INVALID, name + ": device ordinal out of range");
    const size_t n = (size_t)w * h;
    std::vector<float4> hnh(n), hxt(n), hal(n);
    for (size_t i = 0; i < n; i++) {
        const bool on = hit[i] != 0;
        hnh[i] = make_float4(nrm3[3 * i], nrm3[3 * i + 1], nrm3[3 * i + 2], on ? 1.f : 0.f);
        hxt[i] = make_float4(pos3[3 * i], pos3[3 * i + 1], pos3[3 * i + 2], 0.f);
        hal[i] = alb3 ? make_float4(alb3[3 * i], alb3[3 * i + 1], alb3[3 * i + 2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    PT_HC(hipSetDevice(device));
    DevBuf<float> d_rgb, d_out, d_var, d_vout;           // (n >= 1: no array of no elements)
    DevBuf<float4> d_nh, d_xt, d_al, d_t0, d_t1;
    DevBuf<int2> d_ids;
    PT_HC(d_out.alloc(3 * n)); PT_HC(d_t0.alloc(n)); PT_HC(d_t1.alloc(n));
    PT_HC(d_rgb.upload(rgb, 3 * n));
    PT_HC(d_nh.upload(hnh.data(), n)); PT_HC(d_xt.upload(hxt.data(), n)); PT_HC(d_al.upload(hal.data(), n));
    if (variance) {
        PT_HC(d_vout.alloc(n));
        if (var1) PT_HC(d_var.upload(var1, n));
        else if (ids2) PT_HC(d_ids.upload(ids2, n));
    }
    PT_HC(pt_atrous_prep_enqueue(nullptr, (int)n, d_rgb.p, 1.0f, d_nh.p, d_al.p, dp.demodulate ? 1 : 0, variance ? 1 : 0, d_var.p, d_t0.p));
    if (variance && !var1) PT_HC(pt_variance_spatial_enqueue(nullptr, w, h, dp, vp, d_nh.p, d_xt.p, d_ids.p, 0, d_t0.p));
    PT_HC(pt_atrous_enqueue(nullptr, w, h, d_nh.p, d_xt.p, d_al.p, d_t0.p, d_t1.p, d_out.p, dp, variance ? &vp : nullptr, nullptr, d_vout.p));
    PT_HC(hipStreamSynchronize(nullptr));
    PT_HC(hipMemcpy(out_rgb, d_out.p, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
    if (variance && out_var1) PT_HC(hipMemcpy(out_var1, d_vout.p, sizeof(float) * n, hipMemcpyDeviceToHost));
    return PTX_OK;
}

}  // namespace

const char *pt_denoise_params_problem(const ptx_denoise_params &p) {
    if (p.passes < 1 || p.passes > 10) return "ptx_denoise_params.passes must be 1 .. 10";
    if (!(p.phi_color > 0.f) || !(p.phi_normal > 0.f) || !(p.phi_position > 0.f))
        return "ptx_denoise_params: phi_color, phi_normal and phi_position must be positive";
    return nullptr;
}

const char *pt_variance_params_problem(const ptx_variance_params &p) {
    if (!(p.phi_luminance > 0.f) || isinf(p.phi_luminance)) return "ptx_variance_params.phi_luminance must be finite and positive";
    if (!(p.epsilon > 0.f) || isinf(p.epsilon)) return "ptx_variance_params.epsilon must be finite and positive";
    if (p.spatial_radius < 1 || p.spatial_radius > RMAX) return "ptx_variance_params.spatial_radius must be 1 .. 3";
    return nullptr;
}

hipError_t pt_atrous_prep_enqueue(hipStream_t st, int n, const float *rgb, float spp, const float4 *nh, const float4 *alb, int demod,
                                  int variance, const float *var1, float4 *c) {
    hipLaunchKernelGGL(k_atrous_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rgb, spp, nh, alb, demod, variance, var1, c);
    return hipGetLastError();
}

hipError_t pt_variance_prep_state_enqueue(hipStream_t st, int n, const PtTemporalState &s, float4 *c) {
    hipLaunchKernelGGL(k_variance_prep_state, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const float4 *)s.nh,
                       (const float4 *)s.xn, (const float4 *)s.dd, c);
    return hipGetLastError();
}

hipError_t pt_variance_spatial_enqueue(hipStream_t st, int w, int h, const ptx_denoise_params &dp, const ptx_variance_params &vp,
                                       const float4 *nh, const float4 *xn, const int2 *ids, int count_from_xn, float4 *cv) {
    const double l2e = 1.4426950408889634;
    hipLaunchKernelGGL(k_variance_spatial, pt_pixel_grid(w, h), dim3(BX, BY), 0, st, w, h, vp.spatial_radius, (float)(l2e / dp.phi_normal),
                       (float)(l2e / dp.phi_position), nh, xn, ids, count_from_xn, reinterpret_cast<float *>(cv));
    return hipGetLastError();
}

hipError_t pt_atrous_enqueue(hipStream_t st, int w, int h, const float4 *nh, const float4 *xt, const float4 *alb, float4 *tmp0,
                             float4 *tmp1, float *out_rgb, const ptx_denoise_params &dp, const ptx_variance_params *vp, float *var_in,
                             float *var_out) {
    const int demod = dp.demodulate ? 1 : 0;
    const ptx_variance_params v = vp ? *vp : ptx_variance_params();
    float4 *src = tmp0, *dst = tmp1;
    for (int i = 0; i < dp.passes; i++) {
        const double l2e = 1.4426950408889634, s = (double)(1 << i);
        const float kc = (float)(l2e * s / dp.phi_color), kn = (float)(l2e / (s * s * dp.phi_normal)), kx = (float)(l2e / dp.phi_position);
        const bool last = i == dp.passes - 1;
        const auto kernel = vp ? (last ? k_atrous_pass<true, true> : k_atrous_pass<true, false>)
                               : (last ? k_atrous_pass<false, true> : k_atrous_pass<false, false>);
        hipLaunchKernelGGL(kernel, pt_pixel_grid(w, h), dim3(BX, BY), 0, st, w, h, 1 << i, kc, kn, kx, v, nh, xt, src, dst, alb, demod,
                           out_rgb, i == 0 ? var_in : nullptr, var_out);
        std::swap(src, dst);
    }
    return hipGetLastError();
}

extern "C" {

void ptx_default_denoise_params(ptx_denoise_params *p) {
    if (!p) return;
    p->passes = 5;
    p->demodulate = 1;
    p->phi_color = 16.0f;      // chosen on the quality test's frames (tools/gpu_denoise_quality.py)
    p->phi_normal = 0.1f;
    p->phi_position = 0.5f;
}

void ptx_default_variance_params(ptx_variance_params *p) {
    if (!p) return;
    p->phi_luminance = 4.0f;       // the sweep of tools/gpu_variance_quality.py
    p->epsilon = 1e-4f;
    p->spatial_radius = 3;
    p->prefilter = 1;
}

size_t ptx_sizeof_denoise_params(void) { return sizeof(ptx_denoise_params); }
size_t ptx_sizeof_variance_params(void) { return sizeof(ptx_variance_params); }

int ptx_denoise_buffers(int device, int w, int h, const float *rgb, const float *alb3, const float *nrm3, const float *pos3,
                        const uint8_t *hit, const ptx_denoise_params *params, float *out_rgb) {
    return denoise_buffers("ptx_denoise_buffers", false, device, w, h, rgb, alb3, nrm3, pos3, hit, nullptr, nullptr, params, nullptr, out_rgb,
                           nullptr);
}

int ptx_denoise_buffers_variance(int device, int w, int h, const float *rgb, const float *alb3, const float *nrm3, const float *pos3,
                                 const uint8_t *hit, const int32_t *ids2, const float *var1, const ptx_denoise_params *dparams,
                                 const ptx_variance_params *vparams, float *out_rgb, float *out_var1) {
    return denoise_buffers("ptx_denoise_buffers_variance", true, device, w, h, rgb, alb3, nrm3, pos3, hit, ids2, var1, dparams, vparams,
                           out_rgb, out_var1);
}

}  // extern "C"
