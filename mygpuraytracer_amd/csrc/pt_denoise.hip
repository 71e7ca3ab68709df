// pt_denoise.hip -- edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) for the denoiser entry points
// of include/mi355x_pathtracer.h.  The G-buffer that guides it is written by k_gbuffer in pt_engine.hip; this file only filters.
//
// Kernels (all fp32, plain vector loads and stores, guide layout in pt_denoise.h):
//   k_atrous_prep : c = rgb / spp (/ max(albedo, 1e-3) on hit pixels when demodulating) -> float4 colour buffer
//   k_atrous_pass : one 5x5 a-trous pass at step 2^i; the last pass writes W*H*3 floats, multiplied back by the albedo factor.
// One thread per pixel, workgroups of 64 x 4 pixels (a wave is one 64-pixel row segment: every tap it reads is 1 KB contiguous).  Each
// pass reads its own pixel's 48 B of records from HBM and the other 24 taps' through the caches.  The three edge-stopping weights are
// evaluated as ONE exponential, exp2(-(|dc|^2 kc + |dn|^2 kn + |dx|^2 kx)) with the per-pass constants (log2 e folded in) computed on
// the host in double -- the same product as the three factors of the definition.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <string>
#include <utility>
#include <vector>

#include "pt_denoise.h"

extern "C" void ptx_internal_set_error(const char *msg);

namespace {

constexpr int BX = 64, BY = 4;

__global__ __launch_bounds__(256) void k_atrous_prep(int n, const float *__restrict__ rgb, float spp, const float4 *__restrict__ nh,
                                                     const float4 *__restrict__ alb, int demod, float4 *__restrict__ c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r = rgb[3 * (size_t)i] / spp, g = rgb[3 * (size_t)i + 1] / spp, b = rgb[3 * (size_t)i + 2] / spp;
    if (demod && nh[i].w != 0.f) {
        const float4 a = alb[i];
        r = r / fmaxf(a.x, 1e-3f); g = g / fmaxf(a.y, 1e-3f); b = b / fmaxf(a.z, 1e-3f);
    }
    c[i] = make_float4(r, g, b, 0.f);
}

template <bool LAST>
__global__ __launch_bounds__(BX * BY) void k_atrous_pass(int w, int h, int step, float kc, float kn, float kx, const float4 *__restrict__ nh,
                                                         const float4 *__restrict__ xt, const float4 *__restrict__ cin, float4 *__restrict__ cout,
                                                         const float4 *__restrict__ alb, int demod, float *__restrict__ out) {
    const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int p = y * w + x;
    const float4 np = nh[p], cp = cin[p];
    float4 res = cp;                                     // miss pixels pass through
    if (np.w != 0.f) {
        const float4 xp = xt[p];
        const float b[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
        float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
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
                const float c0 = cp.x - cq.x, c1 = cp.y - cq.y, c2 = cp.z - cq.z;
                const float n0 = np.x - nq.x, n1 = np.y - nq.y, n2 = np.z - nq.z;
                const float x0 = xp.x - xq.x, x1 = xp.y - xq.y, x2 = xp.z - xq.z;
                const float dc2 = c0 * c0 + c1 * c1 + c2 * c2, dn2 = n0 * n0 + n1 * n1 + n2 * n2, dx2 = x0 * x0 + x1 * x1 + x2 * x2;
                const float wt = b[i] * b[j] * exp2f(-(dc2 * kc + dn2 * kn + dx2 * kx));
                sr += wt * cq.x; sg += wt * cq.y; sb += wt * cq.z; sw += wt;
            }
        }
        res = make_float4(sr / sw, sg / sw, sb / sw, 0.f);   // sw >= 9/64: the centre tap
    }
    if (LAST) {
        if (demod && np.w != 0.f) {
            const float4 a = alb[p];
            res.x = res.x * fmaxf(a.x, 1e-3f); res.y = res.y * fmaxf(a.y, 1e-3f); res.z = res.z * fmaxf(a.z, 1e-3f);
        }
        out[3 * (size_t)p] = res.x; out[3 * (size_t)p + 1] = res.y; out[3 * (size_t)p + 2] = res.z;
    } else {
        cout[p] = res;
    }
}

template <class T> struct DevMem {
    T *p = nullptr;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, sizeof(T) * (n ? n : 1)); }
};

int fail(int code, const std::string &msg) { ptx_internal_set_error(msg.c_str()); return code; }

}  // namespace

const char *pt_denoise_params_problem(const ptx_denoise_params &p) {
    if (p.passes < 1 || p.passes > 10) return "ptx_denoise_params.passes must be 1 .. 10";
    if (!(p.phi_color > 0.f) || !(p.phi_normal > 0.f) || !(p.phi_position > 0.f))
        return "ptx_denoise_params: phi_color, phi_normal and phi_position must be positive";
    return nullptr;
}

hipError_t pt_atrous_enqueue(hipStream_t st, int w, int h, const float *rgb, float spp, const float4 *nh, const float4 *xt,
                             const float4 *alb, float4 *tmp0, float4 *tmp1, float *out_rgb, const ptx_denoise_params &p) {
    const int n = w * h, demod = p.demodulate ? 1 : 0;
    hipLaunchKernelGGL(k_atrous_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rgb, spp, nh, alb, demod, tmp0);
    const dim3 grid((unsigned)((w + BX - 1) / BX), (unsigned)((h + BY - 1) / BY)), block(BX, BY);
    float4 *src = tmp0, *dst = tmp1;
    for (int i = 0; i < p.passes; i++) {
        const double l2e = 1.4426950408889634, s = (double)(1 << i);
        const float kc = (float)(l2e * s / p.phi_color), kn = (float)(l2e / (s * s * p.phi_normal)), kx = (float)(l2e / p.phi_position);
        if (i == p.passes - 1)
            hipLaunchKernelGGL(k_atrous_pass<true>, grid, block, 0, st, w, h, 1 << i, kc, kn, kx, nh, xt, src, dst, alb, demod, out_rgb);
        else
            hipLaunchKernelGGL(k_atrous_pass<false>, grid, block, 0, st, w, h, 1 << i, kc, kn, kx, nh, xt, src, dst, alb, demod, out_rgb);
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

size_t ptx_sizeof_denoise_params(void) { return sizeof(ptx_denoise_params); }

int ptx_denoise_buffers(int device, int w, int h, const float *rgb, const float *alb3, const float *nrm3, const float *pos3,
                        const uint8_t *hit, const ptx_denoise_params *params, float *out_rgb) {
    ptx_denoise_params p;
    if (params) p = *params;
    else ptx_default_denoise_params(&p);
    if (w < 1 || h < 1 || (long long)w * h > INT_MAX / 3) return fail(PTX_ERR_INVALID, "ptx_denoise_buffers: bad frame size");
    if (!rgb || !nrm3 || !pos3 || !hit || !out_rgb) return fail(PTX_ERR_INVALID, "ptx_denoise_buffers: rgb, nrm3, pos3, hit and out_rgb are required");
    if (p.demodulate && !alb3) return fail(PTX_ERR_INVALID, "ptx_denoise_buffers: demodulation needs alb3");
    if (const char *why = pt_denoise_params_problem(p)) return fail(PTX_ERR_INVALID, why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return fail(PTX_ERR_NODEVICE, "no HIP device available; the denoiser has no CPU path");
    }
    if (device < 0 || device >= ndev) return fail(PTX_ERR_INVALID, "ptx_denoise_buffers: device ordinal out of range");
    const size_t n = (size_t)w * h;
    std::vector<float4> hnh(n), hxt(n), hal(n);
    for (size_t i = 0; i < n; i++) {
        const bool on = hit[i] != 0;
        hnh[i] = make_float4(nrm3[3 * i], nrm3[3 * i + 1], nrm3[3 * i + 2], on ? 1.f : 0.f);
        hxt[i] = make_float4(pos3[3 * i], pos3[3 * i + 1], pos3[3 * i + 2], 0.f);
        hal[i] = alb3 ? make_float4(alb3[3 * i], alb3[3 * i + 1], alb3[3 * i + 2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#define HC(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(PTX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
    HC(hipSetDevice(device));
    DevMem<float> d_rgb, d_out;
    DevMem<float4> d_nh, d_xt, d_al, d_t0, d_t1;
    HC(d_rgb.alloc(3 * n)); HC(d_out.alloc(3 * n));
    HC(d_nh.alloc(n)); HC(d_xt.alloc(n)); HC(d_al.alloc(n)); HC(d_t0.alloc(n)); HC(d_t1.alloc(n));
    HC(hipMemcpy(d_rgb.p, rgb, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
    HC(hipMemcpy(d_nh.p, hnh.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    HC(hipMemcpy(d_xt.p, hxt.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    HC(hipMemcpy(d_al.p, hal.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    HC(pt_atrous_enqueue(nullptr, w, h, d_rgb.p, 1.0f, d_nh.p, d_xt.p, d_al.p, d_t0.p, d_t1.p, d_out.p, p));
    HC(hipStreamSynchronize(nullptr));
    HC(hipMemcpy(out_rgb, d_out.p, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
#undef HC
    return PTX_OK;
}

}  // extern "C"
