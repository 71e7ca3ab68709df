// pt_temporal.hip -- temporal reuse in front of the a-trous denoiser (in the spirit of SVGF, Schied et al., HPG 2017): the history
// handle of include/mi355x_pathtracer.h (ptx_temporal_*) and its one kernel.  ptx_denoise_temporal itself is pt_engine.hip's: it needs
// the tracer's G-buffer and accumulation buffer.
//
// k_temporal_reproject: one thread per pixel of the current G-buffer, workgroups of 64 x 4 pixels as k_atrous_pass (a wave is one
// 64-pixel row segment, so its bilinear taps into hist are two contiguous runs of records).  fp32, plain vector loads and stores.
// Per pixel: reproject into hist's camera, accept / reject up to four taps, mix with rgb / spp, write the new cur record, the mix and
// (h, n_h).  It copies what the next segment needs out of the G-buffer, which ensure_gbuffer rewrites in place on the next view.
// k_reproject_variance (ptx_denoise_variance) is the same pixel function, reproject_pixel<true>: the same arithmetic plus the per-sample luminance variance V in dd.w: inherited
// and updated where the history carries one, -1 (= "pt_denoise.hip's spatial estimate fills this in") on the other hit pixels.
// k_reproject_measured (ptx_denoise_temporal_measured) is reproject_pixel<true, true>: it also reads the pixel's share of a moments state
// (ma as one float4, its (rb, gb) of mb as one float2: 24 B more per pixel) and takes from it q, the measured per-sample variance of
// the demodulated luminance with B - 1 degrees of freedom.  Where V is inherited, q is pooled with the between-view term e (one degree
// of freedom) by degrees of freedom; the other hit pixels get q in place of -1.  A measured V is per pixel and as spiky as the samples
// (0 beside 3 where one of eight samples found the light), so V_h and mu_h are ill-conditioned in the bilinear weights where the
// spatial estimate's windowed V was not: u near 100 carries an fp32 ulp of 8e-6 of a pixel, 2 % of a weight of 5e-4.  This kernel
// therefore takes the weights of those two sums -- and of nothing else: taps, n_h, h and mix are the other kernels', bit for bit --
// from the projection redone in double (PtTemporalCamD; fp64 is full rate on CDNA).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include <string.h>
#include <string>

#include "pt_denoise.h"

namespace {

constexpr int BX = PT_BX, BY = PT_BY;

template <bool VAR, bool MEASURED = false>
__device__ __forceinline__ void reproject_pixel(
        int w, int h, const PtTemporalCam cam, float max_history, int specular_history, float normal_cos, float plane_tolerance,
        int hist_has_v,
        const float *__restrict__ rgb, float spp, const float4 *__restrict__ gnh, const float4 *__restrict__ gxt,
        const float4 *__restrict__ galb, const int2 *__restrict__ gids, const uint8_t *__restrict__ spec, int nmats,
        float4 *__restrict__ cnh, float4 *__restrict__ cxn, float4 *__restrict__ cdd, int2 *__restrict__ cids,
        const float4 *__restrict__ hnh, const float4 *__restrict__ hxn, const float4 *__restrict__ hdd, const int2 *__restrict__ hids,
        float *__restrict__ mix, float4 *__restrict__ hn,
        const float4 *__restrict__ ma = nullptr, const float2 *__restrict__ mb2 = nullptr, int pairs = 0, float batches = 0.f,
        const PtTemporalCamD camd = PtTemporalCamD()) {
    const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int p = y * w + x;
    const float4 np = gnh[p], xp = gxt[p];
    const int2 id = gids[p];
    const bool hit = np.w != 0.f;
    const float c0 = rgb[3 * (size_t)p] / spp, c1 = rgb[3 * (size_t)p + 1] / spp, c2 = rgb[3 * (size_t)p + 2] / spp;   // = k_atrous_prep
    float4 a = make_float4(1.f, 1.f, 1.f, 0.f);
    float h0 = 0.f, h1 = 0.f, h2 = 0.f, nhist = 0.f;
    float var = hit ? -1.f : 0.f;                        // VAR only: V, or -1 where the spatial estimate has to supply it
    float q = 0.f;                                       // MEASURED only: max(g^T M g / (B - 1), 0), g = the demodulated luminance's weights
    if (hit) {
        const float4 al = galb[p];
        a = make_float4(fmaxf(al.x, 1e-3f), fmaxf(al.y, 1e-3f), fmaxf(al.z, 1e-3f), 0.f);
        if (MEASURED) {                                  // = k_moments_prep's v * W when demodulating
            const float2 m2 = mb2[(size_t)y * pairs * 2 + x];
            q = fmaxf(quad_form(0.2126f / a.x, 0.7152f / a.y, 0.0722f / a.z, ma[p], m2.x, m2.y, batches), 0.f);
            var = q;                                     // nothing inherited: the measured variance alone
        }
        const bool specular = id.x >= 0 && id.x < nmats && spec[id.x] != 0;
        if (cam.valid && (specular_history || !specular)) {
            const float dx = xp.x - cam.pos[0], dy = xp.y - cam.pos[1], dz = xp.z - cam.pos[2];
            const float s = cam.minv[0] * dx + cam.minv[1] * dy + cam.minv[2] * dz;
            const float su = cam.minv[3] * dx + cam.minv[4] * dy + cam.minv[5] * dz;
            const float sv = cam.minv[6] * dx + cam.minv[7] * dy + cam.minv[8] * dz;
            const float u = su / s, v = sv / s;
            // (a NaN fails every comparison: no tap)
            if (s > 0.f && u > -1.f && u < (float)w && v > -1.f && v < (float)h) {
                const float uf = floorf(u), vf = floorf(v);
                const int u0 = (int)uf, v0 = (int)vf;
                const float fu = u - uf, fv = v - vf;
                const float lim = plane_tolerance * sqrtf(dx * dx + dy * dy + dz * dz);
                float sr = 0.f, sg = 0.f, sb = 0.f, sn = 0.f, sw = 0.f, sv = 0.f;
                float pfu = 0.f, pfv = 0.f, pr = 0.f, pg = 0.f, pb = 0.f, pw = 0.f, pv = 0.f;     // MEASURED only: the precise weights' sums
                if (MEASURED) {                          // the same taps' fractions from (u, v) in double, clamped to their cell
                    const double ex = (double)xp.x - camd.pos[0], ey = (double)xp.y - camd.pos[1], ez = (double)xp.z - camd.pos[2];
                    const double ds = camd.minv[0] * ex + camd.minv[1] * ey + camd.minv[2] * ez;
                    const double du = (camd.minv[3] * ex + camd.minv[4] * ey + camd.minv[5] * ez) / ds;
                    const double dv = (camd.minv[6] * ex + camd.minv[7] * ey + camd.minv[8] * ez) / ds;
                    pfu = (float)fmin(fmax(du - (double)uf, 0.0), 1.0);
                    pfv = (float)fmin(fmax(dv - (double)vf, 0.0), 1.0);
                }
#pragma unroll
                for (int j = 0; j < 2; j++) {
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int qx = u0 + i, qy = v0 + j;
                        const float wt = (i ? fu : 1.f - fu) * (j ? fv : 1.f - fv);
                        if (!(wt > 0.f) || qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                        const int q = qy * w + qx;
                        const float4 nq = hnh[q];
                        if (nq.w == 0.f) continue;
                        const int2 iq = hids[q];
                        if (iq.x != id.x || iq.y != id.y) continue;
                        if (!(np.x * nq.x + np.y * nq.y + np.z * nq.z >= normal_cos)) continue;
                        const float4 xq = hxn[q];
                        const float pl = np.x * (xq.x - xp.x) + np.y * (xq.y - xp.y) + np.z * (xq.z - xp.z);
                        if (!(fabsf(pl) <= lim)) continue;
                        const float4 dq = hdd[q];
                        sr += wt * dq.x; sg += wt * dq.y; sb += wt * dq.z; sn += wt * xq.w; sw += wt;
                        if (VAR) sv += wt * dq.w;
                        if (MEASURED) {
                            const float pt = (i ? pfu : 1.f - pfu) * (j ? pfv : 1.f - pfv);
                            pr += pt * dq.x; pg += pt * dq.y; pb += pt * dq.z; pv += pt * dq.w; pw += pt;
                        }
                    }
                }
                if (sw > 0.f) {
                    nhist = fminf(sn / sw, max_history);
                    if (nhist > 0.f) { h0 = sr / sw * a.x; h1 = sg / sw * a.y; h2 = sb / sw * a.z; }
                    else nhist = 0.f;
                    if (VAR && hist_has_v && nhist > 0.f) {
                        // the pairwise update of a per-sample variance: between-batch term e, then the mean by sample counts
                        const bool precise = MEASURED && pw > 0.f;          // (pw == 0: every accepted tap sits on a clamped edge)
                        const float mu = precise ? pt_luminance(pr / pw, pg / pw, pb / pw) : pt_luminance(sr / sw, sg / sw, sb / sw);
                        const float lc = pt_luminance(c0 / a.x, c1 / a.y, c2 / a.z);
                        const float d = lc - mu, tot = nhist + spp, e = d * d * nhist * spp / tot;
                        if (MEASURED) var = (nhist * (precise ? pv / pw : sv / sw) + spp * (((batches - 1.f) * q + e) / batches)) / tot;
                        else var = (nhist * (sv / sw) + spp * e) / tot;
                    }
                }
            }
        }
    }
    float m0 = c0, m1 = c1, m2 = c2, n = spp;            // a miss, or nothing inherited: mix is c exactly
    if (nhist > 0.f) {
        const float tot = spp + nhist;
        m0 = (spp * c0 + nhist * h0) / tot; m1 = (spp * c1 + nhist * h1) / tot; m2 = (spp * c2 + nhist * h2) / tot;
        n = tot;
    }
    cnh[p] = np;
    cxn[p] = make_float4(xp.x, xp.y, xp.z, n);
    cdd[p] = hit ? make_float4(m0 / a.x, m1 / a.y, m2 / a.z, VAR ? var : 0.f) : make_float4(m0, m1, m2, 0.f);
    cids[p] = id;
    mix[3 * (size_t)p] = m0; mix[3 * (size_t)p + 1] = m1; mix[3 * (size_t)p + 2] = m2;
    hn[p] = make_float4(h0, h1, h2, nhist);
}

#define REPROJECT_PARAMS \
        int w, int h, const PtTemporalCam cam, float max_history, int specular_history, float normal_cos, float plane_tolerance, \
        int hist_has_v, const float *__restrict__ rgb, float spp, const float4 *__restrict__ gnh, const float4 *__restrict__ gxt, \
        const float4 *__restrict__ galb, const int2 *__restrict__ gids, const uint8_t *__restrict__ spec, int nmats, \
        float4 *__restrict__ cnh, float4 *__restrict__ cxn, float4 *__restrict__ cdd, int2 *__restrict__ cids, \
        const float4 *__restrict__ hnh, const float4 *__restrict__ hxn, const float4 *__restrict__ hdd, const int2 *__restrict__ hids, \
        float *__restrict__ mix, float4 *__restrict__ hn
#define REPROJECT_ARGS \
        w, h, cam, max_history, specular_history, normal_cos, plane_tolerance, hist_has_v, rgb, spp, gnh, gxt, galb, gids, spec, nmats, cnh, \
        cxn, cdd, cids, hnh, hxn, hdd, hids, mix, hn

__global__ __launch_bounds__(BX * BY) void k_temporal_reproject(REPROJECT_PARAMS) { reproject_pixel<false>(REPROJECT_ARGS); }
// ptx_denoise_variance's: the same pixel function with V
__global__ __launch_bounds__(BX * BY) void k_reproject_variance(REPROJECT_PARAMS) { reproject_pixel<true>(REPROJECT_ARGS); }
// ptx_denoise_temporal_measured's: V from the moments state too (batches = B >= 2, one number per handle)
__global__ __launch_bounds__(BX * BY) void k_reproject_measured(REPROJECT_PARAMS, const float4 *__restrict__ ma,
                                                                const float2 *__restrict__ mb2, int pairs, float batches,
                                                                const PtTemporalCamD camd) {
    reproject_pixel<true, true>(REPROJECT_ARGS, ma, mb2, pairs, batches, camd);
}

}  // namespace

const char *pt_temporal_params_problem(const ptx_temporal_params &p) {
    if (p.max_history < 0) return "ptx_temporal_params.max_history must be >= 0";
    if (!(p.normal_cos >= -1.f && p.normal_cos <= 1.f)) return "ptx_temporal_params.normal_cos must be in -1 .. 1";
    if (!(p.plane_tolerance >= 0.f) || isinf(p.plane_tolerance)) return "ptx_temporal_params.plane_tolerance must be finite and >= 0";
    return nullptr;
}

PtTemporalCam pt_temporal_camera(const ptx_camera &c, bool have_hist, PtTemporalCamD *precise) {
    PtTemporalCam k;
    memset(&k, 0, sizeof k);
    const double W = c.resolution[0], H = c.resolution[1];
    double R[3], U[3], A[3];
    for (int i = 0; i < 3; i++) {
        R[i] = (double)c.right[i] * c.pixelLength[0];
        U[i] = (double)c.up[i] * c.pixelLength[1];
        A[i] = (double)c.view[i] + R[i] * (W * 0.5) + U[i] * (H * 0.5);
    }
    const double m[3][3] = {{A[0], -R[0], -U[0]}, {A[1], -R[1], -U[1]}, {A[2], -R[2], -U[2]}};
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    double inv[9];
    inv[0] = (m[1][1] * m[2][2] - m[1][2] * m[2][1]) / det;
    inv[1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det;
    inv[2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
    inv[3] = (m[1][2] * m[2][0] - m[1][0] * m[2][2]) / det;
    inv[4] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det;
    inv[5] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
    inv[6] = (m[1][0] * m[2][1] - m[1][1] * m[2][0]) / det;
    inv[7] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
    inv[8] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
    bool ok = have_hist && det != 0.0 && std::isfinite(det);
    for (int i = 0; i < 9; i++) {
        k.minv[i] = (float)inv[i];
        ok = ok && std::isfinite(k.minv[i]);
    }
    for (int i = 0; i < 3; i++) k.pos[i] = c.position[i];
    if (precise) {
        for (int i = 0; i < 9; i++) precise->minv[i] = inv[i];
        for (int i = 0; i < 3; i++) precise->pos[i] = c.position[i];
    }
    k.valid = ok ? 1 : 0;
    return k;
}

hipError_t pt_temporal_enqueue(hipStream_t st, int w, int h, const PtTemporalCam &cam, const ptx_temporal_params &p, const float *rgb,
                               float spp, const float4 *gnh, const float4 *gxt, const float4 *galb, const int2 *gids,
                               const uint8_t *spec, int nmats, const PtTemporalState &cur, const PtTemporalState &hist, float *mix,
                               float4 *hn, int variance, int hist_has_v, const PtMomentsState *moments, int batches,
                               const PtTemporalCamD *camd) {
    if (variance && moments && camd && batches >= 2) {
        hipLaunchKernelGGL(k_reproject_measured, pt_pixel_grid(w, h), dim3(BX, BY), 0, st, w, h, cam, (float)p.max_history,
                           p.specular_history ? 1 : 0, p.normal_cos, p.plane_tolerance, hist_has_v, rgb, spp, gnh, gxt, galb, gids, spec,
                           nmats, cur.nh, cur.xn, cur.dd, cur.ids, (const float4 *)hist.nh, (const float4 *)hist.xn, (const float4 *)hist.dd,
                           (const int2 *)hist.ids, mix, hn, (const float4 *)moments->ma, reinterpret_cast<const float2 *>(moments->mb),
                           pt_moments_pairs(w), (float)batches, *camd);
        return hipGetLastError();
    }
    const auto kernel = variance ? k_reproject_variance : k_temporal_reproject;
    hipLaunchKernelGGL(kernel, pt_pixel_grid(w, h), dim3(BX, BY), 0, st, w, h, cam, (float)p.max_history, p.specular_history ? 1 : 0,
                       p.normal_cos, p.plane_tolerance, hist_has_v, rgb, spp, gnh, gxt, galb, gids, spec, nmats, cur.nh, cur.xn, cur.dd,
                       cur.ids, (const float4 *)hist.nh, (const float4 *)hist.xn, (const float4 *)hist.dd, (const int2 *)hist.ids, mix, hn);
    return hipGetLastError();
}

extern "C" {

void ptx_default_temporal_params(ptx_temporal_params *p) {
    if (!p) return;
    p->max_history = 16;           // the sweep of tools/gpu_temporal_quality.py
    p->specular_history = 0;
    p->normal_cos = 0.9f;
    p->plane_tolerance = 0.01f;
}

size_t ptx_sizeof_temporal_params(void) { return sizeof(ptx_temporal_params); }

static int alloc_temporal(ptx_temporal *t) {
    const size_t n = (size_t)t->w * t->h;
    PT_HC(hipSetDevice(t->device));
    for (int i = 0; i < 2; i++) {
        PT_HC(t->d_nh[i].alloc(n)); PT_HC(t->d_xn[i].alloc(n));
        PT_HC(t->d_dd[i].alloc(n)); PT_HC(t->d_ids[i].alloc(n));
        t->st[i].nh = t->d_nh[i]; t->st[i].xn = t->d_xn[i]; t->st[i].dd = t->d_dd[i]; t->st[i].ids = t->d_ids[i];
    }
    PT_HC(t->d_mix.alloc(3 * n));
    PT_HC(t->d_hn.alloc(n));
    PT_HC(t->ev.create(hipEventDisableTiming));
    return PTX_OK;
}

int ptx_temporal_create(int device, int width, int height, ptx_temporal **out) {
    return pt_handle_create("ptx_temporal_create", "the temporal denoiser", device, width, height, INT_MAX / 3, out, alloc_temporal);
}

void ptx_temporal_destroy(ptx_temporal *t) { pt_handle_destroy(t); }

int ptx_temporal_reset(ptx_temporal *t) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null temporal handle");
    t->cur_valid = t->hist_valid = false;    // (the buffers are only read behind these flags; the next call waits for the last)
    return PTX_OK;
}

int ptx_temporal_read(ptx_temporal *t, float *hist_rgb3, float *hist_count1, float *mix_rgb3) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null temporal handle");
    if (!t->done) return pt_fail(PTX_ERR_INVALID, "ptx_temporal_read: no ptx_denoise_temporal with this handle yet");
    const size_t n = (size_t)t->w * t->h;
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipEventSynchronize(t->ev));
    if (mix_rgb3) PT_HC(hipMemcpy(mix_rgb3, t->d_mix, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
    if (hist_rgb3 || hist_count1) {
        std::vector<float4> hn(n);
        PT_HC(hipMemcpy(hn.data(), t->d_hn, sizeof(float4) * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) {
            if (hist_rgb3) { hist_rgb3[3 * i] = hn[i].x; hist_rgb3[3 * i + 1] = hn[i].y; hist_rgb3[3 * i + 2] = hn[i].z; }
            if (hist_count1) hist_count1[i] = hn[i].w;
        }
    }
    return PTX_OK;
}

// The reprojection alone over caller-owned host arrays (tests/test_gpu_temporal_grid.py): arguments checked, float3 -> float4 staging
// into the layouts of pt_denoise.h, then pt_temporal_camera and pt_temporal_enqueue -- what temporal_step (pt_post.hip) calls -- on the
// null stream, and the raw records back.  No kernel is launched here.
int ptx_kat_reproject(int device, int w, int h, int variant, const ptx_camera *hist_cam, const ptx_temporal_params *params, int spp,
                      const float *rgb, const float *nrm3, const float *pos3, const float *alb3, const int32_t *ids2, const uint8_t *hit,
                      const uint8_t *spec, int nmats, const uint8_t *hist_hit, const float *hist_nrm3, const float *hist_pos3,
                      const float *hist_n1, const float *hist_D3, const float *hist_V1, const int32_t *hist_ids2, const float *scatter6,
                      int batches, float *out_nh4, float *out_xn4, float *out_dd4, int32_t *out_ids2, float *out_mix3, float *out_hn4) {
    const std::string name = "ptx_kat_reproject";
    ptx_temporal_params tp;
    if (params) tp = *params;
    else ptx_default_temporal_params(&tp);
    if (w < 1 || h < 1 || (long long)w * h > INT_MAX / 4)
        return pt_fail(PTX_ERR_INVALID, name + ": bad frame size " + std::to_string(w) + " x " + std::to_string(h));
    if (variant < 0 || variant > 2) return pt_fail(PTX_ERR_INVALID, name + ": variant must be 0, 1 or 2, not " + std::to_string(variant));
    if (spp < 1) return pt_fail(PTX_ERR_INVALID, name + ": spp must be >= 1, not " + std::to_string(spp));
    if (nmats < 0) return pt_fail(PTX_ERR_INVALID, name + ": nmats must be >= 0, not " + std::to_string(nmats));
    if (!rgb || !nrm3 || !pos3 || !alb3 || !ids2 || !hit) return pt_fail(PTX_ERR_INVALID, name + ": rgb, nrm3, pos3, alb3, ids2 and hit are required");
    if (nmats > 0 && !spec) return pt_fail(PTX_ERR_INVALID, name + ": spec is required for nmats = " + std::to_string(nmats));
    if (hist_cam && (!hist_hit || !hist_nrm3 || !hist_pos3 || !hist_n1 || !hist_D3 || !hist_ids2))
        return pt_fail(PTX_ERR_INVALID, name + ": a hist camera needs hist_hit, hist_nrm3, hist_pos3, hist_n1, hist_D3 and hist_ids2");
    if (hist_cam && (hist_cam->resolution[0] != w || hist_cam->resolution[1] != h))
        return pt_fail(PTX_ERR_INVALID, name + ": the hist camera's resolution is " + std::to_string(hist_cam->resolution[0]) + " x " +
                                            std::to_string(hist_cam->resolution[1]) + ", the frame " + std::to_string(w) + " x " + std::to_string(h));
    if (variant == 2 && !scatter6) return pt_fail(PTX_ERR_INVALID, name + ": variant 2 needs scatter6");
    if (variant == 2 && batches < 2) return pt_fail(PTX_ERR_INVALID, name + ": variant 2 needs batches >= 2, not " + std::to_string(batches));
    if (const char *why = pt_temporal_params_problem(tp)) return pt_fail(PTX_ERR_INVALID, why);
    if (device < 0) return pt_fail(PTX_ERR_INVALID, name + ": device ordinal out of range: " + std::to_string(device));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return pt_fail(PTX_ERR_NODEVICE, "no HIP device available; the temporal denoiser has no CPU path");
    }
    if (device >= ndev) return pt_fail(PTX_ERR_INVALID, name + ": device ordinal out of range: " + std::to_string(device));

    const size_t n = (size_t)w * h;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    std::vector<float4> gnh(n), gxt(n), gal(n), hnh(n, zero), hxn(n, zero), hdd(n, zero);
    std::vector<int2> gid(n), hid(n, make_int2(0, 0));
    for (size_t i = 0; i < n; i++) {
        gnh[i] = make_float4(nrm3[3 * i], nrm3[3 * i + 1], nrm3[3 * i + 2], hit[i] ? 1.f : 0.f);
        gxt[i] = make_float4(pos3[3 * i], pos3[3 * i + 1], pos3[3 * i + 2], 0.f);
        gal[i] = make_float4(alb3[3 * i], alb3[3 * i + 1], alb3[3 * i + 2], 0.f);
        gid[i] = make_int2(ids2[2 * i], ids2[2 * i + 1]);
        if (!hist_cam) continue;
        hnh[i] = make_float4(hist_nrm3[3 * i], hist_nrm3[3 * i + 1], hist_nrm3[3 * i + 2], hist_hit[i] ? 1.f : 0.f);
        hxn[i] = make_float4(hist_pos3[3 * i], hist_pos3[3 * i + 1], hist_pos3[3 * i + 2], hist_n1[i]);
        hdd[i] = make_float4(hist_D3[3 * i], hist_D3[3 * i + 1], hist_D3[3 * i + 2], hist_V1 ? hist_V1[i] : 0.f);
        hid[i] = make_int2(hist_ids2[2 * i], hist_ids2[2 * i + 1]);
    }
    const int pairs = pt_moments_pairs(w);
    std::vector<float4> hma, hmb;
    if (variant == 2) {                                  // pt_denoise.h: ma = (rr, gg, bb, rg), mb = (rb, gb) of a row's pixel pairs
        hma.resize(n);
        hmb.assign((size_t)h * pairs, zero);             // (the second half of an odd row's last record stays 0)
        float2 *mb2 = reinterpret_cast<float2 *>(hmb.data());
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const float *m = scatter6 + 6 * ((size_t)y * w + x);
                hma[(size_t)y * w + x] = make_float4(m[0], m[1], m[2], m[3]);
                mb2[(size_t)y * pairs * 2 + x] = make_float2(m[4], m[5]);
            }
    }
    ptx_camera cam;
    memset(&cam, 0, sizeof cam);
    if (hist_cam) cam = *hist_cam;
    PtTemporalCamD camd;
    const PtTemporalCam hcam = pt_temporal_camera(cam, hist_cam != nullptr, &camd);

    PT_HC(hipSetDevice(device));
    DevBuf<float> d_rgb, d_mix;
    DevBuf<float4> d_gnh, d_gxt, d_gal, d_hnh, d_hxn, d_hdd, d_cnh, d_cxn, d_cdd, d_hn, d_ma, d_mb;
    DevBuf<int2> d_gid, d_hid, d_cid;
    DevBuf<uint8_t> d_spec;
    PT_HC(d_rgb.upload(rgb, 3 * n));
    PT_HC(d_gnh.upload(gnh)); PT_HC(d_gxt.upload(gxt)); PT_HC(d_gal.upload(gal)); PT_HC(d_gid.upload(gid));
    PT_HC(d_hnh.upload(hnh)); PT_HC(d_hxn.upload(hxn)); PT_HC(d_hdd.upload(hdd)); PT_HC(d_hid.upload(hid));
    if (nmats > 0) PT_HC(d_spec.upload(spec, (size_t)nmats));
    PT_HC(d_cnh.alloc(n)); PT_HC(d_cxn.alloc(n)); PT_HC(d_cdd.alloc(n)); PT_HC(d_cid.alloc(n));
    PT_HC(d_mix.alloc(3 * n)); PT_HC(d_hn.alloc(n));
    PtTemporalState cur, hist;
    cur.nh = d_cnh; cur.xn = d_cxn; cur.dd = d_cdd; cur.ids = d_cid;
    hist.nh = d_hnh; hist.xn = d_hxn; hist.dd = d_hdd; hist.ids = d_hid;
    PtMomentsState ms;
    if (variant == 2) {
        PT_HC(d_ma.upload(hma)); PT_HC(d_mb.upload(hmb));
        ms.ma = d_ma; ms.mb = d_mb;
    }
    PT_HC(pt_temporal_enqueue(nullptr, w, h, hcam, tp, d_rgb, (float)spp, d_gnh, d_gxt, d_gal, d_gid, d_spec, nmats, cur, hist, d_mix, d_hn,
                              variant >= 1 ? 1 : 0, variant >= 1 && hist_cam && hist_V1 ? 1 : 0, variant == 2 ? &ms : nullptr,
                              variant == 2 ? batches : 0, &camd));
    PT_HC(hipStreamSynchronize(nullptr));
    if (out_nh4) PT_HC(d_cnh.download(out_nh4));
    if (out_xn4) PT_HC(d_cxn.download(out_xn4));
    if (out_dd4) PT_HC(d_cdd.download(out_dd4));
    if (out_ids2) PT_HC(d_cid.download(out_ids2));
    if (out_mix3) PT_HC(d_mix.download(out_mix3));
    if (out_hn4) PT_HC(d_hn.download(out_hn4));
    return PTX_OK;
}

}  // extern "C"
