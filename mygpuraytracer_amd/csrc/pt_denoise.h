// pt_denoise.h -- internal interface between the tracer (pt_engine.hip: the G-buffer pass; pt_post.hip: the six ptx_denoise* entry
// points and ptx_moments_add), the a-trous filter with its variance guidance (pt_denoise.hip), the temporal reprojection
// (pt_temporal.hip) and the batch-means moments (pt_moments.hip).
// Not part of the C ABI; include/mi355x_pathtracer.h has the public side and the definitions.
//
// Device layout of the guide images, one record per pixel, pixelIndex = x + y*W (the frame's own order):
//   nh[i]  = float4(shading normal xyz, hit ? 1 : 0)
//   xt[i]  = float4(world position xyz, t)              (t is not read by the filter; ptx_read_gbuffer hands it out)
//   alb[i] = float4(albedo rgb, 0)                       (sampled guides: the fourth float is the coverage H / K; nothing reads it but
//                                                         ptx_read_guide_coverage)
// Misses are all zeros.  The filter's colour ping-pong buffers are float4(rgb, v) per pixel: v is 0 in the plain filter and the variance
// of the pixel's luminance (v0 = V / n going in) in the variance-guided one.  Before that one runs, -1 in that float (a hit pixel's)
// means "no estimate yet": pt_variance_spatial_enqueue replaces it.
//
// A temporal state (the handle keeps two, `cur` and `hist`, and swaps their pointers on a camera change), one record per pixel:
//   nh[i]  = float4(normal xyz, hit ? 1 : 0)          (copied from the tracer's G-buffer)
//   xn[i]  = float4(world position xyz, sample count n)
//   dd[i]  = float4(D rgb, V)                          (D = mix / max(albedo, 1e-3) on hit pixels, mix on miss pixels; V = the per-sample
//                                                        luminance variance when ptx_denoise_variance or
//                                                        ptx_denoise_temporal_measured wrote the state, else 0)
//   ids[i] = int2(material id, geom id)
// 56 B per pixel: a bilinear tap reads one whole record.
//
// A moments state (ptx_moments, pt_moments.hip), 56 B per pixel:
//   snap[i] = float4(accumulation rgb at the last add, W = the samples it held)
//   mean[i] = float4(weighted mean rgb of the batch means, batch count B)
//   ma[i]   = float4(M rr, gg, bb, rg)                  (the weighted scatter matrix's upper triangle)
//   mb      = float4(M rb, gb of pixel (2j, y), M rb, gb of pixel (2j + 1, y)) at [y * pt_moments_pairs(W) + j]: the two floats that
//             are left share a 16-byte record with the row neighbour's, so that k_moments_add moves whole float4 only (lanes 2j and
//             2j + 1 of a wave are always that pair: a workgroup's x0 is a multiple of 64).  An odd W pads each row by 8 B.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/mi355x_pathtracer.h"
#include "pt_handle.h"

struct PtTemporalState {
    float4 *nh = nullptr, *xn = nullptr, *dd = nullptr;
    int2 *ids = nullptr;
};

// hist's camera as the kernel takes it: the inverse of M = [A | -R | -U] (row major), A = view + R*W/2 + U*H/2, R = right*pl.x,
// U = up*pl.y, so that (s, s*u, s*v) = minv * (x - position).  valid == 0: no history (first call, after a reset, singular camera).
struct PtTemporalCam {
    float pos[3];
    float minv[9];
    int32_t valid;
};

// The same inverse and position in double, for k_reproject_measured's weights of V_h and mu_h alone (pt_temporal.hip)
struct PtTemporalCamD {
    double pos[3] = {0.0, 0.0, 0.0};
    double minv[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
};

struct ptx_temporal : PtHandle {
    DevBuf<float4> d_nh[2], d_xn[2], d_dd[2];
    DevBuf<int2> d_ids[2];
    PtTemporalState st[2];                // views of the four above, filled once, at create: what the kernels take
    int cur = 0;                          // st[cur] is cur, st[cur ^ 1] is hist
    ptx_camera cam[2];                    // the camera of each state
    bool cur_valid = false, hist_valid = false;
    bool has_v[2] = {false, false};       // st[i].dd.w holds a V (not after ptx_denoise_temporal, which writes 0 there)
    DevBuf<float> d_mix;                  // W*H*3: the last call's mix (the filter's input)
    DevBuf<float4> d_hn;                  // W*H: the last call's (h rgb, n_h)
    bool done = false;                    // d_mix, d_hn hold a result
};

struct PtMomentsState {
    float4 *snap = nullptr, *mean = nullptr, *ma = nullptr, *mb = nullptr;
};
inline int pt_moments_pairs(int w) { return (w + 1) / 2; }

// one workgroup's (stage one) or the frame's (stage two) share of ptx_moments_summarize
struct PtMomentsPartial {
    double sum_rel, sum_rel2, max_rel, sum_q;
    unsigned long long n, over;
};

struct ptx_moments : PtHandle {
    DevBuf<float4> d_snap, d_mean, d_ma, d_mb;
    PtMomentsState st;                    // a view of the four above, filled once, at create: what the kernels take
    DevBuf<float> d_stage;                // W*H*3: ptx_moments_add_host's upload (first use)
    DevBuf<PtMomentsPartial> d_part;      // one per workgroup of the pixel grid, then the total
    long long samples = 0;                // W: samples_total of the last add; 0 = fresh (the buffers are read as zeros)
    int batches = 0;                      // B
    // adds in which the tiles of ptx_tile_pixels() pixels advance by different amounts (k_moments_add_tiled).  `tiled` from the first of
    // them until ptx_moments_reset: samples and batches are then the maxima over the tiles, whose own are kept here
    bool tiled = false;
    std::vector<long long> tile_samples;
    std::vector<int> tile_batches;
    DevBuf<float2> d_tile_kt;             // ptx_moments_add_host_tiled's table (first use): (k, W') per tile
};
inline int pt_moments_tiles(int w, int h) { return (int)(((long long)w * h + ptx_tile_pixels() - 1) / ptx_tile_pixels()); }

// Rec. 709 luminance, the one every variance of the denoiser is a variance of
__host__ __device__ inline float pt_luminance(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

// g^T M g / (B - 1) for the weights g of a linear functional of the colour, M a moments state's scatter matrix (ma, and rb, gb of mb):
// the one definition pt_moments.hip's summary and prep and pt_temporal.hip's k_reproject_measured evaluate
__device__ __forceinline__ float quad_form(float g0, float g1, float g2, const float4 A, float rb, float gb, float B) {
    const float diag = g0 * g0 * A.x + g1 * g1 * A.y + g2 * g2 * A.z;
    const float off = g0 * g1 * A.w + g0 * g2 * rb + g1 * g2 * gb;
    return (diag + 2.f * off) / (B - 1.f);
}

// What pt_denoise.hip and pt_temporal.hip share: the pixel kernels' workgroup of 64 x 4 pixels (a wave is one 64-pixel row segment)
// and its grid (pt_fail and PT_HC, which every unit but pt_engine.hip reports through, are pt_handle.h's).
constexpr int PT_BX = 64, PT_BY = 4;
inline dim3 pt_pixel_grid(int w, int h) { return dim3((unsigned)((w + PT_BX - 1) / PT_BX), (unsigned)((h + PT_BY - 1) / PT_BY)); }

// NULL when the parameters are usable, else what is wrong with them (the ptx_last_error message)
const char *pt_denoise_params_problem(const ptx_denoise_params &p);
const char *pt_temporal_params_problem(const ptx_temporal_params &p);
const char *pt_variance_params_problem(const ptx_variance_params &p);

// c = float4(rgb / spp (/ max(albedo, 1e-3) on hit pixels when demodulating), v), rgb: W*H*3 floats, e.g. the accumulation buffer.
// variance == 0: v = 0.  Else v = max(var1, 0) on hit pixels when var1 is given, -1 on hit pixels when it is NULL; 0 on miss pixels.
hipError_t pt_atrous_prep_enqueue(hipStream_t st, int n, const float *rgb, float spp, const float4 *nh, const float4 *alb, int demod,
                                  int variance, const float *var1, float4 *c);
// The same from a temporal state whose dd.w holds V everywhere: c = float4(D, hit ? V / n : 0).
hipError_t pt_variance_prep_state_enqueue(hipStream_t st, int n, const PtTemporalState &s, float4 *c);
// The spatial estimate for every hit pixel whose cv[p].w is negative: cv[p].w = count * var_s(l(cv.rgb)), count = xn[p].w when
// count_from_xn, else 1.  nh / xn: normal + hit flag and position (+ count) per pixel; ids may be NULL (no id test).
hipError_t pt_variance_spatial_enqueue(hipStream_t st, int w, int h, const ptx_denoise_params &dp, const ptx_variance_params &vp,
                                       const float4 *nh, const float4 *xn, const int2 *ids, int count_from_xn, float4 *cv);
// dp.passes a-trous passes from tmp0 (filled by one of the preps), ping-ponging with tmp1 (W*H float4 each); result W*H*3 floats of mean
// radiance in out_rgb, multiplied back by max(albedo, 1e-3) when demodulating.  vp == NULL: the plain filter (colour weight
// |dc|^2 / phi_color).  Else the variance-guided one: var_in (may be NULL) receives v0, var_out (may be NULL) the last pass's v, W*H
// floats each.  Launch errors come back as the hipError_t of the first launch that failed.
hipError_t pt_atrous_enqueue(hipStream_t st, int w, int h, const float4 *nh, const float4 *xt, const float4 *alb, float4 *tmp0,
                             float4 *tmp1, float *out_rgb, const ptx_denoise_params &dp, const ptx_variance_params *vp = nullptr,
                             float *var_in = nullptr, float *var_out = nullptr);

// The sampled guides (pt_guides.hip; ptx_set_guide_samples): the guide images above averaged over the camera rays of iterations
// iter_first .. iter_first + count - 1 (count >= 1) with the tracer's antialiasing / depth-of-field options and trace depth, into the
// same four arrays; alb[i].w receives the coverage H / count.  sc / cam: the tracer's scene and camera (pt_device.h).
namespace ptd { struct DScene; struct DCamera; }
hipError_t pt_guides_enqueue(hipStream_t st, const ptd::DScene &sc, const ptd::DCamera &cam, int traceDepth, int aa, int dof, int iter_first,
                             int count, float4 *nh, float4 *xt, float4 *alb, int2 *ids);
// The same guides followed through mirrors and glass (pt_guides_follow.hip; ptx_set_guide_bounces): every one of the `count` rays is
// continued through at most `bounces` perfectly specular hits and the last surface hit is recorded, its albedo times the chain's
// throughput.  aa = dof = 0, count = 1: the pixel-centre ray.  bounces: already min(B, traceDepth - 1), >= 0.
hipError_t pt_guides_follow_enqueue(hipStream_t st, const ptd::DScene &sc, const ptd::DCamera &cam, int traceDepth, int aa, int dof,
                                    int iter_first, int count, int bounces, float4 *nh, float4 *xt, float4 *alb, int2 *ids);

const char *pt_moments_params_problem(const ptx_moments_params &p);
// One add on `st`: rgb = the accumulation buffer (W*H*3) holding `total` samples, k = total - the last add's; fresh: the state reads
// as zeros (first add after create / reset).
hipError_t pt_moments_add_enqueue(hipStream_t st, int w, int h, const float *rgb, float k, float total, int fresh, const PtMomentsState &s);
// The add in which every tile advances by its own amount, on `st`: d_kt[tile] = (k, W') on the device, host_k[tile] = the same k for
// the handle's own counts (0: the tile is idle and its pixels keep their state bit for bit; on a fresh handle they are written as
// zeros).  tile = (y * W + x) / ptx_tile_pixels().  Waits for nothing and records nothing: the caller orders it, as with
// pt_moments_add_enqueue.  An add in which no tile advances enqueues nothing.
int pt_moments_add_tiled(ptx_moments *m, hipStream_t st, const float *rgb, const float2 *d_kt, const int32_t *host_k);
// pt_atrous_prep_enqueue with the measured variance: c = float4(rgb / spp (demodulated on hit pixels), v), v = max(g^T C g, 0) / W on
// hit pixels with B >= min_batches (>= 2), -1 on the other hit pixels (pt_variance_spatial_enqueue fills those in), 0 on miss pixels.
hipError_t pt_moments_prep_enqueue(hipStream_t st, int w, int h, const float *rgb, float spp, const float4 *nh, const float4 *alb, int demod,
                                   const PtMomentsState &s, int min_batches, float4 *c);

// hist's camera -> PtTemporalCam (in double, then rounded); valid = 0 when the system is singular or not finite
// (precise: the unrounded inverse too)
PtTemporalCam pt_temporal_camera(const ptx_camera &c, bool have_hist, PtTemporalCamD *precise = nullptr);

// Enqueues the reprojection + mix on `st`: reads the tracer's G-buffer (gnh, gxt, galb, gids) and accumulation rgb / spp, writes
// st_cur, mix (W*H*3) and hn (W*H).  spec: one byte per material (!= 0: reflective or refractive).
// variance != 0: cur.dd.w = V where hist supplies one (hist_has_v != 0 and n_h > 0), -1 on the other hit pixels
// (pt_variance_spatial_enqueue fills those in); variance == 0: dd.w = 0.
// moments != NULL (with variance != 0; batches = its B >= 2): ptx_denoise_temporal_measured's V.  q = max(g^T M g / (B - 1), 0) with
// g_k = l_k / max(albedo_k, 1e-3); where hist supplies a V the current view's share is ((B - 1) q + e) / B in place of e, and the
// other hit pixels get q, so nothing is left for the spatial estimate; camd: hist's camera from pt_temporal_camera's `precise`.
// NULL / 0: the kernels above, as they were.
hipError_t pt_temporal_enqueue(hipStream_t st, int w, int h, const PtTemporalCam &cam, const ptx_temporal_params &p, const float *rgb,
                               float spp, const float4 *gnh, const float4 *gxt, const float4 *galb, const int2 *gids,
                               const uint8_t *spec, int nmats, const PtTemporalState &cur, const PtTemporalState &hist, float *mix,
                               float4 *hn, int variance = 0, int hist_has_v = 0, const PtMomentsState *moments = nullptr, int batches = 0,
                               const PtTemporalCamD *camd = nullptr);
