// pt_temporal.h -- internal interface between the tracer (pt_engine.hip: ptx_denoise_temporal) and the temporal reprojection
// (pt_temporal.hip).  Not part of the C ABI; include/mi355x_pathtracer.h has the public side and the definition.
//
// A state (the handle keeps two, `cur` and `hist`, and swaps their pointers on a camera change), one record per pixel,
// pixelIndex = x + y*W:
//   nh[i]  = float4(normal xyz, hit ? 1 : 0)          (copied from the tracer's G-buffer)
//   xn[i]  = float4(world position xyz, sample count n)
//   dd[i]  = float4(D rgb, V)                          (D = mix / max(albedo, 1e-3) on hit pixels, mix on miss pixels; V = the per-sample
//                                                        luminance variance when ptx_denoise_variance wrote the state, else 0)
//   ids[i] = int2(material id, geom id)
// 56 B per pixel: a bilinear tap reads one whole record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355x_pathtracer.h"

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

struct ptx_temporal {
    int device = 0, w = 0, h = 0;
    PtTemporalState st[2];
    int cur = 0;                          // st[cur] is cur, st[cur ^ 1] is hist
    ptx_camera cam[2];                    // the camera of each state
    bool cur_valid = false, hist_valid = false;
    bool has_v[2] = {false, false};       // st[i].dd.w holds a V (written by ptx_denoise_variance, not by ptx_denoise_temporal)
    float *d_mix = nullptr;               // W*H*3: the last call's mix (the filter's input)
    float4 *d_hn = nullptr;               // W*H: the last call's (h rgb, n_h)
    hipEvent_t ev = nullptr;              // recorded after each call's work (on that call's stream)
    bool used = false, done = false;      // ev was recorded / d_mix, d_hn hold a result
};

// NULL when the parameters are usable, else what is wrong with them (the ptx_last_error message)
const char *pt_temporal_params_problem(const ptx_temporal_params &p);

// hist's camera -> PtTemporalCam (in double, then rounded); valid = 0 when the system is singular or not finite
PtTemporalCam pt_temporal_camera(const ptx_camera &c, bool have_hist);

// Enqueues the reprojection + mix on `st`: reads the tracer's G-buffer (gnh, gxt, galb, gids; pt_denoise.h layout) and accumulation
// rgb / spp, writes st_cur, mix (W*H*3) and hn (W*H).  spec: one byte per material (!= 0: reflective or refractive).
// variance != 0: cur.dd.w = V where hist supplies one (hist_has_v != 0 and n_h > 0), -1 on the other hit pixels (pt_variance.h:
// pt_variance_spatial_enqueue fills those in); variance == 0: dd.w = 0.
hipError_t pt_temporal_enqueue(hipStream_t st, int w, int h, const PtTemporalCam &cam, const ptx_temporal_params &p, const float *rgb,
                               float spp, const float4 *gnh, const float4 *gxt, const float4 *galb, const int2 *gids,
                               const uint8_t *spec, int nmats, const PtTemporalState &cur, const PtTemporalState &hist, float *mix,
                               float4 *hn, int variance = 0, int hist_has_v = 0);

// Rec. 709 luminance, the one every variance of the denoiser is a variance of
__host__ __device__ inline float pt_luminance(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
