// pt_variance.h -- internal interface between the tracer (pt_engine.hip: ptx_denoise_variance) and the variance-guided a-trous filter
// (pt_variance.hip).  Not part of the C ABI; include/mi355x_pathtracer.h has the public side and the definition.
//
// The colour ping-pong buffers are float4(rgb, v): v is the variance of the pixel's luminance (v0 = V / n going in).  Before the filter
// runs, -1 in that float (a hit pixel's) means "no estimate yet": pt_variance_spatial_enqueue replaces it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_temporal.h"

// NULL when the parameters are usable, else what is wrong with them (the ptx_last_error message)
const char *pt_variance_params_problem(const ptx_variance_params &p);

// c = float4(rgb / spp (/ max(albedo, 1e-3) on hit pixels when demodulating), v): v = max(var1, 0) on hit pixels when var1 is given, else -1
// on hit pixels; 0 on miss pixels.
hipError_t pt_variance_prep_enqueue(hipStream_t st, int n, const float *rgb, float spp, const float4 *nh, const float4 *alb, int demod,
                                    const float *var1, float4 *c);
// The same from a temporal state whose dd.w holds V everywhere: c = float4(D, hit ? V / n : 0).
hipError_t pt_variance_prep_state_enqueue(hipStream_t st, int n, const PtTemporalState &s, float4 *c);
// The spatial estimate for every hit pixel whose cv[p].w is negative: cv[p].w = count * var_s(l(cv.rgb)), count = xn[p].w when
// count_from_xn, else 1.  nh / xn: normal + hit flag and position (+ count) per pixel; ids may be NULL (no id test).
hipError_t pt_variance_spatial_enqueue(hipStream_t st, int w, int h, const ptx_denoise_params &dp, const ptx_variance_params &vp,
                                       const float4 *nh, const float4 *xn, const int2 *ids, int count_from_xn, float4 *cv);
// dp.passes variance-guided passes from tmp0 (filled by one of the preps), ping-ponging with tmp1; out_rgb as pt_atrous_enqueue's;
// var_in (may be NULL) receives v0, var_out (may be NULL) the last pass's v, W*H floats each.
hipError_t pt_atrous_var_enqueue(hipStream_t st, int w, int h, const float4 *nh, const float4 *xt, const float4 *alb, float4 *tmp0,
                                 float4 *tmp1, float *out_rgb, float *var_in, float *var_out, const ptx_denoise_params &dp,
                                 const ptx_variance_params &vp);
