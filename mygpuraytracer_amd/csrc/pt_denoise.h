// pt_denoise.h -- internal interface between the tracer (pt_engine.hip: G-buffer pass, tracer-level entry points) and the
// edge-avoiding a-trous filter (pt_denoise.hip).  Not part of the C ABI; include/mi355x_pathtracer.h has the public side.
//
// Device layout of the guide images, one record per pixel, pixelIndex = x + y*W (the frame's own order):
//   nh[i]  = float4(shading normal xyz, hit ? 1 : 0)
//   xt[i]  = float4(world position xyz, t)              (t is not read by the filter; ptx_read_gbuffer hands it out)
//   alb[i] = float4(albedo rgb, 0)
// Misses are all zeros.  The filter's colour ping-pong buffers are float4(rgb, 0) per pixel.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mi355x_pathtracer.h"

// NULL when the parameters are usable, else what is wrong with them (the ptx_last_error message)
const char *pt_denoise_params_problem(const ptx_denoise_params &p);

// Enqueues the whole filter on `st`: colour = rgb / spp (rgb: W*H*3 floats, e.g. the accumulation buffer), optional demodulation by
// max(albedo, 1e-3), p.passes a-trous passes ping-ponging between tmp0 and tmp1 (W*H float4 each), result W*H*3 floats of mean
// radiance in out_rgb.  Launch errors come back as the hipError_t of the first launch that failed.
hipError_t pt_atrous_enqueue(hipStream_t st, int w, int h, const float *rgb, float spp, const float4 *nh, const float4 *xt,
                             const float4 *alb, float4 *tmp0, float4 *tmp1, float *out_rgb, const ptx_denoise_params &p);
