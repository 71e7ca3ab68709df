// pt_nn_lightmap.h -- internal header of the lightmap filter (pt_nn_lightmap.hip: ptx_nn_denoise_lightmap_* of
// include/mi355x_pathtracer.h, "lightmap"): the constants of OIDN's Log transfer function and what a call refuses of its two scalar
// arguments.  No hip* call.  Not part of the C ABI.
#pragma once
#include <math.h>

namespace pt_nn_lightmap {

// log(65504 + 1) in double, rounded once: the normalisation of the HDR mode and its reciprocal, formed like pu_xmax / pu_norm
// (pt_nn_transfer.h).  0x1.62e050p+3 and 0x1.71587ep-4.
inline float log_xmax() { return (float)log(65505.0); }
inline float log_norm() { return (float)(1.0 / (double)log_xmax()); }

// NULL when usable, else what is wrong (the ptx_last_error message after the entry point's name)
inline const char *args_problem(int directional, float input_scale) {
    if (directional != 0 && directional != 1) return "directional must be 0 (the HDR lightmap) or 1 (the directional lightmap)";
    if (!isnan(input_scale) && (!(input_scale > 0.f) || isinf(input_scale))) return "input_scale must be NaN (automatic) or finite and > 0";
    return nullptr;
}

}  // namespace pt_nn_lightmap
