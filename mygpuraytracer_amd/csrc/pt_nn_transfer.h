// pt_nn_transfer.h -- the network denoiser's transfer functions and their constants (OIDN core/color.ispc, restated; the definition is in
// include/mi355x_pathtracer.h), for the units whose kernels stand at the network's ends: pt_nn.hip (colour, with its guides as they
// are), pt_nn_aux.hip (an albedo or a normal image alone) and pt_nn_image.hip (either, on described images).  Every step is one IEEE
// fp32 operation under -ffp-contract=off, which all of them keep.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

namespace pt_nn_transfer {

constexpr float PU_A = 1.41283765e+03f, PU_B = 1.64593172e+00f, PU_C = 4.31384981e-01f, PU_D = -2.94139609e-03f, PU_E = 1.92653254e-01f,
                PU_F = 6.26026094e-03f, PU_G = 9.98620152e-01f, PU_Y0 = 1.57945760e-06f, PU_Y1 = 3.22087631e-02f, PU_X0 = 2.23151711e-03f,
                PU_X1 = 3.70974749e-01f;
constexpr float SRGB_A = 12.92f, SRGB_B = 1.055f, SRGB_C = 1.f / 2.4f, SRGB_D = -0.055f, SRGB_Y0 = 0.0031308f, SRGB_X0 = 0.04045f;
enum { MODE_LINEAR = 0, MODE_SRGB = 1, MODE_PU = 2 };

// PU(65504) in double from the fp32 constants, rounded once: the normalisation of the hdr mode and its reciprocal
inline float pu_xmax() { return (float)((double)PU_E * log(65504.0 + (double)PU_F) + (double)PU_G); }
inline float pu_norm() { return (float)(1.0 / (double)pu_xmax()); }

__device__ __forceinline__ float sanitise(float v, float lo, float hi) { return v != v ? 0.f : fminf(fmaxf(v, lo), hi); }

__device__ __forceinline__ float transfer_forward(float y, int mode, float norm) {
    if (mode == MODE_LINEAR) return y;
    if (mode == MODE_SRGB) return y <= SRGB_Y0 ? SRGB_A * y : SRGB_B * powf(y, SRGB_C) + SRGB_D;
    const float x = y <= PU_Y0 ? PU_A * y : y <= PU_Y1 ? PU_B * powf(y, PU_C) + PU_D : PU_E * logf(y + PU_F) + PU_G;
    return x * norm;
}

__device__ __forceinline__ float transfer_inverse(float x, int mode, float xmax) {
    if (mode == MODE_LINEAR) return x;
    if (mode == MODE_SRGB) return x <= SRGB_X0 ? x / SRGB_A : powf((x - SRGB_D) / SRGB_B, 1.f / SRGB_C);
    x = x * xmax;
    return x <= PU_X0 ? x / PU_A : x <= PU_X1 ? powf((x - PU_D) / PU_B, 1.f / PU_C) : expf((x - PU_G) / PU_E) - PU_F;
}

}  // namespace pt_nn_transfer
