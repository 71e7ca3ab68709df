"""The lightmap filter restated (include/mi355x_pathtracer.h, "lightmap"; csrc/pt_nn_lightmap.hip), for its tests.  tests/unet_ref.py
and tests/unet_aux_ref.py are imported as they are.  Both modes, twice:
  * in numpy float32, step for step as the kernels take them.  The directional mode has no transcendental function, so there these are
    the device's bits; the HDR mode's logf / expf are the correctly rounded ones on the device (formed in double, rounded once) and
    here, so there they are the device's bits too but for the rare value whose double lies within a double's ulp of a float tie;
  * in float64, the definition the device is held to within a bound.  Two steps of it are float32 operations by definition and are
    formed in float32 here as well, as tests/unet_aux_ref.py forms image * scale: image * scale and, in the HDR mode, v + 1.  (v + 1
    rounds to a float near 1 for a small v; that rounding is the function's, OIDN's own, not an error of an implementation.)
HDR is OIDN's Log transfer function with hdr: x = log(v + 1) / log(65505), y = exp(x log(65505)) - 1.  Directional is OIDN's Linear one
with snorm: the normal role's arithmetic (unet_aux_ref.aux_input_f32 / aux_output_f32 of kind NORMAL)."""
import numpy as np

import unet_aux_ref as X
import unet_ref as U

F32 = np.float32
FLT_MAX32 = X.FLT_MAX32
LOG_XMAX = float(F32(np.log(65505.0)))                 # log(65504 + 1) in double, rounded once
LOG_NORM = float(F32(1.0 / LOG_XMAX))                  # its reciprocal in double, rounded once


# ---- float32, step for step ------------------------------------------------------------------------------------------------------------
def input_f32(image, directional, scale=1.0):
    """(H, W, 3) float32: what k_nn_lightmap_input gives the network before the rounding to fp16"""
    image = np.asarray(image, F32)
    with np.errstate(all="ignore"):
        v = (image * F32(scale)).astype(F32)
        if directional:
            return (X._sanitise32(v, -1.0, 1.0) * F32(0.5) + F32(0.5)).astype(F32)
        v = X._sanitise32(v, 0.0, FLT_MAX32)
        return (np.log((v + F32(1)).astype(F32).astype(np.float64)).astype(F32) * F32(LOG_NORM)).astype(F32)


def output_f32(net, directional, scale=1.0):
    """(H, W, 3) float32: k_nn_lightmap_output on the network's three output channels"""
    with np.errstate(all="ignore"):
        v = X._sanitise32(net, 0.0, FLT_MAX32)
        if directional:
            v = (v * F32(2) - F32(1)).astype(F32)
            v = X._min32(X._max32(v, -1.0), 1.0)
        else:
            v = (np.exp((v * F32(LOG_XMAX)).astype(F32).astype(np.float64)).astype(F32) - F32(1)).astype(F32)
        return (v * X._inv32(scale)).astype(F32)


# ---- float64 -----------------------------------------------------------------------------------------------------------------------------
def input_f64(image, directional, scale=1.0):
    """(H, W, 3) float64; image * scale and v + 1 are formed in float32, as the definition has them"""
    with np.errstate(all="ignore"):
        c = (np.asarray(image, F32) * F32(scale)).astype(F32)
        if directional:
            return U._sanitise(c, -1.0, 1.0) * 0.5 + 0.5
        v1 = (X._sanitise32(c, 0.0, FLT_MAX32) + F32(1)).astype(F32)
        return np.log(v1.astype(np.float64)) * LOG_NORM


def output_f64(net, directional, scale=1.0):
    with np.errstate(all="ignore"):
        v = U._sanitise(net, 0.0, U.FLT_MAX)
        if directional:
            v = np.clip(v * 2.0 - 1.0, -1.0, 1.0)
        else:
            v = np.exp(v * LOG_XMAX) - 1.0
        return v * float(X._inv32(scale))


def denoise(image, directional, weights, scale=1.0, dtype_name="float64"):
    """the whole filter, (H, W, 3) float64: transform, network (unet_ref.unet), transform"""
    if dtype_name == "float32":
        net = U.unet(input_f32(image, directional, scale), weights, dtype_name)
        return output_f32(net.astype(F32), directional, scale).astype(np.float64)
    return output_f64(U.unet(input_f64(image, directional, scale), weights), directional, scale)
