"""The prefilter of the network denoiser's guides restated (include/mi355x_pathtracer.h, "prefiltered guides"; csrc/pt_nn_aux.hip), for
its tests.  tests/unet_ref.py is imported as it is: the TZA writer, the network and the colour transforms are its own.  Added here:
  * the two auxiliary transforms (an albedo image, a normal image) in numpy float32, step for step as the kernels take them -- every
    step is one IEEE fp32 operation, so these give the device's bits -- and in float64 for the bound of the whole filter;
  * the whole auxiliary filter (transform, network, transform) in float64 or float32;
  * a pass-through weight builder: a blob of any accepted channel table through which three chosen input channels come out as
    fp16(g * fp16(x)) exactly, so that what a network was fed can be read from what it gives."""
import numpy as np

import unet_ref as U

ALBEDO, NORMAL = 1, 2                       # PTX_NN_AUX_ALBEDO, PTX_NN_AUX_NORMAL
F32 = np.float32
FLT_MAX32 = np.finfo(np.float32).max


# ---- the transforms, float32, step for step ------------------------------------------------------------------------------------------
def _max32(v, lo):
    """fmaxf(v, lo) on numbers; of the two zeros the positive one, as the device's maximum orders them"""
    return np.where(v > lo, v, F32(lo)).astype(F32)


def _min32(v, hi):
    return np.where(v < hi, v, F32(hi)).astype(F32)


def _sanitise32(v, lo, hi):
    v = np.asarray(v, F32)
    return np.where(np.isnan(v), F32(0), _min32(_max32(v, lo), hi)).astype(F32)


def _inv32(scale):
    return F32(1) / F32(scale) if scale != 0 else F32(0)


def aux_input_f32(image, kind, srgb=0, scale=1.0):
    """(H, W, 3) float32: what k_nn_aux_input gives the network before the rounding to fp16.  The albedo kind is restated in float32
    only without its curve (srgb != 0): the curve has a powf, which the device's own colour path is the reference for."""
    image = np.asarray(image, F32)
    with np.errstate(all="ignore"):
        if kind == NORMAL:
            assert not srgb
            return (_sanitise32(image * F32(scale), -1.0, 1.0) * F32(0.5) + F32(0.5)).astype(F32)
        assert srgb, "the sRGB curve is not restated in float32"
        return _sanitise32((image / F32(1)) * F32(scale), 0.0, 1.0)


def aux_output_f32(net, kind, srgb=0, scale=1.0):
    """(H, W, 3) float32: k_nn_aux_output on the network's three output channels"""
    with np.errstate(all="ignore"):
        v = _sanitise32(net, 0.0, FLT_MAX32)
        if kind == NORMAL:
            assert not srgb
            v = (v * F32(2) - F32(1)).astype(F32)
            v = _max32(v, -1.0)
        else:
            assert srgb, "the sRGB curve is not restated in float32"
        return (_min32(v, 1.0) * _inv32(scale)).astype(F32)


# ---- the transforms, float64 ---------------------------------------------------------------------------------------------------------
def aux_input(image, kind, srgb=0, scale=1.0):
    """(H, W, 3) float64; image * scale is formed in float32, as the device forms it"""
    c = (np.asarray(image, F32) * F32(scale)).astype(F32)
    if kind == NORMAL:
        return U._sanitise(c, -1.0, 1.0) * 0.5 + 0.5
    return U.forward(U._sanitise(c, 0.0, 1.0), U.mode_of(0, srgb))


def aux_output(net, kind, srgb=0, scale=1.0):
    if kind != NORMAL:
        return U.output_transform(net, 0, srgb, scale)
    v = np.clip(U._sanitise(net, 0.0, U.FLT_MAX) * 2.0 - 1.0, -1.0, 1.0)
    return v * (float(_inv32(scale)))


def aux_denoise(image, kind, weights, srgb=0, scale=1.0, dtype_name="float64"):
    """the whole auxiliary filter, (H, W, 3) float64.  float64: the definition; float32: the float32 transforms above where they exist
    (the normal kind, the albedo kind without its curve) around the network in float32."""
    f32 = dtype_name == "float32" and (kind == NORMAL or srgb)
    x = aux_input_f32(image, kind, srgb, scale) if f32 else aux_input(image, kind, srgb, scale)
    net = U.unet(x, weights, dtype_name)
    if f32:
        return aux_output_f32(net.astype(F32), kind, srgb, scale).astype(np.float64)
    return aux_output(net, kind, srgb, scale)


# ---- pass-through weights --------------------------------------------------------------------------------------------------------------
def passthrough_weights(ic, pick, g=1.0, channels=None):
    """{name.weight / name.bias: array} of the table `channels` (default: the standard one with ic inputs), every weight and bias zero
    except three centre taps per end layer: dec_conv1a's output k reads input channel pick[k] (of the skip, behind the upsampled
    source's channels) times g, dec_conv1b and dec_conv0 hand output k on.  The network's output k is then fp16(g * fp16(x[pick[k]]))
    for x >= 0: every sum has one non-zero term, the ReLUs pass it, dec_conv1a rounds it once and nothing after changes it."""
    channels = channels or U.standard_channels(ic)
    assert len(pick) == 3 and all(0 <= c < ic for c in pick)
    out = {}
    for name, cin, cout in channels:
        total = sum(cin) if isinstance(cin, tuple) else cin
        w = np.zeros((cout, total, 3, 3), np.float32)
        if name == "dec_conv1a":
            d2 = cin[0]
            assert cin[1] == ic and cout >= 3
            for k, c in enumerate(pick):
                w[k, d2 + c, 1, 1] = g
        elif name in ("dec_conv1b", "dec_conv0"):
            assert cout >= 3 and total >= 3
            for k in range(3):
                w[k, k, 1, 1] = 1.0
        out[name + ".weight"] = w
        out[name + ".bias"] = np.zeros(cout, np.float32)
    return out


def passthrough(x, g=1.0):
    """fp16(g * fp16(x)) as float32: what a pass-through network gives for the input value x (float32, >= 0), g a power of two or 1"""
    with np.errstate(over="ignore"):
        xh = np.asarray(x, F32).astype(np.float16).astype(F32)
        return (F32(g) * xh).astype(np.float16).astype(F32)
