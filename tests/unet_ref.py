"""The network denoiser restated (include/mi355x_pathtracer.h, "network denoiser"; csrc/pt_nn.hip, csrc/pt_tza.h), for its tests.
Nothing here reads the library or the reference tree:
  * a TZA writer and reader of their own (format version 2), on struct + numpy;
  * the U-Net on CPU torch tensors with the definition's fp16 rounding points, in float64 or float32;
  * the transfer functions and the input / output transforms in numpy float64 (constants rounded to float32 first, as the device has them);
  * synthetic weights (He-normal, seeded) for the standard channel table or any other that follows the graph (table())."""
import struct

import numpy as np

MAGIC = 0x41D7

# OIDN 1.4's channel table (training/model.py): name -> (cin as a function of ic, cout)
EC1, EC2, EC3, EC4, EC5, DC4, DC3, DC2, DC1A, DC1B = 32, 48, 64, 80, 96, 112, 96, 64, 64, 32
LAYER_NAMES = ["enc_conv0", "enc_conv1", "enc_conv2", "enc_conv3", "enc_conv4", "enc_conv5a", "enc_conv5b", "dec_conv4a", "dec_conv4b",
               "dec_conv3a", "dec_conv3b", "dec_conv2a", "dec_conv2b", "dec_conv1a", "dec_conv1b", "dec_conv0"]


def standard_channels(ic):
    """[(name, cin, cout)] of the standard network with ic input channels; the two-source layers' cin is (upsampled, skip)"""
    return [("enc_conv0", ic, EC1), ("enc_conv1", EC1, EC1), ("enc_conv2", EC1, EC2), ("enc_conv3", EC2, EC3), ("enc_conv4", EC3, EC4),
            ("enc_conv5a", EC4, EC5), ("enc_conv5b", EC5, EC5), ("dec_conv4a", (EC5, EC3), DC4), ("dec_conv4b", DC4, DC4),
            ("dec_conv3a", (DC4, EC2), DC3), ("dec_conv3b", DC3, DC3), ("dec_conv2a", (DC3, EC1), DC2), ("dec_conv2b", DC2, DC2),
            ("dec_conv1a", (DC2, ic), DC1A), ("dec_conv1b", DC1A, DC1B), ("dec_conv0", DC1B, 3)]


def table(ic, e1, e2, e3, e4, e5, d4, d3, d2, d1a, d1b):
    """[(name, cin, cout)] of the same graph with channel counts of the caller's (each in 1 .. 256): what a blob may bring.
    standard_channels(ic) == table(ic, 32, 48, 64, 80, 96, 112, 96, 64, 64, 32)"""
    return [("enc_conv0", ic, e1), ("enc_conv1", e1, e1), ("enc_conv2", e1, e2), ("enc_conv3", e2, e3), ("enc_conv4", e3, e4),
            ("enc_conv5a", e4, e5), ("enc_conv5b", e5, e5), ("dec_conv4a", (e5, e3), d4), ("dec_conv4b", d4, d4),
            ("dec_conv3a", (d4, e2), d3), ("dec_conv3b", d3, d3), ("dec_conv2a", (d3, e1), d2), ("dec_conv2b", d2, d2),
            ("dec_conv1a", (d2, ic), d1a), ("dec_conv1b", d1a, d1b), ("dec_conv0", d1b, 3)]


# two tables off the standard one (tests/test_gpu_nn_channels.py, tests/test_nn_cpu.py).  NARROW: counts that are no multiple of 16, 8 or
# 4, a layer below one block (8, 5), ragged two-source layers.  WIDE: Cout of 8 blocks in one group (128), above 128 (two groups: 144,
# 256, 200, 136, and 129, whose tenth block is padding), Cin up to 256 + 144 over two sources.
NARROW = (20, 40, 8, 17, 33, 50, 24, 12, 31, 5)
WIDE = (48, 72, 128, 144, 256, 200, 136, 129, 16, 64)
# the level (frame >> level) of each layer's output before its pool, in the graph's order: ptx_nn_info.macs sums 9 Cin Cout pixels over it
LEVELS = (0, 0, 1, 2, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 0)


# ---- TZA -----------------------------------------------------------------------------------------------------------------------------
_TYPES = {"f": np.float32, "h": np.float16}


def write_tza(tensors):
    """bytes of a TZA blob from [(name, array, layout)]; float32 -> f, float16 -> h.  Data and table aligned to 64 bytes."""
    out = bytearray(struct.pack("<HBBQ", MAGIC, 2, 0, 0))
    table = []
    pad = lambda: out.extend(b"\0" * (-len(out) % 64))
    for name, a, layout in tensors:
        a = np.ascontiguousarray(a)
        code = {np.dtype(np.float32): "f", np.dtype(np.float16): "h"}[a.dtype]
        assert len(layout) == a.ndim
        pad()
        table.append((name, a.shape, layout, code, len(out)))
        out.extend(a.tobytes())
    pad()
    at = len(out)
    out.extend(struct.pack("<I", len(table)))
    for name, shape, layout, code, offset in table:
        nb = name.encode()
        out.extend(struct.pack("<H", len(nb)) + nb + struct.pack("<B", len(shape)))
        for d in shape:
            out.extend(struct.pack("<I", d))
        out.extend(layout.encode("ascii") + code.encode("ascii") + struct.pack("<Q", offset))
    out[4:12] = struct.pack("<Q", at)
    return bytes(out)


def read_tza(blob):
    """{name: (array, layout, type code, offset)} of a TZA blob; ValueError on what the format does not allow"""
    blob = bytes(blob)
    magic, major, _minor, at = struct.unpack_from("<HBBQ", blob, 0)
    if magic != MAGIC or major != 2:
        raise ValueError("not a TZA version 2 blob")
    (count,) = struct.unpack_from("<I", blob, at)
    at += 4
    out = {}
    for _ in range(count):
        (n,) = struct.unpack_from("<H", blob, at)
        name = blob[at + 2:at + 2 + n].decode()
        at += 2 + n
        nd = blob[at]
        shape = struct.unpack_from("<%dI" % nd, blob, at + 1)
        at += 1 + 4 * nd
        layout = blob[at:at + nd].decode("ascii")
        code = blob[at + nd:at + nd + 1].decode("ascii")
        (offset,) = struct.unpack_from("<Q", blob, at + nd + 1)
        at += nd + 9
        if code not in _TYPES:
            raise ValueError("unsupported tensor data type")
        dt = np.dtype(_TYPES[code])
        a = np.frombuffer(blob, dt, int(np.prod(shape)), offset).reshape(shape)
        out[name] = (a, layout, code, offset)
    return out


def table_of(blob):
    """[(name, dims, layout, type, offset)] in the table's order: what ptx_debug_tza_list returns"""
    return [(k, tuple(int(d) for d in a.shape), layout, code, offset) for k, (a, layout, code, offset) in read_tza(blob).items()]


# ---- synthetic weights ---------------------------------------------------------------------------------------------------------------
def synthetic_weights(ic, seed, channels=None, dtype=np.float32):
    """{name.weight / name.bias: array}: He-normal weights (std sqrt(2 / (9 cin))), biases N(0, 0.1), from `seed`"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, cin, cout in channels or standard_channels(ic):
        cin = sum(cin) if isinstance(cin, tuple) else cin
        out[name + ".weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(dtype)
        out[name + ".bias"] = (rng.standard_normal(cout) * 0.1).astype(dtype)
    return out


def weights_blob(weights):
    return write_tza([(k, v, "oihw" if v.ndim == 4 else "x") for k, v in weights.items()])


# ---- transfer functions, float64 on float32 constants --------------------------------------------------------------------------------
_f = lambda v: float(np.float32(v))
PU_A, PU_B, PU_C, PU_D, PU_E, PU_F, PU_G = (_f(v) for v in (1.41283765e+03, 1.64593172e+00, 4.31384981e-01, -2.94139609e-03,
                                                           1.92653254e-01, 6.26026094e-03, 9.98620152e-01))
PU_Y0, PU_Y1, PU_X0, PU_X1 = (_f(v) for v in (1.57945760e-06, 3.22087631e-02, 2.23151711e-03, 3.70974749e-01))
SRGB_A, SRGB_B, SRGB_D, SRGB_Y0, SRGB_X0 = (_f(v) for v in (12.92, 1.055, -0.055, 0.0031308, 0.04045))
SRGB_C = _f(np.float32(1.0) / np.float32(2.4))
SRGB_RC = _f(np.float32(1.0) / np.float32(SRGB_C))
PU_RC = _f(np.float32(1.0) / np.float32(PU_C))
PU_XMAX = _f(PU_E * np.log(65504.0 + PU_F) + PU_G)        # PU(65504) in double, rounded once
PU_NORM = _f(1.0 / PU_XMAX)
FLT_MAX = float(np.finfo(np.float32).max)


def mode_of(hdr, srgb):
    return "pu" if hdr else "linear" if srgb else "srgb"


def forward(y, mode):
    y = np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        if mode == "linear":
            return y
        if mode == "srgb":
            return np.where(y <= SRGB_Y0, SRGB_A * y, SRGB_B * np.power(y, SRGB_C) + SRGB_D)
        x = np.where(y <= PU_Y0, PU_A * y, np.where(y <= PU_Y1, PU_B * np.power(y, PU_C) + PU_D, PU_E * np.log(y + PU_F) + PU_G))
        return x * PU_NORM


def inverse(x, mode):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if mode == "linear":
            return x
        if mode == "srgb":
            return np.where(x <= SRGB_X0, x / SRGB_A, np.power((x - SRGB_D) / SRGB_B, SRGB_RC))
        x = x * PU_XMAX
        return np.where(x <= PU_X0, x / PU_A, np.where(x <= PU_X1, np.power((x - PU_D) / PU_B, PU_RC), np.exp((x - PU_G) / PU_E) - PU_F))


def _sanitise(v, lo, hi):
    v = np.asarray(v, np.float64)
    return np.clip(np.where(np.isnan(v), 0.0, v), lo, hi)


def input_transform(rgb, albedo=None, normal=None, hdr=0, srgb=0, scale=1.0):
    """(H, W, ic) float64: what the network gets before the rounding to fp16.  rgb, albedo, normal float32 frames; rgb * scale is formed
    in float32, as the device forms it."""
    c = (np.asarray(rgb, np.float32) * np.float32(scale)).astype(np.float32)
    parts = [forward(_sanitise(c, 0.0, FLT_MAX if hdr else 1.0), mode_of(hdr, srgb))]
    if albedo is not None:
        parts.append(_sanitise(np.asarray(albedo, np.float32), 0.0, 1.0))
    if normal is not None:
        parts.append(_sanitise(np.asarray(normal, np.float32), -1.0, 1.0) * 0.5 + 0.5)
    return np.concatenate(parts, axis=-1)


def output_transform(net, hdr=0, srgb=0, scale=1.0):
    """(H, W, 3) float64 from the network's three output channels"""
    v = inverse(_sanitise(net, 0.0, FLT_MAX), mode_of(hdr, srgb))
    if not hdr:
        v = np.minimum(v, 1.0)
    inv = float(np.float32(1.0) / np.float32(scale)) if scale != 0 else 0.0
    return v * inv


# ---- the network ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _h(x, dtype):
    """one rounding to fp16 (nearest even), carried on in dtype.  Subnormal fp16 values are kept, as results here and as operands of
    the next convolution: that is the definition, and what the device does (measured on gfx950, tests/test_gpu_nn_channels.py), so
    the restatement has no flush-to-zero switch.  65520 and above rounds to inf."""
    torch = _torch()
    return x.to(torch.float16).to(dtype)


def conv(x, w, b, dtype, relu=True, half=True):
    """x (1, C, H, W) holding fp16 values in dtype; w float32 array rounded to fp16 here; b float32 array"""
    torch = _torch()
    F = torch.nn.functional
    wt = torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(torch.float16).to(dtype)
    bt = torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(dtype)
    y = F.conv2d(x, wt, None, padding=1)
    y = y + bt.view(1, -1, 1, 1)
    if relu:
        y = torch.relu(y)
    return _h(y, dtype) if half else y


def unet(x_in, weights, dtype_name="float64"):
    """The network on its input x_in (H, W, ic) (any float array: it is rounded to fp16 first), zero-padded right and bottom to
    multiples of 16; returns the three output channels (H, W, 3) as float64, before the output transform."""
    torch = _torch()
    F = torch.nn.functional
    dtype = {"float64": torch.float64, "float32": torch.float32}[dtype_name]
    h, w, _ic = x_in.shape
    hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    x = torch.from_numpy(np.ascontiguousarray(x_in, np.float64)).permute(2, 0, 1)[None]
    x = F.pad(x, (0, wp - w, 0, hp - h))
    x = _h(x.to(torch.float32), dtype)               # the device holds the transformed input in fp32 and rounds that
    W = lambda n: (weights[n + ".weight"], weights[n + ".bias"])
    pool = lambda t: F.max_pool2d(t, 2)
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
    t = conv(x, *W("enc_conv0"), dtype)
    p1 = pool(conv(t, *W("enc_conv1"), dtype))
    p2 = pool(conv(p1, *W("enc_conv2"), dtype))
    p3 = pool(conv(p2, *W("enc_conv3"), dtype))
    p4 = pool(conv(p3, *W("enc_conv4"), dtype))
    t = conv(conv(p4, *W("enc_conv5a"), dtype), *W("enc_conv5b"), dtype)
    for level, skip in (("4", p3), ("3", p2), ("2", p1), ("1", x)):
        t = torch.cat([up(t), skip], 1)
        t = conv(conv(t, *W("dec_conv%sa" % level), dtype), *W("dec_conv%sb" % level), dtype)
    t = conv(t, *W("dec_conv0"), dtype, relu=False, half=False)
    return t[0].permute(1, 2, 0)[:h, :w].to(torch.float64).numpy()


def denoise(rgb, weights, albedo=None, normal=None, hdr=0, srgb=0, scale=1.0, dtype_name="float64"):
    """the whole filter: input transform, network, output transform; (H, W, 3) float64"""
    x = input_transform(rgb, albedo, normal, hdr, srgb, scale)
    return output_transform(unet(x, weights, dtype_name), hdr, srgb, scale)
