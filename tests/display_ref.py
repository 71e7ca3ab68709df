"""The display transform (ptx_display_* of include/mi355x_pathtracer.h, csrc/pt_display.hip) restated in numpy: float64 everywhere
but in two places where the rule itself names fp32 -- the sanitiser's IEEE division rgb / samples, which is ptx_write_pbo's, and the
quantiser, which numpy in float32 reproduces bit for bit from an fp32 z."""
import numpy as np

METER_MANUAL, METER_BLOCKS = 0, 1
TONE_CLAMP, TONE_REINHARD, TONE_ACES = 0, 1, 2
TRANSFER_LINEAR, TRANSFER_SRGB = 0, 1
C_MAX = 65504.0
L_MIN = 1e-8
LUM = np.array([0.2126, 0.7152, 0.0722])

BAYER8 = np.array([[0, 32, 8, 40, 2, 34, 10, 42],
                   [48, 16, 56, 24, 50, 18, 58, 26],
                   [12, 44, 4, 36, 14, 46, 6, 38],
                   [60, 28, 52, 20, 62, 30, 54, 22],
                   [3, 35, 11, 43, 1, 33, 9, 41],
                   [51, 19, 59, 27, 49, 17, 57, 25],
                   [15, 47, 7, 39, 13, 45, 5, 37],
                   [63, 31, 55, 23, 61, 29, 53, 21]])


def sanitise(rgb, samples):
    """step 1: (..., 3) float64 of rgb / samples (divided in fp32), NaN -> 0, clamped to [0, 65504]"""
    with np.errstate(all="ignore"):
        c = (np.asarray(rgb, np.float32) / np.float32(samples)).astype(np.float64)
    c = np.where(np.isnan(c), 0.0, c)
    return np.clip(c, 0.0, C_MAX)


def luminance(c):
    return c @ LUM


def block_grid(w, h):
    """(row_begin, col_begin): HK + 1 and WK + 1 integers, or two empty lists when the frame has no block"""
    hk, wk = (h + 8) // 16, (w + 8) // 16
    if hk == 0 or wk == 0:
        return [], []
    return [i * h // hk for i in range(hk + 1)], [j * w // wk for j in range(wk + 1)]


def block_means(rgb, samples, w, h):
    """(HK, WK) float64: the mean luminance of every block of the sanitised frame"""
    rows, cols = block_grid(w, h)
    lum = luminance(sanitise(rgb, samples).reshape(h, w, 3))
    out = np.zeros((max(len(rows) - 1, 0), max(len(cols) - 1, 0)))
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            out[i, j] = lum[rows[i]:rows[i + 1], cols[j]:cols[j + 1]].mean()
    return out


def meter(blocks, key=0.18):
    """dict(metered, log2_mean, blocks_used, blocks_total) of step 2 from the block means"""
    voters = blocks[blocks > L_MIN]
    m = float(np.log2(voters).mean()) if voters.size else 0.0
    metered = float(np.float64(np.float32(key)) / 2.0 ** m) if voters.size else 1.0
    return dict(metered=metered, log2_mean=m, blocks_used=int(voters.size), blocks_total=int(blocks.size))


def adapt(applied, metered, rate):
    """step 3 for a frame that is not the first: the new applied exposure"""
    la = np.log2(float(applied))
    return float(2.0 ** (la + float(np.float32(rate)) * (np.log2(float(metered)) - la)))


def tone(x, curve, white=4.0):
    if curve == TONE_REINHARD:
        lum = luminance(x)[..., None]
        y = x * (1.0 + lum / (white * white)) / (1.0 + lum)
    elif curve == TONE_ACES:
        y = x * (2.51 * x + 0.03) / (x * (2.43 * x + 0.59) + 0.14)
    else:
        y = x
    return np.clip(y, 0.0, 1.0)


def transfer(y, kind):
    if kind == TRANSFER_LINEAR:
        return y
    return np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.power(y, 1.0 / 2.4) - 0.055)


def display(rgb, samples, exposure, curve, kind, white=4.0):
    """steps 1, 4, 5, 6 in float64: z (..., 3) for the whole exposure E = `exposure` (MANUAL: the parameter; BLOCKS: applied * it)"""
    x = sanitise(rgb, samples) * float(exposure)
    return transfer(tone(x, curve, white), kind)


def quantise(z, w, h, quantize=1, dither=0):
    """step 7 on a float32 z (h*w*3 values, row major): (h, w, 4) uint8 codes with alpha 0, in the device's own arithmetic"""
    z = np.asarray(z, np.float32).reshape(h, w, 3)
    if not quantize:
        q = (z.astype(np.float64) * 255.0).astype(np.int32)
    else:
        t = np.full((h, w), np.float32(0.5))
        if dither:
            ys, xs = np.mgrid[0:h, 0:w]
            t = ((2 * BAYER8[ys & 7, xs & 7] + 1).astype(np.float32) / np.float32(128.0)).astype(np.float32)
        q = (z * np.float32(255.0) + t[..., None]).astype(np.float32).astype(np.int32)
    out = np.zeros((h, w, 4), np.uint8)
    out[..., :3] = q.astype(np.uint8)
    return out


def reference_setting_codes(rgb, samples, w, h):
    """meter MANUAL, exposure 1, tone CLAMP, transfer LINEAR, quantize 0: what ptx_write_pbo writes"""
    z = display(rgb, samples, 1.0, TONE_CLAMP, TRANSFER_LINEAR)
    return quantise_f64_truncate(z, w, h)


def quantise_f64_truncate(z, w, h):
    """quantize 0 on a float64 z whose values are fp32 numbers (the reference setting: z is the clamped fp32 quotient itself)"""
    out = np.zeros((h, w, 4), np.uint8)
    out[..., :3] = (np.asarray(z, np.float64).reshape(h, w, 3) * 255.0).astype(np.int32).astype(np.uint8)
    return out
