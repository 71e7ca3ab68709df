"""Cases for the display transform's kernels (csrc/pt_display.hip) at the sizes and settings the small frames of tests/test_gpu_display.py
cannot reach, in pure numpy: tests/test_display_grid_cpu.py checks that they are what they claim to be, tests/test_gpu_display_grid.py
runs them on the device.

    column_frame : a frame of one column of blocks, the cheapest with a given block count, for k_display_meter's four loads per trip
    hdr_buffer   : tests/test_gpu_display.py's random HDR recipe without the zeroed first block, for blocks of more than 512 pixels
    sweep_frame  : every value class a channel can hold, as grey pixels and beside saturated channels, for k_display_map
    MAP_GRID     : tone x transfer x exposure, a samples axis and a white axis, meter MANUAL throughout
    TAIL_SIZES   : every W*H mod 4, frames below one quad, and exactly one quad
"""
import numpy as np

import display_ref as dr

NTM = 1024                                   # k_display_meter's workgroup: thread t takes blocks t, t + NTM, t + 2 NTM, t + 3 NTM per trip
# around every guard of the four loads (k + j NTM < nblocks, j = 1..3), the second trip (4097) and its first guard (5121)
METER_BLOCK_COUNTS = (1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097, 5121)
BELOW_L_MIN, ABOVE_L_MIN = 2.0 ** -27, 2.0 ** -26        # 7.45e-9 and 1.49e-8 around L_MIN = 1e-8: a factor above 1.3 either way


def block_exponents(nblocks):
    """e_b = (7 b mod 37) - 18: 7 * 1024 j mod 37 = 27, 17, 7, 34 for j = 1..4, so blocks NTM j apart never share an exponent"""
    return (7 * np.arange(nblocks) % 37) - 18


def column_blocks(nblocks, seed):
    """(values (nblocks,) float64 of the constant blocks, index of the block below L_MIN, index of the one above)"""
    assert nblocks >= 4
    b = np.arange(nblocks)
    v = np.ldexp(1.0, block_exponents(nblocks))
    v[b % 53 == 0] = 0.0
    below, above = np.random.default_rng(seed).choice(np.flatnonzero(b % 53 != 0), 2, replace=False)
    v[below], v[above] = BELOW_L_MIN, ABOVE_L_MIN
    return v, int(below), int(above)


def column_frame(nblocks, seed=0, scale=1.0):
    """8 x (16 nblocks - 8): WK = 1, HK = nblocks, blocks of 8 x 15 or 8 x 16 pixels.  Block b is constant in all three channels at
    2^e_b but for every 53rd block (zeros), one block at 2^-27 (no vote) and one at 2^-26 (a vote), times `scale` (a power of two).
    dict(rgb (H, 8, 3) float32, w, h, blocks (nblocks,) float64: the luminances of the sanitised blocks, blocks_used, log2_mean: the
    float64 mean of log2 over the voting ones, below, above)"""
    w, h = 8, 16 * nblocks - 8
    rows, cols = dr.block_grid(w, h)
    assert len(rows) == nblocks + 1 and len(cols) == 2
    v, below, above = column_blocks(nblocks, seed)
    v = v * float(scale)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)                 # every value is an fp32 number
    per_row = np.repeat(v.astype(np.float32), np.diff(rows))
    rgb = np.ascontiguousarray(np.broadcast_to(per_row[:, None, None], (h, w, 3)))
    lum = np.minimum(v, dr.C_MAX) * dr.LUM.sum()
    voters = lum > dr.L_MIN
    assert not ((lum > 0.75 * dr.L_MIN) & (lum < 1.3 * dr.L_MIN)).any()               # no vote is decided by rounding
    return dict(rgb=rgb, w=w, h=h, blocks=lum, blocks_used=int(voters.sum()), log2_mean=float(np.log2(lum[voters]).mean()),
                below=below, above=above)


def hdr_buffer(w, h):
    """tests/test_gpu_display.py's _buffer without the zeroed block (0, 0) -- a 23 x 23 frame is one block: a log-normal luminance over
    six decades, about 30 % exact zeros, a few NaN, negative, +inf and 1e30 entries, one 1e30 in the last pixel"""
    rng = np.random.default_rng(1000 * w + h)
    lum = 10.0 ** np.clip(rng.normal(0.0, 1.0, (h, w)), -3.0, 3.0)
    rgb = (lum[..., None] * rng.uniform(0.2, 1.8, (h, w, 3))).astype(np.float32)
    rgb[rng.random((h, w)) < 0.3] = 0.0
    flat = rgb.reshape(-1)
    bad = rng.choice(3 * w * h, 12, replace=False)
    flat[bad[0:3]] = np.nan
    flat[bad[3:6]] = -2.5
    flat[bad[6:9]] = np.inf
    flat[bad[9:12]] = 1e30
    flat[-1] = 1e30           # the clamped entries carry most of a block's sum: one of them in the last pixel, the third trip's at 23 x 23
    return rgb


EXPOSURES = (2.0 ** -20, 2.0 ** -6, 1.0, 37.5, 2.0 ** 20, 1e7, 1e15, 3e34)          # 65504 * 3e34 overflows fp32
SAMPLES = (1.0, 3.0, 4096.0, 0.125)
WHITES = (1e-20, 0.25, 1.0, 4.0, 1e4, 1e20)
TONES = ("clamp", "reinhard", "aces")
TRANSFERS = ("linear", "srgb")
SRGB_KNEE = 0.0031308
SWEEP_SIZE = (64, 67)


def _neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def sweep_values():
    """the channel values of sweep_frame, float32, before the test's `samples` scales them"""
    f = np.float32
    out = [f(0.0), f(-0.0), f(1e-40), f(1e-8)]
    out += list(np.geomspace(1e-8, 65504.0, 160).astype(f))
    out += _neighbours(65504.0)
    out += [f(1e30), f(np.inf), f(-2.5), f(-1e30), f(np.nan)]
    for e in EXPOSURES:                                                              # the pre-images of the sRGB branch point
        out += _neighbours(f(SRGB_KNEE) / f(e))
    return np.array(out, f)


def sweep_frame(w=SWEEP_SIZE[0], h=SWEEP_SIZE[1]):
    """(h, w, 3) float32.  Every value of sweep_values as a grey pixel, as one channel beside one saturated channel and one of the next
    value, and beside two saturated ones (65504, 1e30 and +inf in turn, in every channel position in turn), so that Reinhard's L
    differs from the channel it scales; the list repeated in row-major order until the frame is full, so that a value meets several
    dither phases and both the vector body and its tail."""
    v = sweep_values()
    sat = np.array([65504.0, 1e30, np.inf], np.float32)
    pix = []
    for i, x in enumerate(v):
        nxt, s = v[(i + 1) % len(v)], sat[i % 3]
        pix.append((x, x, x))
        pix.append(tuple(np.roll(np.array([x, s, nxt], np.float32), i % 3)))
        pix.append(tuple(np.roll(np.array([x, s, s], np.float32), i % 3)))
    pix = np.array(pix, np.float32)
    assert len(pix) <= w * h
    return np.ascontiguousarray(np.resize(pix, (w * h, 3)).reshape(h, w, 3))


HUGE_WHITES = (1e10, 1e15, 1e20)             # with E of 1e15 and 3e34: x and L beyond fp32 while a channel's y = x / white^2 stays below 1


def _grid():
    g = [dict(tone=t, transfer=x, exposure=e, samples=3.0, white=4.0) for t in TONES for x in TRANSFERS for e in EXPOSURES]
    g += [dict(tone=t, transfer=x, exposure=e, samples=s, white=4.0) for t in TONES for x in TRANSFERS for e in (1.0, 37.5)
          for s in SAMPLES if s != 3.0]
    g += [dict(tone="reinhard", transfer=x, exposure=e, samples=3.0, white=wh) for x in TRANSFERS for e in (1.0, 37.5)
          for wh in WHITES if wh != 4.0]
    g += [dict(tone="reinhard", transfer=x, exposure=e, samples=3.0, white=wh) for x in TRANSFERS for e in (1e15, 3e34) for wh in HUGE_WHITES]
    return tuple(g)


# every tone x transfer x exposure at samples 3 and white 4 (48), the other samples (36) and, for Reinhard, the other whites (20) at
# exposure 1 and 37.5, and the huge whites at the two largest exposures (12)
MAP_GRID = _grid()
QUANTISERS = ((0, 0), (1, 0), (1, 1))        # (quantize, dither)


def case_id(c):
    return "%s-%s-E%.4g-s%g-w%g" % (c["tone"], c["transfer"], c["exposure"], c["samples"], c["white"])


def map_launches():
    """[(case, (quantize, dither))]: every case once with keep_float, the quantiser taken in turn, and all three quantisers for the six
    tone x transfer pairs at exposure 37.5, samples 3, white 4: 128 launches"""
    out = [(c, QUANTISERS[i % 3]) for i, c in enumerate(MAP_GRID)]
    for i, c in enumerate(MAP_GRID):
        if (c["exposure"], c["samples"], c["white"]) == (37.5, 3.0, 4.0):
            out += [(c, q) for q in QUANTISERS if q != QUANTISERS[i % 3]]
    return out


# W*H mod 4 = 1, 2, 3, 0, 1, 2, 0, 3, 1; no quad at all (1, 2, 3 pixels) and exactly one quad with no tail (2 x 2)
TAIL_SIZES = ((1, 1), (2, 1), (3, 1), (2, 2), (5, 1), (6, 7), (8, 8), (37, 23), (97, 61))
TAIL_MOD4 = (1, 2, 3, 0, 1, 2, 0, 3, 1)

X_CAP = 2.0 ** 60                              # map_pixel's (csrc/pt_display.hip): ACES holds x to it, Reinhard changes form at L = X_CAP


def premapped(case):
    """float64 y before the clamp, (h, w, 3), of one grid case on the sweep frame: the rule itself"""
    rgb = sweep_frame() * np.float32(case["samples"])
    x = dr.sanitise(rgb, case["samples"]) * float(np.float32(case["exposure"]))
    if case["tone"] == "reinhard":
        lum = dr.luminance(x)[..., None]
        w = float(np.float32(case["white"]))
        return x * (1.0 + lum / (w * w)) / (1.0 + lum)
    if case["tone"] == "aces":
        return x * (2.51 * x + 0.03) / (x * (2.43 * x + 0.59) + 0.14)
    return x


def saturated(case, y):
    """where z has to be exactly transfer(1): y >= 1, as the rule says.  With the huge whites at the two largest exposures a grey pixel's y = x (1 + L / white^2) /
    (1 + L) comes down on 1 from above, to within far less than an fp32 ulp, over the whole upper half of the sweep; whether the fp32
    quotient lands on 1 or on 1 - 2^-24 is rounding there, not a decision, so those cases ask for exactness from 1 + 2e-6 (16 ulps) on
    and leave the band below it to the metric.  (tests/test_display_grid_cpu.py: no other case has a y in that band.)"""
    return y >= (1.0 + 2e-6 if huge(case) else 1.0)


def huge(case):
    """the cases beyond the issue's grid: a huge white at one of the two largest exposures"""
    return case["white"] in HUGE_WHITES and case["exposure"] >= 1e15


def _aces_f32(x):
    f = np.float32
    return (x * (f(2.51) * x + f(0.03))) / (x * (f(2.43) * x + f(0.59)) + f(0.14))


def tone_f32(c, E, tone, white=4.0, fixed=True):
    """Steps 4 and 5 of map_pixel operation for operation in float32 on sanitised pixels c (..., 3): y after the clamp.  fixed=False is
    the rule's expression written down as it stands, which divides inf by inf beyond fp32's range."""
    f = np.float32
    c, E, w = np.asarray(c, f), f(E), f(white)
    with np.errstate(all="ignore"):
        x = (c * E).astype(f)
        if tone == "aces":
            y = _aces_f32(np.where(x > f(X_CAP), f(X_CAP), x).astype(f) if fixed else x)
        elif tone == "reinhard":
            lum = lambda v: ((f(0.2126) * v[..., 0] + f(0.7152) * v[..., 1]) + f(0.0722) * v[..., 2])[..., None]
            L = lum(x)
            w2 = w * w
            num, den = f(1) + L / w2, f(1) + L
            y = x * num / den
            if fixed:
                y = np.where(num > np.finfo(f).max, x / w2 * (L / den), y)
                y = np.where(~(L < f(X_CAP)), c / lum(c) + c / w * E / w, y)
        else:
            y = x
    return clamp01_f32(y)


def clamp01_f32(y):
    """fminf(fmaxf(y, 0), 1): both return the other operand when one is NaN"""
    y = np.asarray(y, np.float32)
    return np.where(np.isnan(y), np.float32(0), np.clip(y, np.float32(0), np.float32(1))).astype(np.float32)
