"""The image metrics' test cases, shared by tests/test_metrics_cpu.py, tests/test_gpu_metrics.py and tests/golden/make_metrics_golden.py:
the shapes, the seeded images, and the two restatements of every case computed once (tests/metrics_ref.py: A in float64, B in
float32), with d, the largest |A - B| of the SSIM family over the whole list, which the GPU tier's bound is 4 times of."""
import numpy as np

import metrics_ref as R

# (W, H), the smallest at which each part can go wrong: below the window (SSIM not defined), one window, one more either way, no
# multiple of the 32 x 16 tile and several tiles, the smallest MS-SSIM frame (odd at every level: 161 -> 81 -> 41 -> 21 -> 11, every
# pool pads, the last scale is one window), even and odd mixed with both sides ending at 11, and one more.
SHAPES = [(1, 1), (10, 10), (11, 11), (12, 11), (11, 43), (27, 21), (193, 170), (161, 161), (176, 162), (200, 163)]
SSIM_SHAPES = [s for s in SHAPES if min(s) >= 11]
MSSSIM_SHAPES = [s for s in SHAPES if min(s) > 160]
DISTS = ["uniform", "normal"]
SEEDS = [1, 2, 3]
TRANSFORMS = ["none", "srgb", "hdr", "snorm"]
NOISE = 0.15                   # a = clip(b + NOISE * N(0, 1)): keeps every case's SSIM well inside (0, 1), see the CPU tier
EXPOSURE = 1.0                 # the hdr cases' (the metered one has a test of its own)


def shape_id(s):
    return "%dx%d" % s


def images(shape, dist, seed):
    """(a, b): float32 (H, W, 3) in [0, 1]; b uniform or N(0.5, 0.2) clipped, a = b + noise, clipped"""
    w, h = shape
    rng = np.random.default_rng([seed, w, h, DISTS.index(dist)])
    b = rng.random((h, w, 3)) if dist == "uniform" else np.clip(rng.normal(0.5, 0.2, (h, w, 3)), 0.0, 1.0)
    a = np.clip(b + NOISE * rng.standard_normal((h, w, 3)), 0.0, 1.0)
    return a.astype(np.float32), b.astype(np.float32)


def cases(shapes=SHAPES):
    return [(s, d, seed, t) for s in shapes for d in DISTS for seed in SEEDS for t in TRANSFORMS]


_CACHE = {}


def restated(case):
    """(A, B) of a case, each metrics_ref.metrics' dict with the map; computed once"""
    if case not in _CACHE:
        shape, dist, seed, t = case
        a, b = images(shape, dist, seed)
        _CACHE[case] = tuple(R.metrics(a, b, T, t, exposure=EXPOSURE, want_map=min(shape) >= 11) for T in (np.float64, np.float32))
    return _CACHE[case]


SSIM_FIELDS = ("ssim", "msssim", "ssim_c", "msssim_c", "mcs", "map")


def ssim_difference(x, y):
    """the largest difference of the SSIM family's fields that both hold (NaN where neither is defined)"""
    worst = 0.0
    for k in SSIM_FIELDS:
        if k in x and k in y:
            p, q = np.asarray(x[k], np.float64), np.asarray(y[k], np.float64)
            if not np.all(np.isnan(p)):
                worst = max(worst, float(np.nanmax(np.abs(p - q))))
    return worst


_D = []


def d_of_the_list():
    """d: the largest |A - B| of ssim, msssim, their per-channel values, mcs and the map, pixel by pixel, over every case"""
    if not _D:
        _D.append(max(ssim_difference(*restated(c)) for c in cases(SSIM_SHAPES)))
    return _D[0]
