"""The texel lookup rule in plain numpy (test infrastructure only): an independent restatement of what scatterRay, the albedo AOV and
the bump lookup do with a texture coordinate (src/interactions.h:172-179 and its copies), with the clamp this project puts where the
reference leaves the index undefined.  It calls neither the oracle nor the product.

    coordU = int32(trunc(f32(u) * f32(w)))          coordV likewise with h          (float32 products, truncated towards zero)
    pixelID = coordV * w + coordU                                                    (int64 here; no lookup of the tests overflows int32)
    byte    = clip(pixelID * ch + c, 0, w * h * ch - 1)                              (c = 0, 1, 2; a fourth channel is never read)

Nearest texel, no wrap, no flip: u == 1 gives coordU == w, which is the first texel of the NEXT row; v == 1 gives an index past the
last byte, which the clamp turns into the last byte of the map (all three channels then read that one byte); a negative index reads byte 0.

Keep |u|, |v| <= 8: beyond int32 the conversion of a float to int is undefined on the host and saturates on the GPU.  No NaN, no infinity."""
import functools

import numpy as np

INTERIOR, WRAP_ROW, CLAMPED_LOW, CLAMPED_HIGH, LAST_ROW, LAST_TEXEL, WRAP_OTHER = range(7)
CLASS_NAMES = ("interior", "coordU == w (wraps a row)", "clamped low", "clamped high", "last row", "last texel", "coordU outside [0, w]")


def coords(u, v, w, h):
    """(coordU, coordV) as int64 arrays"""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    assert np.all(np.abs(u) <= 8) and np.all(np.abs(v) <= 8), "texture coordinates beyond |8| are outside what the rule defines"
    cu = np.trunc(u * np.float32(w)).astype(np.int32).astype(np.int64)
    cv = np.trunc(v * np.float32(h)).astype(np.int32).astype(np.int64)
    return cu, cv


def byte_index(u, v, w, h, ch, c):
    cu, cv = coords(u, v, w, h)
    pixel = cv * np.int64(w) + cu
    return np.clip(pixel * np.int64(ch) + np.int64(c), 0, np.int64(w) * h * ch - 1)


def fetch(img, u, v):
    """img: (h, w, ch) uint8 -> (n, 3) uint8, the three bytes a lookup at (u, v) reads"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, ch = img.shape
    flat = img.reshape(-1)
    return np.stack([flat[byte_index(u, v, w, h, ch, c)] for c in range(3)], axis=-1)


def unit(b):
    """byte / 255 in float32 (one IEEE division)"""
    return np.asarray(b).astype(np.float32) / np.float32(255)


def emission_colour(c_in, b):
    """colour of a path that meets an emissive texel: c_in * ((b / 255) * 5)"""
    return np.asarray(c_in, np.float32) * (unit(b) * np.float32(5))


def tint(c_in, b):
    """colour of a path that scatters off a kd or ks texel: c_in * (b / 255)"""
    return np.asarray(c_in, np.float32) * unit(b)


def lit(b):
    """the emissive branch is taken when some channel of the ke texel exceeds FLT_EPSILON: when some byte is not 0"""
    return (np.asarray(b) != 0).any(axis=-1)


def classes_of_coords(cu, cv, w, h):
    """One label per lookup, in this order of precedence: clamped low (pixelID < 0: every channel reads byte 0), clamped high
    (pixelID >= w * h: every channel reads the last byte); then, for indices inside the map: coordU == w (the first texel of the next
    row), coordU elsewhere outside [0, w) (another row's texel), the last texel, the last row, and the interior (everything else)."""
    cu, cv = np.asarray(cu, np.int64), np.asarray(cv, np.int64)
    pixel = cv * w + cu
    out = np.full(pixel.shape, INTERIOR, np.int8)
    out[cv == h - 1] = LAST_ROW
    out[pixel == w * h - 1] = LAST_TEXEL
    out[(cu < 0) | (cu > w)] = WRAP_OTHER
    out[cu == w] = WRAP_ROW
    out[pixel >= w * h] = CLAMPED_HIGH
    out[pixel < 0] = CLAMPED_LOW
    return out


def classes(u, v, w, h, ch=3):
    """(ch does not change the label: with 3 <= ch and c <= 2 the byte index leaves [0, w*h*ch) exactly when pixelID leaves [0, w*h))"""
    cu, cv = coords(u, v, w, h)
    return classes_of_coords(cu, cv, w, h)


def clamped(cls):
    return (cls == CLAMPED_LOW) | (cls == CLAMPED_HIGH)


def lattice(w, h, lo=-0.5, hi=1.5):
    """Every pair of integer coordinates (coordU, coordV) that u, v in [lo, hi] reach on a w x h map, as two flat arrays.  Beyond 2^20
    pairs only the coordinates that the labels distinguish: both ends of the range and the two next to each edge of the map, per axis."""
    ends = [(int(np.trunc(lo * n)), int(np.trunc(hi * n))) for n in (w, h)]
    axes = [np.arange(a, b + 1) for a, b in ends]
    if len(axes[0]) * len(axes[1]) > 1 << 20:
        axes = [np.unique(np.clip([a, -2, -1, 0, 1, n - 2, n - 1, n, n + 1, b], a, b)) for (a, b), n in zip(ends, (w, h))]
    cu, cv = np.meshgrid(*axes)
    return cu.reshape(-1), cv.reshape(-1)


@functools.lru_cache(maxsize=None)
def _admitted(w, h, lo, hi):
    return frozenset(np.unique(classes_of_coords(*lattice(w, h, lo, hi), w, h)).tolist())


def admitted(w, h, lo=-0.5, hi=1.5):
    """The classes a w x h map can show for u, v in [lo, hi]: the lattice, labelled."""
    return set(_admitted(w, h, lo, hi))
