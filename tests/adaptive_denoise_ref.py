"""float64 restatement of the variance-guided filter on an adaptively sampled frame (include/mi355x_pathtracer.h: ptx_denoise_adaptive,
DESIGN.md 10), composed from the restatements of its parts and nothing else: tests/test_adaptive_denoise_cpu.py checks it by hand,
tests/test_gpu_adaptive_denoise.py holds the device to it.

    tile = (y W + x) // tile_px, s = samples[tile]: c = acc / s, the frame normalised tile by tile (adaptive_ref.resolve's)
    v0 on a hit pixel with B >= min_batches: max(g^T C g, 0) / W, moments_ref.measured_v0's with the pixel's own W (= s) and B
    v0 on the other hit pixels: variance_ref.spatial_variance of the demodulated c; 0 on miss pixels
    then variance_ref.atrous_variance, multiplied back by max(albedo, 1e-3) when demodulating
"""
import numpy as np

from adaptive_ref import tile_of
from moments_ref import LUM, quad
from variance_ref import atrous_variance, demodulated, spatial_variance


def measured_v0_pixels(C, samples, batches, hit, albedo=None, demodulate=1, min_batches=4):
    """moments_ref.measured_v0 with samples (W) and batches (B) per pixel, (H, W) each: NaN on the hit pixels that fall back to the
    spatial estimate, 0 on miss pixels"""
    hit = np.asarray(hit) != 0
    g = np.broadcast_to(LUM, C.shape[:-1])
    if demodulate:
        g = g / np.where(hit[..., None], np.maximum(np.asarray(albedo, np.float64), 1e-3), 1.0)
    W = np.maximum(np.broadcast_to(np.asarray(samples, np.float64), hit.shape), 1.0)
    v = np.maximum(quad(C, g), 0.0) / W
    B = np.broadcast_to(np.asarray(batches), hit.shape)
    return np.where(hit, np.where(B >= min_batches, v, np.nan), 0.0)


def normalised(acc, tile_samples, h, w, tile_px):
    """(H, W, 3) float64: acc over the samples of the pixel's tile (every tile holds some)"""
    s = np.asarray(tile_samples, np.float64)[tile_of(h, w, tile_px)]
    assert (s > 0).all()
    return np.asarray(acc, np.float64).reshape(h, w, 3) / s[..., None], s


def denoise_adaptive(acc, tile_samples, C, batches, albedo, normal, position, hit, ids=None, tile_px=256, min_batches=4, passes=5,
                     demodulate=1, phi_normal=0.1, phi_position=0.5, phi_luminance=4.0, epsilon=1e-4, spatial_radius=3, prefilter=1):
    """ptx_denoise_adaptive: acc (H, W, 3) sums, tile_samples (tiles,), C (H, W, 3, 3) and batches (H, W) of the moments state.
    Returns (rgb_out, v_out, v0, fallback) -- fallback (H, W) bool: the hit pixels whose v0 is the spatial estimate"""
    hit = np.asarray(hit) != 0
    h, w = hit.shape
    c, s = normalised(acc, tile_samples, h, w, tile_px)
    col, f = demodulated(c, albedo, hit, demodulate)
    v0 = measured_v0_pixels(C, s, batches, hit, albedo, demodulate, min_batches)
    fallback = np.isnan(v0)
    if fallback.any():
        v0 = np.where(fallback, spatial_variance(col, normal, position, hit, ids, spatial_radius, phi_normal, phi_position), v0)
    out, v = atrous_variance(col, v0, normal, position, hit, passes, phi_luminance, epsilon, prefilter, phi_normal, phi_position)
    return out * f, v, v0, fallback
