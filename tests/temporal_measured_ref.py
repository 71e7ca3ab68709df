"""float64 restatement of the temporal denoiser that uses the measured sample variance (include/mi355x_pathtracer.h:
ptx_denoise_temporal_measured), composed from the restatements of its parts: temporal_ref.reproject for the taps,
variance_ref.update / temporal_variance for today's rule, moments_ref.quad for the measured variance.  tests/test_temporal_measured_cpu.py
checks it on synthetic samples, tests/test_gpu_temporal_measured.py holds the device to it.

    B = the moments handle's batches; q = max(g^T C g, 0), C = M / (B - 1), g_k = l_k / max(albedo_k, 1e-3)
    B < min_batches: variance_ref.temporal_variance, untouched
    a hit pixel that inherits a V (hist with V, n_h > 0), e, V_h, mu_h as there:
        V_c = ((B - 1) q + e) / B, V = (n_h V_h + spp V_c) / (n_h + spp)
    every other hit pixel: V = q; miss pixels: 0
"""
import numpy as np

from moments_ref import LUM, quad
from temporal_ref import reproject
from variance_ref import lum, temporal_variance


def pooled(V_h, mu_h, n_h, l_c, spp, q, B):
    """variance_ref.update with the current view's share e (one degree of freedom) pooled with q (B - 1 of them)"""
    tot = n_h + spp
    e = (l_c - mu_h) ** 2 * n_h * spp / tot
    V_c = ((B - 1) * q + e) / B
    return (n_h * V_h + spp * V_c) / tot


def measured_q(C, hit, albedo):
    """q (H, W): the per-sample variance of the demodulated luminance from the covariance C (H, W, 3, 3); 0 on miss pixels"""
    hit = np.asarray(hit) != 0
    g = LUM / np.where(hit[..., None], np.maximum(np.asarray(albedo, np.float64), 1e-3), 1.0)
    return np.where(hit, np.maximum(quad(C, g), 0.0), 0.0)


def temporal_measured_variance(prev_cam, cur, prev, spec, c, spp, C, B, min_batches=4, **tparams):
    """V (H, W) as ptx_denoise_temporal_measured leaves it in the state; NaN where the spatial estimate has to supply it (only with
    B < min_batches).  prev: temporal_ref.state(...) of the committed history, with prev["V"] when it carries one, or None; c: rgb / spp;
    C: the moments' covariance (moments_ref.Moments.cov() or from_cov6 of the device's), B its batches."""
    hit = np.asarray(cur["hit"]) != 0
    inherits = prev is not None and "V" in prev
    if B < min_batches:
        return temporal_variance(prev_cam, cur, prev, spec, c, spp, **tparams) if inherits else np.where(hit, np.nan, 0.0)
    q = measured_q(C, hit, cur["albedo"])
    if not inherits:
        return q
    ones = dict(cur, albedo=np.ones_like(np.asarray(cur["albedo"], np.float64)))          # as temporal_variance: sum w X_q / S
    Dh, nh, _ = reproject(prev_cam, ones, prev, spec, **tparams)
    Vh, _, _ = reproject(prev_cam, ones, dict(prev, D=np.repeat(np.asarray(prev["V"], np.float64)[..., None], 3, -1)), spec, **tparams)
    a = np.maximum(np.asarray(cur["albedo"], np.float64), 1e-3)
    V = pooled(Vh[..., 0], lum(Dh), nh, lum(np.asarray(c, np.float64) / a), float(spp), q, float(B))
    return np.where(hit, np.where(nh > 0, V, q), 0.0)


def estimator_samples(h, w, spp=16, views=2, sigma2=0.09, seed=2024):
    """s (views, spp, H, W): iid samples of mean 1 and variance sigma2 (a gamma distribution: positive, as radiance is), seeded.  A pixel
    whose sample j is max(albedo, 1e-3) * s_j has a demodulated luminance of s_j exactly (the Rec. 709 weights sum to 1), so its true
    per-sample variance is sigma2 on every hit pixel."""
    rng = np.random.default_rng(seed)
    return rng.gamma(1.0 / sigma2, sigma2, (views, spp, h, w))


def estimator_figures(V, sigma2):
    """mean of V / sigma2 and the relative RMS error of V"""
    r = np.asarray(V, np.float64).ravel() / sigma2
    return float(r.mean()), float(np.sqrt(((r - 1.0) ** 2).mean()))
