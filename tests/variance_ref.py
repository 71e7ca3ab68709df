"""float64 restatement of the denoiser's variance guidance (include/mi355x_pathtracer.h: ptx_denoise_variance), written from
the definition and nothing else: tests/test_variance_cpu.py checks it by hand, tests/test_gpu_variance.py holds the device to it.

    l(c) = 0.2126 r + 0.7152 g + 0.0722 b, of the filter's input in the filter's colour space (demodulated when demodulate != 0)
    V = per-sample luminance variance (the variance of a mean of n samples is V / n)
    spatial: w_q = exp(-|n_p - n_q|^2 / phi_n) exp(-|x_p - x_q|^2 / phi_x) over the (2r+1)^2 window, hit taps of the same ids, clamped:
        lbar = sum w l_q / sum w, var_s = sum w (l_q - lbar)^2 / sum w;  without history V = n var_s
    temporal: V_h = sum w V_q / S, mu_h = l(sum w D_q / S), l_c = l(c / a):
        e = (l_c - mu_h)^2 n_h spp / (n_h + spp), V = (n_h V_h + spp e) / (n_h + spp)
    filter, pass i, s = 2^i: g_p = 3x3 Gaussian of v over hit taps (renormalised), w_q = b b exp(-|l(c_p) - l(c_q)| / (phi_l sqrt(g_p) + eps))
        x normal term x position term; c_out = sum w c_q / sum w, v_out = sum w^2 v_q / (sum w)^2; miss pixels keep c, v = 0
"""
import numpy as np

from atrous_ref import B3
from temporal_ref import reproject

LUM = np.array([0.2126, 0.7152, 0.0722])
G3 = np.array([0.25, 0.5, 0.25])


def lum(c):
    return np.asarray(c, np.float64) @ LUM


def demodulated(rgb, albedo, hit, demodulate=True):
    """the filter's input in the filter's colour space, and the factor that takes it back"""
    hit = np.asarray(hit) != 0
    c = np.asarray(rgb, np.float64)
    f = np.ones_like(c)
    if demodulate:
        f = np.where(hit[..., None], np.maximum(np.asarray(albedo, np.float64), 1e-3), 1.0)
    return c / f, f


def spatial_variance(col, normal, position, hit, ids=None, radius=3, phi_normal=0.1, phi_position=0.5):
    """var_s (H, W) of l(col); ids: (H, W, 2) of (material, geom) or None (no id test); miss pixels 0"""
    hit = np.asarray(hit) != 0
    l, n, x = lum(col), np.asarray(normal, np.float64), np.asarray(position, np.float64)
    H, W = hit.shape
    ys, xs = np.arange(H), np.arange(W)
    taps = []
    for dy in range(-radius, radius + 1):
        yy = np.clip(ys + dy, 0, H - 1)
        for dx in range(-radius, radius + 1):
            xx = np.clip(xs + dx, 0, W - 1)
            ok = hit[yy][:, xx]
            if ids is not None:
                ids = np.asarray(ids)
                ok = ok & (ids[yy][:, xx] == ids).all(-1)
            w = np.exp(-((n - n[yy][:, xx]) ** 2).sum(-1) / phi_normal) * np.exp(-((x - x[yy][:, xx]) ** 2).sum(-1) / phi_position) * ok
            taps.append((w, l[yy][:, xx]))
    sw = sum(w for w, _ in taps)
    safe = np.where(hit, sw, 1.0)
    lbar = sum(w * lq for w, lq in taps) / safe
    var = sum(w * (lq - lbar) ** 2 for w, lq in taps) / safe
    return np.where(hit, var, 0.0)


def update(V_h, mu_h, n_h, l_c, spp):
    """the pairwise update: per-sample variance of n_h old samples (mean luminance mu_h) joined by a batch of spp (mean l_c)"""
    tot = n_h + spp
    e = (l_c - mu_h) ** 2 * n_h * spp / tot
    return (n_h * V_h + spp * e) / tot


def temporal_variance(prev_cam, cur, prev, spec, c, spp, **tparams):
    """V (H, W) of the pixels that inherit one, NaN where the spatial estimate has to supply it (hit pixels with n_h == 0), 0 on misses.
    prev: temporal_ref.state(...) with prev["V"] (H, W); c: rgb / spp (H, W, 3).  The taps, weights and S are temporal_ref.reproject's:
    with D replaced by V (and by D itself) and the current albedo by 1 it returns sum w V_q / S (and sum w D_q / S)."""
    hit = np.asarray(cur["hit"]) != 0
    ones = dict(cur, albedo=np.ones_like(np.asarray(cur["albedo"], np.float64)))
    Dh, nh, _ = reproject(prev_cam, ones, prev, spec, **tparams)
    Vh, _, _ = reproject(prev_cam, ones, dict(prev, D=np.repeat(np.asarray(prev["V"], np.float64)[..., None], 3, -1)), spec, **tparams)
    a = np.maximum(np.asarray(cur["albedo"], np.float64), 1e-3)
    V = update(Vh[..., 0], lum(Dh), nh, lum(np.asarray(c, np.float64) / a), float(spp))
    return np.where(hit, np.where(nh > 0, V, np.nan), 0.0)


def atrous_variance(col, var, normal, position, hit, passes=5, phi_luminance=4.0, epsilon=1e-4, prefilter=1, phi_normal=0.1,
                    phi_position=0.5):
    """the passes on a colour already in the filter's space: col (H, W, 3), var (H, W) = v0; returns (colour, variance)"""
    hit = np.asarray(hit) != 0
    c, v = np.asarray(col, np.float64).copy(), np.where(hit, np.asarray(var, np.float64), 0.0)
    n, x = np.asarray(normal, np.float64), np.asarray(position, np.float64)
    H, W = hit.shape
    ys, xs = np.arange(H), np.arange(W)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        for i in range(passes):
            s = 2 ** i
            g = v
            if prefilter:
                gs, ks = np.zeros((H, W)), np.zeros((H, W))
                for dy in (-1, 0, 1):
                    yy = np.clip(ys + dy, 0, H - 1)
                    for dx in (-1, 0, 1):
                        xx = np.clip(xs + dx, 0, W - 1)
                        k = G3[dx + 1] * G3[dy + 1] * hit[yy][:, xx]
                        gs += k * v[yy][:, xx]
                        ks += k
                g = gs / np.where(hit, ks, 1.0)
            sigma = phi_luminance * np.sqrt(g) + epsilon
            l = lum(c)
            num, nv, den = np.zeros_like(c), np.zeros((H, W)), np.zeros((H, W))
            for dy in range(-2, 3):
                yy = np.clip(ys + s * dy, 0, H - 1)
                for dx in range(-2, 3):
                    xx = np.clip(xs + s * dx, 0, W - 1)
                    cq, nq, xq, hq = c[yy][:, xx], n[yy][:, xx], x[yy][:, xx], hit[yy][:, xx]
                    wl = np.exp(-np.abs(l - l[yy][:, xx]) / sigma)
                    wn = np.exp(-(((n - nq) ** 2).sum(-1) / s ** 2) / phi_normal)
                    wx = np.exp(-((x - xq) ** 2).sum(-1) / phi_position)
                    w = np.where(hq, B3[dx + 2] * B3[dy + 2] * wl * wn * wx, 0.0)
                    num += w[..., None] * cq
                    nv += w * w * v[yy][:, xx]
                    den += w
            safe = np.where(hit, den, 1.0)
            c = np.where(hit[..., None], num / safe[..., None], c)
            v = np.where(hit, nv / safe ** 2, 0.0)
    return c, v


def denoise_buffers_variance(rgb, albedo, normal, position, hit, ids=None, variance=None, passes=5, demodulate=1, phi_normal=0.1,
                             phi_position=0.5, phi_luminance=4.0, epsilon=1e-4, spatial_radius=3, prefilter=1):
    """ptx_denoise_buffers_variance: returns (rgb_out, v_out, v0)"""
    col, f = demodulated(rgb, albedo, hit, demodulate)
    if variance is None:
        v0 = spatial_variance(col, normal, position, hit, ids, spatial_radius, phi_normal, phi_position)     # n = 1
    else:
        v0 = np.where(np.asarray(hit) != 0, np.maximum(np.asarray(variance, np.float64), 0.0), 0.0)
    c, v = atrous_variance(col, v0, normal, position, hit, passes, phi_luminance, epsilon, prefilter, phi_normal, phi_position)
    return c * f, v, v0
