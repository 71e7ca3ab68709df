"""float32 conditioning probe of the denoiser: the definitions of tests/atrous_ref.py and tests/variance_ref.py once more, in numpy, with
every intermediate rounded to float32 and the operations in the order pt_denoise.hip performs them (taps row by row, sums accumulated tap
by tap, the per-pass constants formed in double with log2 e folded in and rounded once, exp2 evaluated in double and rounded once).

It is NOT a reference for the device and nothing that ran on a GPU is ever compared with it.  Its one use (tests/test_denoise_grid_cpu.py)
is to measure, for a given case, how far float32 arithmetic alone departs from the float64 restatement: a case in which that distance is a
large part of the bound the device is held to is ill conditioned and cannot tell a wrong kernel from a right one.

Every array below is float32, so every numpy operation on them rounds once to float32; constants enter as float32 arrays or as Python
floats (which numpy keeps at the array's type)."""
import numpy as np

F = np.float32
L2E = 1.4426950408889634
B5 = [1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16]          # exact in float32, and so is every product of two of them
G3 = [0.25, 0.5, 0.25]
FLOOR = F(1e-3)


def _f(a):
    return np.ascontiguousarray(a, F)


def _exp2neg(a):
    """exp2(-a): evaluated in double, rounded once"""
    with np.errstate(under="ignore", over="ignore"):
        return np.exp2(-a.astype(np.float64)).astype(F)


def lum(c):
    return F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1] + F(0.0722) * c[..., 2]


def _sq3(a, b):
    d0, d1, d2 = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return d0 * d0 + d1 * d1 + d2 * d2


def demodulated(rgb, albedo, hit, demodulate):
    """(the filter's input, the factor that takes it back), as k_atrous_prep forms them"""
    c = _f(rgb).copy()
    f = np.ones_like(c)
    if demodulate:
        f = np.where(hit[..., None], np.maximum(_f(albedo), FLOOR), F(1))
        c = c / f
    return c, f


def _constants(i, phi_color, phi_normal, phi_position):
    """pt_atrous_enqueue's kc, kn, kx of pass i: the phi are the floats of ptx_denoise_params, the arithmetic is double"""
    s = float(1 << i)
    pc, pn, px = float(F(phi_color)), float(F(phi_normal)), float(F(phi_position))
    return F(L2E * s / pc), F(L2E / (s * s * pn)), F(L2E / px)


def atrous(rgb, albedo, normal, position, hit, passes, demodulate, phi_color, phi_normal, phi_position):
    hit = np.asarray(hit) != 0
    c, f = demodulated(rgb, albedo, hit, demodulate)
    n, x = _f(normal), _f(position)
    H, W = hit.shape
    ys, xs = np.arange(H), np.arange(W)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(passes):
            s = 1 << i
            kc, kn, kx = _constants(i, phi_color, phi_normal, phi_position)
            num, den = np.zeros_like(c), np.zeros((H, W), F)
            for j in range(5):
                yy = np.clip(ys + (j - 2) * s, 0, H - 1)
                for k in range(5):
                    xx = np.clip(xs + (k - 2) * s, 0, W - 1)
                    cq, hq = c[yy][:, xx], hit[yy][:, xx]
                    e = _sq3(c, cq) * kc + _sq3(n, n[yy][:, xx]) * kn + _sq3(x, x[yy][:, xx]) * kx
                    wt = np.where(hq, F(B5[k] * B5[j]) * _exp2neg(e), F(0))
                    num += wt[..., None] * cq
                    den += wt
            c = np.where(hit[..., None], num / np.where(hit, den, F(1))[..., None], c)
    return c * f


def spatial_variance(col, normal, position, hit, ids=None, radius=3, phi_normal=0.1, phi_position=0.5):
    """k_variance_spatial with count 1: two sweeps, the mean and then the squared deviations"""
    hit = np.asarray(hit) != 0
    col = _f(col)
    l, n, x = lum(col), _f(normal), _f(position)
    H, W = hit.shape
    ys, xs = np.arange(H), np.arange(W)
    kn, kx = F(L2E / float(F(phi_normal))), F(L2E / float(F(phi_position)))
    taps = []
    for dy in range(-radius, radius + 1):
        yy = np.clip(ys + dy, 0, H - 1)
        for dx in range(-radius, radius + 1):
            xx = np.clip(xs + dx, 0, W - 1)
            ok = hit[yy][:, xx]
            if ids is not None:
                ids = np.asarray(ids)
                ok = ok & (ids[yy][:, xx] == ids).all(-1)
            wt = np.where(ok, _exp2neg(_sq3(n, n[yy][:, xx]) * kn + _sq3(x, x[yy][:, xx]) * kx), F(0))
            taps.append((wt, l[yy][:, xx]))
    s0, s1, s2 = (np.zeros((H, W), F) for _ in range(3))
    for wt, lq in taps:
        s0 += wt
        s1 += wt * lq
    s0 = np.where(hit, s0, F(1))
    lbar = s1 / s0
    for wt, lq in taps:
        d = lq - lbar
        s2 += wt * d * d
    return np.where(hit, s2 / s0, F(0))


def atrous_variance(col, var, normal, position, hit, passes=5, phi_luminance=4.0, epsilon=1e-4, prefilter=1, phi_normal=0.1,
                    phi_position=0.5):
    """k_atrous_pass<true, *> on a colour already in the filter's space; returns (colour, variance)"""
    hit = np.asarray(hit) != 0
    c, v = _f(col).copy(), np.where(hit, _f(var), F(0))
    n, x = _f(normal), _f(position)
    H, W = hit.shape
    ys, xs = np.arange(H), np.arange(W)
    pl, eps = F(phi_luminance), F(epsilon)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i in range(passes):
            s = 1 << i
            _, kn, kx = _constants(i, 1.0, phi_normal, phi_position)
            g = v
            if prefilter:
                gs, ks = np.zeros((H, W), F), np.zeros((H, W), F)
                for j in range(3):
                    yy = np.clip(ys + j - 1, 0, H - 1)
                    for k in range(3):
                        xx = np.clip(xs + k - 1, 0, W - 1)
                        kk = np.where(hit[yy][:, xx], F(G3[k] * G3[j]), F(0))
                        gs += kk * v[yy][:, xx]
                        ks += kk
                g = gs / np.where(hit, ks, F(1))
            kl = F(L2E) / (pl * np.sqrt(g) + eps)
            l = lum(c)
            num, nv, den = np.zeros_like(c), np.zeros((H, W), F), np.zeros((H, W), F)
            for j in range(5):
                yy = np.clip(ys + (j - 2) * s, 0, H - 1)
                for k in range(5):
                    xx = np.clip(xs + (k - 2) * s, 0, W - 1)
                    cq, hq = c[yy][:, xx], hit[yy][:, xx]
                    e = np.abs(l - l[yy][:, xx]) * kl + _sq3(n, n[yy][:, xx]) * kn + _sq3(x, x[yy][:, xx]) * kx
                    wt = np.where(hq, F(B5[k] * B5[j]) * _exp2neg(e), F(0))
                    num += wt[..., None] * cq
                    nv += wt * wt * v[yy][:, xx]
                    den += wt
            safe = np.where(hit, den, F(1))
            c = np.where(hit[..., None], num / safe[..., None], c)
            v = np.where(hit, nv / (safe * safe), F(0))
    return c, v


def denoise_buffers_variance(rgb, albedo, normal, position, hit, ids=None, variance=None, passes=5, demodulate=1, phi_normal=0.1,
                             phi_position=0.5, phi_luminance=4.0, epsilon=1e-4, spatial_radius=3, prefilter=1):
    """ptx_denoise_buffers_variance: returns (rgb_out, v_out, v0)"""
    hit = np.asarray(hit) != 0
    col, f = demodulated(rgb, albedo, hit, demodulate)
    if variance is None:
        v0 = spatial_variance(col, normal, position, hit, ids, spatial_radius, phi_normal, phi_position)
    else:
        v0 = np.where(hit, np.maximum(_f(variance), F(0)), F(0))
    c, v = atrous_variance(col, v0, normal, position, hit, passes, phi_luminance, epsilon, prefilter, phi_normal, phi_position)
    return c * f, v, v0
