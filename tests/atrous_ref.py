"""float64 restatement of the denoiser's edge-avoiding a-trous filter (include/mi355x_pathtracer.h), written from the
definition and nothing else: tests/test_denoise_cpu.py checks it by hand, tests/test_gpu_denoise.py holds the device to it.

    c = rgb (mean radiance); demodulate: c / max(albedo, 1e-3) per channel on hit pixels
    pass i = 0 .. passes-1, s = 2^i, every hit pixel p:
        out_p = sum_q w_q c_q / sum_q w_q,  q = clamp_to_frame(p + s (dx, dy)), dx, dy in -2..2, miss taps weigh 0,
        w_q = b[dx] b[dy] exp(-|c_p - c_q|^2 / (phi_c 2^-i)) exp(-(|n_p - n_q|^2 / s^2) / phi_n) exp(-|x_p - x_q|^2 / phi_x)
    miss pixels keep c; result = last pass, times max(albedo, 1e-3) on hit pixels when demodulating.
"""
import numpy as np

B3 = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16])


def atrous(rgb, albedo, normal, position, hit, passes, demodulate, phi_color, phi_normal, phi_position):
    """All images (H, W, 3) except hit (H, W); returns (H, W, 3) float64."""
    hit = np.asarray(hit) != 0
    c = np.asarray(rgb, np.float64).copy()
    n = np.asarray(normal, np.float64)
    x = np.asarray(position, np.float64)
    H, W = hit.shape
    f = np.ones_like(c)
    if demodulate:
        f = np.where(hit[..., None], np.maximum(np.asarray(albedo, np.float64), 1e-3), 1.0)
        c = c / f
    ys, xs = np.arange(H), np.arange(W)
    with np.errstate(under="ignore"):
        for i in range(passes):
            s = 2 ** i
            num, den = np.zeros_like(c), np.zeros((H, W))
            for dy in range(-2, 3):
                yy = np.clip(ys + s * dy, 0, H - 1)
                for dx in range(-2, 3):
                    xx = np.clip(xs + s * dx, 0, W - 1)
                    cq, nq, xq, hq = c[yy][:, xx], n[yy][:, xx], x[yy][:, xx], hit[yy][:, xx]
                    wc = np.exp(-((c - cq) ** 2).sum(-1) / (phi_color * 2.0 ** -i))
                    wn = np.exp(-(((n - nq) ** 2).sum(-1) / s ** 2) / phi_normal)
                    wx = np.exp(-((x - xq) ** 2).sum(-1) / phi_position)
                    w = B3[dx + 2] * B3[dy + 2] * wc * wn * wx * hq
                    num += w[..., None] * cq
                    den += w
            c = np.where(hit[..., None], num / np.where(hit, den, 1.0)[..., None], c)
    return c * f


def bspline_atrous(rgb, passes):
    """The same passes with every edge-stopping weight 1 and every pixel a hit: the separable B3-spline a-trous convolution, clamp to
    edge -- a row pass then a column pass per step, written independently of atrous()."""
    c = np.asarray(rgb, np.float64).copy()
    H, W = c.shape[:2]
    for i in range(passes):
        s = 2 ** i
        rows = sum(B3[k + 2] * c[:, np.clip(np.arange(W) + s * k, 0, W - 1)] for k in range(-2, 3))
        c = sum(B3[k + 2] * rows[np.clip(np.arange(H) + s * k, 0, H - 1)] for k in range(-2, 3))
    return c


def random_frame(h, w, seed):
    """Guide images with structure (three planes of normals, a position ramp with steps, 15 % misses) and a noisy colour with
    outliers, the kind of inputs the filter meets -- and a few the renderer never produces (albedo 0, colour 40)."""
    rng = np.random.default_rng(seed)
    normals = np.array([[0, 0, 1], [1, 0, 0], [0, 0.6, 0.8]], np.float32)
    n = normals[rng.integers(0, 3, (h, w))] + rng.normal(0, 0.02, (h, w, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    pos = np.stack([xx * 0.04, yy * 0.04, (xx // 17) * 0.7], -1) + rng.normal(0, 0.01, (h, w, 3))
    alb = rng.random((h, w, 3)).astype(np.float32)
    alb[rng.random((h, w)) < 0.05] = 0.0
    rgb = (rng.random((h, w, 3)) * 1.5).astype(np.float32)
    rgb[rng.random((h, w)) < 0.01] = 40.0
    hit = rng.random((h, w)) > 0.15
    return dict(rgb=rgb, albedo=alb, normal=n.astype(np.float32), position=pos.astype(np.float32), hit=hit)
