"""float32 probe of k_moments_add's arithmetic (pt_moments.hip), operation for operation in numpy: every intermediate is a float32, the
operations come in the kernel's order, and the fma's residual of a product p = fl(a b) is float32(float64(a) float64(b) - p), which is
exact (a 48-bit product, and a residual that fp32 holds).  k and the total may differ per pixel, as in k_moments_add_tiled, whose
update is the same; a pixel with k = 0 is idle and keeps its state.

As tests/temporal_f32.py, it is NOT a reference for the device and nothing that ran on a GPU is ever compared with it.  Its one use
(tests/test_moments_grid_cpu.py) is to measure how far float32 arithmetic alone departs from the float64 restatement on the cases of
tests/momentscases.py -- and, with naive=True, how far the form the kernel was written to avoid departs:
d = fl(fl(acc - snap) / k - mean), D = d k W."""
import numpy as np

F = np.float32
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def fma_residual(a, b, p):
    """fmaf(a, b, -p) for p = fl(a b)"""
    return (a.astype(np.float64) * b.astype(np.float64) - p.astype(np.float64)).astype(F)


class Probe:
    def __init__(self, h, w, naive=False):
        self.h, self.w, self.naive = h, w, naive
        self.snap = np.zeros((h, w, 3), F)
        self.W = np.zeros((h, w), F)
        self.mean = np.zeros((h, w, 3), F)
        self.B = np.zeros((h, w), F)
        self.M = np.zeros((h, w, 6), F)
        self.term_finite = True                          # every D_i D_j / den so far was finite

    def add(self, acc, k, total):
        """k, total: the batch's samples and the new W, scalars or (H, W)"""
        acc = np.ascontiguousarray(acc, F).reshape(self.h, self.w, 3)
        k = np.broadcast_to(np.asarray(k, np.float64).astype(F), (self.h, self.w))
        total = np.broadcast_to(np.asarray(total, np.float64).astype(F), (self.h, self.w))
        live = k > 0
        wo = (total - k).astype(F)
        later = live & (wo > 0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            kw = (k * wo).astype(F)
            den = (kw * total).astype(F)
            r = (k / total).astype(F)
            kk, ww, tt = k[..., None], wo[..., None], total[..., None]
            if self.naive:
                d = (((acc - self.snap).astype(F) / kk).astype(F) - self.mean).astype(F)
                D = (d * kw[..., None]).astype(F)
            else:
                p1, p2 = (acc * ww).astype(F), (self.snap * tt).astype(F)
                D = ((p1 - p2).astype(F) + (fma_residual(acc, ww, p1) - fma_residual(self.snap, tt, p2)).astype(F)).astype(F)
            mean = (self.mean + (r[..., None] * (D / kw[..., None]).astype(F)).astype(F)).astype(F)
            terms = np.stack([((D[..., i] * D[..., j]).astype(F) / den).astype(F) for i, j in PAIRS], -1)
            M = (self.M + terms).astype(F)
            first = (acc / kk).astype(F)
        self.term_finite = self.term_finite and bool(np.isfinite(terms[later]).all())
        self.mean = np.where(later[..., None], mean, np.where(live[..., None], first, self.mean)).astype(F)
        self.M = np.where(later[..., None], M, self.M).astype(F)
        self.B = np.where(live, self.B + F(1), self.B).astype(F)
        self.snap = np.where(live[..., None], acc, self.snap).astype(F)
        self.W = np.where(live, total, self.W).astype(F)

    def cov6(self):
        """ptx_moments_read's: M / (B - 1) in float32, 0 where B < 2"""
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (self.M / (self.B - F(1))[..., None]).astype(F)
        return np.where((self.B >= 2)[..., None], c, F(0)).astype(F)


def quad_form(g, M6, B):
    """pt_denoise.h's quad_form on the scatter matrix, float32: g (3,) or (H, W, 3)"""
    g = np.broadcast_to(np.asarray(g, np.float64).astype(F), M6.shape[:-1] + (3,))
    g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
    diag = g0 * g0 * M6[..., 0] + g1 * g1 * M6[..., 1] + g2 * g2 * M6[..., 2]
    off = g0 * g1 * M6[..., 3] + g0 * g2 * M6[..., 4] + g1 * g2 * M6[..., 5]
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((diag + F(2) * off) / (B - F(1))).astype(F)
