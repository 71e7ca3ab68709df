"""float64 restatement of the sample moments by batch means (include/mi355x_pathtracer.h: ptx_moments_*), written from the
definition and nothing else: tests/test_moments_cpu.py checks it on synthetic samples, tests/test_gpu_moments.py holds the device to it.

    add with samples_total = N > W: k = N - W, x = (acc - snap) / k, then West's weighted update
        W' = W + k, d = x - mean, mean' = mean + (k / W') d, M' = M + k d (x - mean')^T, B' = B + 1, snap' = acc
    B >= 2: C = M / (B - 1) estimates the per-sample covariance; the variance of the frame's mean of g . colour is g^T C g / W
    summary over the pixels with B >= 2, g = Rec. 709: q = max(g^T C g, 0), se = sqrt(q / W), rel = se / max(l(mean), floor)
    measured v0 of the filter: max(g^T C g, 0) / W with g_k = l_k / max(albedo_k, 1e-3) when demodulating, else l_k, on hit pixels with
        B >= min_batches; the other hit pixels take the spatial estimate, miss pixels 0
"""
import numpy as np

LUM = np.array([0.2126, 0.7152, 0.0722])
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))     # cov6's order: rr, gg, bb, rg, rb, gb


class Moments:
    """the state of one (H, W) frame; add() takes the accumulation buffer as the device sees it (fp32 values, any shape of H*W*3)"""

    def __init__(self, h, w):
        self.h, self.w = h, w
        self.reset()

    def reset(self):
        self.snap = np.zeros((self.h, self.w, 3))
        self.mean = np.zeros((self.h, self.w, 3))
        self.M = np.zeros((self.h, self.w, 3, 3))
        self.W, self.B = 0, 0

    def add(self, acc, samples_total):
        assert samples_total > self.W
        acc = np.asarray(acc, np.float64).reshape(self.h, self.w, 3)
        k = samples_total - self.W
        x = (acc - self.snap) / k
        d = x - self.mean
        self.W += k
        self.mean = self.mean + (k / self.W) * d
        self.M = self.M + k * d[..., :, None] * (x - self.mean)[..., None, :]
        self.B += 1
        self.snap = acc

    def cov(self):
        """C (H, W, 3, 3), symmetrised; zeros while B < 2"""
        if self.B < 2:
            return np.zeros_like(self.M)
        return 0.5 * (self.M + np.swapaxes(self.M, -1, -2)) / (self.B - 1)

    def cov6(self):
        return to_cov6(self.cov())


def to_cov6(C):
    return np.stack([C[..., i, j] for i, j in PAIRS], -1)


def from_cov6(c6):
    c6 = np.asarray(c6, np.float64)
    C = np.zeros(c6.shape[:-1] + (3, 3))
    for n, (i, j) in enumerate(PAIRS):
        C[..., i, j] = C[..., j, i] = c6[..., n]
    return C


def quad(C, g):
    """g^T C g per pixel; g: (3,) or (..., 3)"""
    g = np.broadcast_to(np.asarray(g, np.float64), C.shape[:-1])
    return np.einsum("...i,...ij,...j->...", g, C, g)


def summary(mean, C, batches, samples, floor=0.05, threshold=0.05):
    """ptx_moments_summarize from a state: mean (H, W, 3), C (H, W, 3, 3), batches (H, W) or an int, samples = W.  Also returns the
    per-pixel rel under "rel" (NaN where batches < 2)."""
    mean = np.asarray(mean, np.float64)
    B = np.broadcast_to(np.asarray(batches), mean.shape[:-1])
    use = B >= 2
    q = np.maximum(quad(C, LUM), 0.0)
    rel = np.sqrt(q / max(samples, 1)) / np.maximum(mean @ LUM, floor)
    n = int(use.sum())
    out = dict(pixels=n, pixels_over=int((rel[use] > threshold).sum()), samples=int(samples), batches=int(B.max()) if B.size else 0,
               mean_rel_se=0.0, rms_rel_se=0.0, max_rel_se=0.0, mean_variance=0.0, rel=np.where(use, rel, np.nan))
    if n:
        out.update(mean_rel_se=float(rel[use].mean()), rms_rel_se=float(np.sqrt((rel[use] ** 2).mean())), max_rel_se=float(rel[use].max()),
                   mean_variance=float(q[use].mean()))
    return out


def measured_v0(C, samples, batches, hit, albedo=None, demodulate=1, min_batches=4):
    """the filter's input variance (H, W): NaN on the hit pixels that fall back to the spatial estimate, 0 on miss pixels"""
    hit = np.asarray(hit) != 0
    g = np.broadcast_to(LUM, C.shape[:-1])
    if demodulate:
        g = g / np.where(hit[..., None], np.maximum(np.asarray(albedo, np.float64), 1e-3), 1.0)
    v = np.maximum(quad(C, g), 0.0) / max(samples, 1)
    B = np.broadcast_to(np.asarray(batches), hit.shape)
    return np.where(hit, np.where(B >= min_batches, v, np.nan), 0.0)
