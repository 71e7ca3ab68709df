"""float64 restatement of adaptive sampling by tiles (include/mi355x_pathtracer.h: ptx_set_active_tiles, ptx_moments_add_host_tiled,
ptx_adaptive_*), written from the definition and nothing else: tests/test_adaptive_cpu.py checks it on synthetic samples,
tests/test_gpu_adaptive.py holds the device to it.

    tile = (y W + x) // tile_px; a tiled add gives every tile its own samples_total: a tile whose total did not move is idle and keeps
        its state, the others take moments_ref's add with their own (k, total) on their own pixels
    per pixel with B >= 2: rel = sqrt(max(g^T C g, 0) / W) / max(l(mean), floor), g = Rec. 709 (moments_ref.summary's)
    e_T = sqrt(sum rel^2 / n_T), n_T = the tile's pixels inside the frame; no pixel with B >= 2: no estimate, e_T reads 0
    active_T = samples_T < max_samples and (batches_T < min_batches or e_T > target)
    resolve: acc / samples of the pixel's tile, 0 where that is 0
"""
import numpy as np

from moments_ref import LUM, Moments, quad


def num_tiles(h, w, tile_px):
    return (h * w + tile_px - 1) // tile_px


def tile_of(h, w, tile_px):
    """(H, W) int: every pixel's tile"""
    return (np.arange(h * w) // tile_px).reshape(h, w)


def tile_sizes(h, w, tile_px):
    return np.bincount(tile_of(h, w, tile_px).ravel(), minlength=num_tiles(h, w, tile_px))


class TiledMoments:
    """moments_ref.Moments per tile: tile t's pixels as a (1, n_t) frame with its own (k, total) sequence"""

    def __init__(self, h, w, tile_px):
        self.h, self.w, self.tile_px = h, w, tile_px
        self.tile = tile_of(h, w, tile_px).ravel()
        self.n = num_tiles(h, w, tile_px)
        self.idx = [np.flatnonzero(self.tile == t) for t in range(self.n)]
        self.reset()

    def reset(self):
        self.m = [Moments(1, len(i)) for i in self.idx]

    def add(self, acc, tile_samples):
        acc = np.asarray(acc, np.float64).reshape(self.h * self.w, 3)
        for t, m in enumerate(self.m):
            total = int(tile_samples[t])
            assert total >= m.W
            if total > m.W:
                m.add(acc[self.idx[t]], total)

    def _gather(self, f, tail):
        out = np.zeros((self.h * self.w,) + tail)
        for t, m in enumerate(self.m):
            out[self.idx[t]] = f(m).reshape((-1,) + tail)
        return out.reshape((self.h, self.w) + tail)

    @property
    def mean(self):
        return self._gather(lambda m: m.mean, (3,))

    def cov(self):
        return self._gather(lambda m: m.cov(), (3, 3))

    @property
    def W(self):
        """(tiles,) samples per tile"""
        return np.array([m.W for m in self.m], np.int64)

    @property
    def B(self):
        return np.array([m.B for m in self.m], np.int64)

    def W_pixels(self):
        return self.W[self.tile].reshape(self.h, self.w)

    def B_pixels(self):
        return self.B[self.tile].reshape(self.h, self.w)


def pixel_rel(mean, C, batches, samples, floor=0.05):
    """(H, W) rel, NaN where batches < 2; batches and samples per pixel"""
    mean = np.asarray(mean, np.float64)
    B = np.broadcast_to(np.asarray(batches), mean.shape[:-1])
    W = np.maximum(np.broadcast_to(np.asarray(samples, np.float64), mean.shape[:-1]), 1.0)
    rel = np.sqrt(np.maximum(quad(C, LUM), 0.0) / W) / np.maximum(mean @ LUM, floor)
    return np.where(B >= 2, rel, np.nan)


def tile_error(rel, tile_px):
    """(e_T per tile, has-an-estimate per tile) from the per-pixel rel (NaN = no estimate)"""
    h, w = rel.shape
    tile, n_t = tile_of(h, w, tile_px).ravel(), tile_sizes(h, w, tile_px)
    r = rel.ravel()
    ok = ~np.isnan(r)
    s2 = np.bincount(tile[ok], weights=r[ok] ** 2, minlength=len(n_t))
    has = np.bincount(tile[ok], minlength=len(n_t)) > 0
    return np.where(has, np.sqrt(s2 / n_t), 0.0), has


def decide(samples, batches, e, target=0.02, min_batches=4, max_samples=1 << 20):
    samples, batches, e = np.asarray(samples), np.asarray(batches), np.asarray(e, np.float64)
    return (samples < max_samples) & ((batches < min_batches) | (e > target))


def status(samples, active, e, has, h, w, tile_px, rounds):
    n_t = tile_sizes(h, w, tile_px)
    samples, active = np.asarray(samples, np.int64), np.asarray(active, bool)
    return dict(samples_total=int((samples * n_t).sum()), pixels_active=int(n_t[active].sum()), tiles=len(n_t), tiles_active=int(active.sum()),
                samples_min=int(samples.min()), samples_max=int(samples.max()), worst_error=float(np.max(np.where(has, e, 0.0))), rounds=rounds)


def resolve(acc, samples, h, w, tile_px):
    """fp32, as the device: acc / float32(samples of the pixel's tile), 0 where that is 0"""
    s = np.asarray(samples)[tile_of(h, w, tile_px)].astype(np.float32)[..., None]
    acc = np.asarray(acc, np.float32).reshape(h, w, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, acc / s, np.float32(0)).astype(np.float32)
