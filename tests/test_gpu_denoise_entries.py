"""GPU: the denoiser's entry points do not see each other (include/mi355x_pathtracer.h: ptx_denoise, ptx_denoise_temporal,
ptx_denoise_variance, ptx_denoise_measured, ptx_denoise_temporal_measured, ptx_denoise_adaptive).  They share the tracer's G-buffer, the
filter's two colour buffers (whose fourth float is a variance for some and 0 for others), the variance pair and the flags that say what
those hold; what one of them leaves there must not reach the next one's result.  For every ordered pair (X, Y), X's call runs immediately
before Y's on one tracer, at two views, and what Y returns is bit for bit what it returns on a tracer that never ran anything else.  An
identity: the expected values are the library's own, so there is no tolerance."""
import contextlib
import ctypes
import os

import pytest

from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

W, H = 70, 9        # crosses one 64-pixel workgroup column, the height no multiple of 4, three tiles, the last partial
DEPTH = 3
BATCH, ADDS = 2, 2  # 4 spp per view as two adds of 2: with min_batches = 2 the measured paths really run
SPP = BATCH * ADDS

# what each entry point takes: a temporal handle, a moments handle, an adaptive handle (with a moments handle of its own kind of add);
# variance: Tracer.variance() is part of its result.  ptx_denoise_variance is there in both of its forms.
KINDS = {
    "denoise": dict(),
    "temporal": dict(temporal=True),
    "variance": dict(variance=True),
    "variance_temporal": dict(temporal=True, variance=True),
    "measured": dict(moments=True, variance=True),
    "temporal_measured": dict(temporal=True, moments=True, variance=True),
    "adaptive": dict(moments=True, adaptive=True, variance=True),
}
NO_HISTORY = [k for k, v in KINDS.items() if not v.get("temporal")]      # the ones that run with sampled guides


class _Entry:
    """one entry point with handles of its own"""

    def __init__(self, pt, stack, kind):
        self.kind, self.has = kind, KINDS[kind]
        self.tm = stack.enter_context(pt.Temporal(0, W, H)) if self.has.get("temporal") else None
        self.m = stack.enter_context(pt.Moments(0, W, H)) if self.has.get("moments") else None
        self.a = stack.enter_context(pt.Adaptive(0, W, H)) if self.has.get("adaptive") else None

    def camera_step(self):
        """a camera step restarts the accumulation: the moments start again with it, and the counts with them"""
        if self.m:
            self.m.reset()
        if self.a:
            self.a.reset()

    def add(self, T, total):
        if self.a:
            self.a.add(self.m, T, BATCH)                               # every tile active: no select, so no mask
        elif self.m:
            self.m.add(T, total)

    def call(self, T, read):
        k = self.kind
        if k == "denoise":
            return T.denoise(SPP, read=read)
        if k == "temporal":
            return T.denoise_temporal(self.tm, SPP, read=read)
        if k in ("variance", "variance_temporal"):
            return T.denoise_variance(SPP, self.tm, read=read)
        if k in ("measured", "temporal_measured"):
            return T.denoise_measured(self.m, SPP, min_batches=2, read=read, temporal=self.tm)
        return T.denoise_adaptive(self.a, self.m, min_batches=2, read=read)

    def result(self, T):
        """the call, and everything it hands back"""
        out = dict(frame=self.call(T, True))
        if self.has.get("variance"):
            out.update(("variance " + k, v) for k, v in T.variance().items())
        if self.tm:
            out.update(("temporal " + k, v) for k, v in self.tm.read().items())
        return out


def _run(pt, before, kind, guides):
    """`kind` at view A and at a small orbit step B on a fresh tracer, `before` (a kind or None) called right before it each time
    -> kind's results at A and at B"""
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"), res=(W, H), depth=DEPTH)
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))
    out = []
    with contextlib.ExitStack() as stack:
        entries = [_Entry(pt, stack, k) for k in ([before] if before else []) + [kind]]
        T = stack.enter_context(pt.Tracer(s))
        assert T.num_tiles == 3
        if guides:
            T.set_guide_samples(guides)
        for view in range(2):
            if view:
                s.orbit_events(o, [("left", 3.0, 1.0)])
                T.set_camera(s)
                T.reset_image()
                for e in entries:
                    e.camera_step()
            for b in range(ADDS):
                T.render(b * BATCH + 1, BATCH)
                for e in entries:
                    e.add(T, (b + 1) * BATCH)
            for e in entries[:-1]:
                e.call(T, False)
            out.append(entries[-1].result(T))
    return out


_ALONE = {}


def _alone(pt, kind, guides):
    """computed once per kind, read by every pair"""
    key = (kind, guides)
    if key not in _ALONE:
        _ALONE[key] = _run(pt, None, kind, guides)
        a, b = _ALONE[key]
        assert a["frame"].any() and not beq(a["frame"], b["frame"])
        if KINDS[kind].get("variance"):
            assert a["variance input"].any() and b["variance input"].any()
        if KINDS[kind].get("temporal"):
            assert not a["temporal count"].any() and (b["temporal count"] > 0).any()      # view B has a history to take
    return _ALONE[key]


def _check_pairs(pt, kind, others, guides):
    want = _alone(pt, kind, guides)
    for before in others:
        got = _run(pt, before, kind, guides)
        for view, (g, w) in enumerate(zip(got, want)):
            assert sorted(g) == sorted(w)
            for key in w:
                assert beq(g[key], w[key]), "%s after %s, view %s, guides %d: %s differs" % (kind, before, "AB"[view], guides, key)


@pytest.mark.parametrize("kind", list(KINDS))
def test_result_does_not_depend_on_the_entry_point_that_ran_before(gpu_product, kind):
    _check_pairs(gpu_product, kind, list(KINDS), 0)


def test_the_measured_paths_are_not_the_fall_backs(gpu_product):
    """two batches at min_batches = 2: the measured variance is used, so these frames are not ptx_denoise_variance's"""
    pt = gpu_product
    for measured, plain in (("measured", "variance"), ("temporal_measured", "variance_temporal"), ("adaptive", "variance")):
        for m, p in zip(_alone(pt, measured, 0), _alone(pt, plain, 0)):
            assert not beq(m["variance input"], p["variance input"]), measured


@pytest.mark.parametrize("kind", NO_HISTORY)
def test_with_sampled_guides_too(gpu_product, kind):
    """the entry points that carry no history, once more with the guides averaged over two camera rays per pixel"""
    _check_pairs(gpu_product, kind, NO_HISTORY, 2)
