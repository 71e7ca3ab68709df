"""CPU: the denoiser's parameter grid (tests/denoisecases.py) before it goes to the device (tests/test_gpu_denoise_grid.py).

Conditioning: for every case the float32 probe (tests/denoise_f32.py) stays within TOL / 4 = 2.5e-5 of the float64 restatement, in the
GPU suites' metric |got - ref| / (|ref| + 1e-3), so float32 arithmetic alone leaves a fourfold margin under the device's bound and a case
that fails there points at the kernel or at the restatement.  Worst probe error per family (153 cases):

    plain 3.8e-6     given variance 1.8e-5     spatial estimate 2.2e-5

The ill-conditioned corner (prefilter = 0 or phi_luminance < 1, where sigma = phi_luminance sqrt(g) + epsilon can reach 0) carries a given
variance with phi_luminance sqrt(v0) >= SIGMA_FLOOR = 1.  The probe figures behind that floor, worst over the grid's 15 such cases on
random_frame / on tame_frame: a variance with exact zeros 8.2e-5 / 3.3e-4; floored at v0 >= 1e-3 3.2e-5 / 5.2e-5 (both over TOL / 4);
floored at phi_luminance sqrt(v0) >= 0.126 (v0 >= 1e-3 at the default phi_luminance) 2.1e-5 / 2.5e-5, >= 0.25 1.7e-5 / 2.2e-5,
>= 0.5 1.6e-5 / 1.6e-5, >= 1 1.3e-5 / 1.7e-5, >= 2 8.1e-6 / 1.1e-5.  What is left at the floor of 1 comes from the later passes, which
shrink v whatever went in.

Coverage: every parameter value, shape and hit mask of the grid still occurs after that tuning.  Hand checks: the restatements where the
grid uses them for the first time (passes 6 .. 10, steps beyond the frame, radius 1, prefilter = 0)."""
import numpy as np
import pytest

import denoise_f32 as probe
import denoisecases as D
from atrous_ref import B3, atrous, bspline_atrous, random_frame
from variance_ref import atrous_variance, spatial_variance

TOL = 1e-4                      # the bound of tests/test_gpu_denoise*.py and tests/test_gpu_variance.py


def _err(got, ref):
    ref = np.asarray(ref, np.float64)
    e = np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + 1e-3)
    return float(e.max()) if e.size else 0.0


@pytest.mark.parametrize("family", ["plain", "given", "spatial"])
def test_every_case_is_well_conditioned(family):
    worst, bad = (0.0, None), []
    for c in D.of_family(family):
        args, ids, var, rc, rv = D.reference(c)
        if family == "plain":
            e = _err(probe.atrous(*args, **c.params), rc)
        else:
            pc, pv, _ = probe.denoise_buffers_variance(*args, ids=ids, variance=var, **c.params)
            e = max(_err(pc, rc), _err(pv, rv))
        worst = max(worst, (e, c.id))
        if not e <= TOL / 4:
            bad.append((c.id, e))
    print("%s: %d cases, worst float32 probe error %.3g (%s)" % (family, len(D.of_family(family)), worst[0], worst[1]))
    assert not bad, bad


def test_the_grid_covers_every_value_shape_and_mask():
    cs = D.CASES
    assert len(cs) <= 155 and max(h * w for h, w in D.SHAPES) <= 7000
    var = [c for c in cs if c.family != "plain"]
    for k, values in D.VALUES.items():
        pool = [c for c in cs if k in c.params] if k != "spatial_radius" else D.of_family("spatial")
        for v in values:
            assert any(c.params[k] == (D.f32(v) if isinstance(v, float) else v) for c in pool), (k, v)
    for fam in ("plain", "given", "spatial"):
        for s in D.SHAPES:
            assert any(c.shape == s for c in D.of_family(fam)), (fam, s)
        for s in D.MASK_SHAPES:
            for m in D.MASKS:
                assert any(c.shape == s and c.mask == m for c in D.of_family(fam)), (fam, s, m)
        for p in (6, 8, 10):
            assert any(c.params["passes"] == p for c in D.of_family(fam)), (fam, p)
    # the steps whose taps stay inside the frame on the shapes made for them
    for s, p in (((9, 130), 6), ((3, 1100), 9), ((2, 2100), 10)):
        assert s[1] > 2 * 2 ** (p - 1) and any(c.shape == s and c.params["passes"] == p for c in D.of_family("plain")), (s, p)
        assert any(c.shape == s and c.params["passes"] == p for c in D.of_family("given")), (s, p)
    sp = D.of_family("spatial")
    assert any(c.ids for c in sp) and any(not c.ids for c in sp)
    for r in (1, 2, 3):
        assert any(c.params["spatial_radius"] == r and c.shape in D.MULTI_TILE and c.mask == "random" for c in sp), r
        assert any(c.params["spatial_radius"] == r and c.params["passes"] == 1 and c.params["prefilter"] == 1 and c.ids == i
                   for c in sp for i in (False, True)), r
    for fam in ("given", "spatial"):
        assert any(c.params["prefilter"] == 0 and c.shape in D.MULTI_TILE for c in D.of_family(fam)), fam
        assert any(c.params["phi_luminance"] < 1 and c.shape in D.MULTI_TILE for c in D.of_family(fam)), fam
    # exact zeros in the given variance stay where they are well conditioned
    assert any((D.reference(c)[2] == 0).any() for c in D.of_family("given") if c.params["prefilter"] == 1)
    # and the ill-conditioned corner is built as the module says
    for c in var:
        if c.sensitive:
            assert c.tame, c.id
            if c.family == "given":
                args, _, v0, _, _ = D.reference(c)
                assert c.params["phi_luminance"] * np.sqrt(v0.min()) >= D.SIGMA_FLOOR * (1 - 1e-6), c.id


def test_masks_are_what_their_names_say():
    for h, w in D.MASK_SHAPES:
        m = {n: D.mask(n, h, w, 0) for n in D.MASKS[1:]}
        assert m["all_hit"].all() and not m["all_miss"].any() and m["single"].sum() == 1
        assert m["checker"].sum() in (h * w // 2, (h * w + 1) // 2) and not (m["checker"][:, 1:] & m["checker"][:, :-1]).any()
        assert not m["hole_tile"][:4, :64].any() and m["hole_tile"][4, :64].all() and m["hole_tile"][:4, 64].all()
        ty, tx = np.mgrid[0:h, 0:w]
        last = (ty // 4 == (h - 1) // 4) & (tx // 64 == (w - 1) // 64)
        assert np.array_equal(m["last_tile"], last) and 0 < last.sum() < 64 * 4


# --- hand checks of the restatements where the grid uses them for the first time ---------------------------------------------------------

HUGE = 1e30


@pytest.mark.parametrize("passes", [6, 7, 8, 9, 10])
def test_deep_passes_without_edge_stopping_are_the_bspline_convolution(passes):
    h, w = 9, 130
    f = random_frame(h, w, 5)
    hit = np.ones((h, w), bool)
    want = bspline_atrous(f["rgb"], passes)
    got = atrous(f["rgb"], f["albedo"], f["normal"], f["position"], hit, passes, 0, HUGE, HUGE, HUGE)
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    gv, _ = atrous_variance(f["rgb"], np.full((h, w), 0.2), f["normal"], f["position"], hit, passes, HUGE, 1e-4, 1, HUGE, HUGE)
    assert np.allclose(gv, want, rtol=1e-12, atol=0)
    # (and the probe agrees to float32)
    assert _err(probe.atrous(f["rgb"], f["albedo"], f["normal"], f["position"], hit, passes, 0, HUGE, HUGE, HUGE), want) <= 1e-5


def _border_pass(c, v, n, x, hit, i, colour_term):
    """one pass at a step no smaller than the frame, written for that case alone: a tap off the centre row is the first or the last
    row, off the centre column the first or the last column.  colour_term(p, q) is the exponent's colour part."""
    H, W = hit.shape
    s = 2.0 ** i
    rows = lambda y: [(0, B3[0] + B3[1]), (y, B3[2]), (H - 1, B3[3] + B3[4])]
    cols = lambda xx: [(0, B3[0] + B3[1]), (xx, B3[2]), (W - 1, B3[3] + B3[4])]
    out, vout = c.copy(), np.zeros((H, W))
    for y in range(H):
        for xx in range(W):
            if not hit[y, xx]:
                continue
            num, nv, den = np.zeros(3), 0.0, 0.0
            for qy, by in rows(y):
                for qx, bx in cols(xx):
                    if not hit[qy, qx]:
                        continue
                    # (the five taps of a side fall on one pixel: their weights differ only in b, which therefore adds up -- but the
                    # variance sums w^2, so it is taken tap by tap)
                    e = np.exp(-colour_term((y, xx), (qy, qx)) - ((n[y, xx] - n[qy, qx]) ** 2).sum() / s ** 2 / PHI_N
                               - ((x[y, xx] - x[qy, qx]) ** 2).sum() / PHI_X)
                    num += by * bx * e * c[qy, qx]
                    den += by * bx * e
                    for b1 in ([B3[0], B3[1]] if by != B3[2] else [B3[2]]):
                        for b2 in ([B3[0], B3[1]] if bx != B3[2] else [B3[2]]):
                            nv += (b1 * b2 * e) ** 2 * v[qy, qx]
            out[y, xx], vout[y, xx] = num / den, nv / den ** 2
    return out, vout


PHI_N, PHI_X = 0.7, 3.0


@pytest.mark.parametrize("passes", [4, 6, 8, 10])
def test_a_step_beyond_the_frame_reads_only_border_pixels(passes):
    h, w = 5, 7                                          # the last pass's step, 2^(passes-1) >= 8, exceeds both
    f = random_frame(h, w, 9)
    f["hit"][0, 0] = f["hit"][h - 1, w - 1] = True
    f["hit"][0, w - 1] = False
    n, x, hit = f["normal"].astype(np.float64), f["position"].astype(np.float64) * 10, f["hit"]
    i = passes - 1
    # the plain filter: the last pass, from the restatement's own result of the passes before it
    before = atrous(f["rgb"], None, n, x, hit, passes - 1, 0, 2.0, PHI_N, PHI_X)
    want, _ = _border_pass(before, np.zeros((h, w)), n, x, hit, i, lambda p, q: ((before[p] - before[q]) ** 2).sum() / (2.0 * 2.0 ** -i))
    assert np.allclose(atrous(f["rgb"], None, n, x, hit, passes, 0, 2.0, PHI_N, PHI_X), want, rtol=1e-12, atol=0)
    # the variance-guided one, without the prefilter
    v0 = np.where(hit, 0.05 + np.random.default_rng(3).random((h, w)), 0.0)
    cb, vb = atrous_variance(f["rgb"], v0, n, x, hit, passes - 1, 2.0, 1e-2, 0, PHI_N, PHI_X)
    lb = cb @ np.array([0.2126, 0.7152, 0.0722])
    want, want_v = _border_pass(cb, vb, n, x, hit, i, lambda p, q: abs(lb[p] - lb[q]) / (2.0 * np.sqrt(vb[p]) + 1e-2))
    got, got_v = atrous_variance(f["rgb"], v0, n, x, hit, passes, 2.0, 1e-2, 0, PHI_N, PHI_X)
    assert np.allclose(got, want, rtol=1e-12, atol=0) and np.allclose(got_v, want_v, rtol=1e-12, atol=0)
    assert (got_v[hit] > 0).all() and not got_v[~hit].any()


def test_radius_one_on_equal_guides_is_the_population_variance_of_the_clamped_window():
    l = np.array([[0.1, 0.9, 0.4], [2.0, 0.3, 0.7], [0.5, 1.1, 0.05]])
    col = np.repeat(l[..., None], 3, -1)                 # the luminance weights add up to 1
    n = np.zeros((3, 3, 3)); n[..., 2] = 1.0
    got = spatial_variance(col, n, np.zeros((3, 3, 3)), np.ones((3, 3), bool), None, 1)
    for y in range(3):
        for x in range(3):
            win = [l[min(max(y + dy, 0), 2), min(max(x + dx, 0), 2)] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
            assert np.isclose(got[y, x], np.var(win), rtol=1e-13, atol=0), (y, x)
    assert np.isclose(got[1, 1], np.var(l), rtol=1e-13, atol=0)
    # the same through the probe, to float32; and a miss in the window or another id leaves the window
    assert _err(probe.spatial_variance(col, n, np.zeros((3, 3, 3)), np.ones((3, 3), bool), None, 1), got) <= 1e-5
    hit = np.ones((3, 3), bool); hit[0, 0] = False
    ids = np.zeros((3, 3, 2), int); ids[2, 2] = (0, 1)
    rest = [l[y, x] for y in range(3) for x in range(3) if (y, x) not in ((0, 0), (2, 2))]
    assert np.isclose(spatial_variance(col, n, np.zeros((3, 3, 3)), hit, ids, 1)[1, 1], np.var(rest), rtol=1e-13, atol=0)


def test_the_prefilter_of_a_constant_variance_changes_nothing():
    h, w = 9, 70
    f = random_frame(h, w, 21)
    v0 = np.full((h, w), 0.37)
    col = f["rgb"].astype(np.float64)
    a = atrous_variance(col, v0, f["normal"], f["position"], f["hit"], passes=1, prefilter=0)
    b = atrous_variance(col, v0, f["normal"], f["position"], f["hit"], passes=1, prefilter=1)
    assert np.allclose(a[0], b[0], rtol=1e-12, atol=0) and np.allclose(a[1], b[1], rtol=1e-12, atol=0)
    # with a variance that is not constant the two differ: the switch is wired
    v1 = v0 + np.random.default_rng(1).random((h, w))
    a = atrous_variance(col, v1, f["normal"], f["position"], f["hit"], passes=1, prefilter=0)
    b = atrous_variance(col, v1, f["normal"], f["position"], f["hit"], passes=1, prefilter=1)
    assert _err(a[0], b[0]) > 1e-3
    pa = probe.atrous_variance(col, v0, f["normal"], f["position"], f["hit"], passes=1, prefilter=0)
    pb = probe.atrous_variance(col, v0, f["normal"], f["position"], f["hit"], passes=1, prefilter=1)
    assert _err(pa[0], pb[0]) <= 1e-5 and _err(pa[1], pb[1]) <= 1e-5
