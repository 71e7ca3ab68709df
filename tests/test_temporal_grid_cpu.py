"""CPU: the reprojection's parameter grid (tests/temporalcases.py) before it goes to the device (tests/test_gpu_temporal_grid.py).

Conditioning: for every case and each of the three kernels the float32 probe (tests/temporal_f32.py) stays within TOL / 4 = 2.5e-5 of
the float64 restatements (temporal_ref.reproject and mix, variance_ref.temporal_variance, temporal_measured_ref.
temporal_measured_variance) in the GPU suites' metric |got - ref| / (|ref| + 1e-3), on the pixels `near` does not exclude, and `near`
excludes 2 % of a case's hit pixels at the most.  So float32 arithmetic alone leaves a fourfold margin under the device's bound, and a
case that fails there points at the kernel or at a restatement.  Worst probe error per variant (100 cases each): plain 7.0e-6, variance
2.1e-5 (the fp32 weights of V_h under (l_c - mu_h)^2), measured 7.0e-6; largest `near` share 0.7 % (the pan that loses a third of the
frame).  What the tuning took: a dolly of exactly 10 % put every ninth column on an integer u (7.7 % near) and became 9.3 %; hist's
displaced strip was moved off the rows the "single" and "last_tile" masks hit.

Coverage: each case reaches what it is for -- inheriting and non-inheriting hit pixels, a binding max_history, taps on all four edges
of hist's frame, specular pixels, taps the normal and the plane test reject beside taps they accept, a third of the frame lost, the
cameras that leave no projection, the thresholds met exactly, the poisoned pixels.  Then the argument refusals of ptx_kat_reproject,
which come before it looks for a device."""
import ctypes

import numpy as np
import pytest

import temporal_f32 as probe
import temporalcases as TC

TOL = 1e-4                      # the bound of tests/test_gpu_denoise_grid.py and tests/test_gpu_temporal_grid.py
NEAR_CAP = 0.02


def _err(got, ref):
    ref = np.asarray(ref, np.float64)
    e = np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + 1e-3)
    return float(e.max()) if e.size else 0.0


def _probe(c, r, variant):
    return probe.reproject(r["cur"], r["rgb"], c.params["spp"], TC.SPEC, r["hist_cam"], r["prev"], variant=variant,
                           has_v=bool(c.params["has_v"]), scatter=r["scatter"], batches=c.params["batches"], **c.tparams)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_every_case_is_well_conditioned(variant):
    worst, bad = (0.0, ""), []
    for c in TC.of_variant(variant):
        r = TC.reference(c)
        p = _probe(c, r, variant)
        keep = ~r["near"]
        e = max(_err(p[k][keep], r[k][keep]) for k in ("h", "nh", "mix", "n", "D"))
        if variant:
            want = r["V1"] if variant == 1 else r["V2"]
            has = keep & np.isfinite(want)
            e = max(e, _err(p["V"][has], want[has]))
            if not (p["V"][keep & ~np.isfinite(want)] == -1).all():
                bad.append((c.id, "V where the spatial estimate is due"))
        elif p["V"].any():
            bad.append((c.id, "V in variant 0"))
        worst = max(worst, (e, c.id))
        if not e <= TOL / 4:
            bad.append((c.id, e))
    print("variant %d: %d cases, worst float32 probe error %.3g (%s)" % (variant, len(TC.of_variant(variant)), worst[0], worst[1]))
    assert not bad, bad


def test_near_excludes_two_percent_at_the_most():
    worst = (0.0, "")
    for c in TC.CASES:
        r = TC.reference(c)
        hit = r["cur"]["hit"]
        frac = r["near"].sum() / max(int(hit.sum()), 1)
        worst = max(worst, (frac, c.id))
        # (a frame of a few hit pixels: one pixel is more than 2 % of it)
        assert frac <= NEAR_CAP or r["near"].sum() <= 1, (c.id, frac)
    print("largest near fraction %.3g (%s)" % worst)


def _first(**want):
    for c in TC.CASES:
        if all(getattr(c, k, None) == v or c.params.get(k) == v for k, v in want.items()):
            return c
    raise AssertionError(want)


def test_the_grid_covers_every_value_shape_mask_and_camera():
    cs = TC.CASES
    assert len(cs) <= 110 and max(h * w for h, w in TC.SHAPES) <= 2000 and max(w for _, w in TC.SHAPES) <= 260
    assert TC.SHAPES == [(1, 1), (3, 63), (4, 64), (5, 65), (8, 128), (9, 130), (70, 2), (6, 257)]
    for k, values in TC.VALUES.items():
        for v in values:
            v = TC.f32(v) if isinstance(v, float) else v
            assert any(c.params[k] == v and c.shape == TC.BASE and c.camera == "pan" for c in cs), (k, v)
            # one at a time around the defaults
            assert any(c.params[k] == v and all(c.params[o] == _first(shape=TC.BASE).params[o] for o in c.params if o != k)
                       for c in cs if c.shape == TC.BASE), (k, v)
    for s in TC.SHAPES:
        assert any(c.shape == s and c.camera == "pan" for c in cs) and any(c.shape == s and c.camera == "subpixel" for c in cs), s
    for s in TC.MASK_SHAPES:
        for m in TC.MASK_PAIRS:
            assert any(c.shape == s and c.masks == m for c in cs), (s, m)
    for side in (0, 1):
        assert {m[side] for m in TC.MASK_PAIRS} == set(TC.MASKS)
    for cam in TC.CAMERAS + TC.NOTHING:
        assert any(c.camera == cam and c.shape == TC.BASE for c in cs), cam
    assert sum(1 for c in cs if c.seed and c.id.count("=") >= 3) >= 15          # the random combinations
    for v in (0, 1):
        assert any(c.params["has_v"] == v for c in cs)


def test_each_case_reaches_what_it_is_for():
    base = TC.reference(_first(shape=TC.BASE, camera="pan", masks=("random", "random"), seed=0))
    h, w = TC.BASE
    hit, nh, why = base["cur"]["hit"], base["nh"], base["reasons"]
    keep = ~base["near"]
    assert (keep & hit & (nh > 0)).sum() > 200 and (keep & hit & (nh == 0)).sum() > 50
    assert why["capped"].any() and (hit & (nh > 0) & ~why["capped"]).any()
    u, v = why["u"], why["v"]
    for name, edge in (("u < 0", (u > -1) & (u < 0)), ("u > w - 1", (u > w - 1) & (u < w)), ("v < 0", (v > -1) & (v < 0)),
                       ("v > h - 1", (v > h - 1) & (v < h))):
        inside = hit & edge & (u > -1) & (u < w) & (v > -1) & (v < h)
        assert (inside & (nh > 0)).any(), name                 # and the taps that are left inside the frame are taken
    for k in ("normal_rejected", "normal_accepted", "plane_rejected", "plane_accepted"):
        assert (why[k] & hit).sum() > 10, k
    # the ids: every band and the upper half occur, one material is -1 and one is nmats
    mats = set(np.unique(base["cur"]["material"]))
    assert mats == {-1, 1, 2, TC.NMATS} and len(np.unique(base["cur"]["geom"])) >= 8
    spec = hit & (base["cur"]["material"] == 2)
    assert spec.sum() > 50 and not nh[spec].any()
    on = TC.reference(_first(shape=TC.BASE, specular_history=1, seed=0))
    assert (on["nh"][spec] > 0).sum() > 20
    # every max_history of the sweep binds, on fractional counts; and the counts reach 40
    assert base["prev"]["n"].max() > 35 and (base["prev"]["n"] % 1 != 0).all()
    for m in (1, 3, 16):
        r = TC.reference(_first(shape=TC.BASE, camera="pan", max_history=m, seed=0))
        got = r["nh"][r["cur"]["hit"] & (r["nh"] > 0)]
        assert r["reasons"]["capped"].sum() > 20 and (got == m).any() and (got <= m).all(), m
        if m > 1:
            assert (got < m).any(), m
    # the thresholds' other values move taps across them
    for k, v, tap in (("normal_cos", 0.5, "normal_rejected"), ("plane_tolerance", 0.5, "plane_rejected")):
        r = TC.reference(_first(shape=TC.BASE, seed=0, **{k: TC.f32(v)}))
        assert (r["reasons"][tap] & hit).sum() < (why[tap] & hit).sum(), k
    # the cameras
    for cam in TC.CAMERAS:
        r = TC.reference(_first(shape=TC.BASE, camera=cam, seed=0))
        hit_c = r["cur"]["hit"]
        assert (hit_c & (r["nh"] > 0)).sum() > 200 and (hit_c & (r["nh"] == 0)).sum() > 20, cam
    third = TC.reference(_first(shape=TC.BASE, camera="lose_third", seed=0))
    projected = third["cur"]["hit"] & (third["cur"]["material"] != 2)        # (u is NaN on the specular pixels: not considered)
    lost = ~((third["reasons"]["u"] > -1) & (third["reasons"]["u"] < w))
    assert 0.25 < lost[projected].mean() < 0.45
    roll = TC.hist_camera("roll", h, w)
    assert abs(np.degrees(np.arcsin(roll["right"][1])) - 10.0) < 0.01
    aniso, skew = TC.hist_camera("aniso", h, w), TC.hist_camera("skew", h, w)
    assert aniso["pl"][0] != aniso["pl"][1] and abs(skew["right"] @ skew["up"]) > 0.01
    for cam in TC.NOTHING:
        for c in TC.CASES:
            if c.camera == cam:
                r = TC.reference(c)
                assert not r["nh"].any() and not r["h"].any() and np.array_equal(r["mix"], r["c32"].astype(np.float64)), c.id
    behind = TC.reference(_first(shape=TC.BASE, camera="behind"))
    assert not behind["reasons"]["s"].any() and np.isnan(behind["reasons"]["u"]).all()
    assert probe.camera(TC.hist_camera("singular", h, w))[2] is False and probe.camera(TC.hist_camera("behind", h, w))[2] is True
    zero = TC.reference(_first(shape=TC.BASE, max_history=0, seed=0))
    assert not zero["nh"].any() and (zero["reasons"]["plane_accepted"] & zero["cur"]["hit"]).any()


def test_the_threshold_cases_are_exact_and_decided_alike():
    n = 0
    for c in TC.CASES:
        if not c.exact:
            continue
        n += 1
        r = TC.reference(c)
        if c.camera in ("none", "singular"):
            continue
        cur, pg = r["cur"], r["prev"]["gbuf"]
        for g in (cur, pg):
            assert (g["normal"] == np.float32([0, 0, 1])).all() and np.isin(g["position"][..., 2], [0.0, 0.25, 0.5, 0.75]).all(), c.id
        hit, why = cur["hit"], r["reasons"]
        inherits = hit & (r["nh"] > 0)
        flagged = why["normal"] | why["plane"]
        if c.params["normal_cos"] == 1.0 or c.params["plane_tolerance"] == 0.0:
            assert (flagged | ~inherits).all(), c.id           # the restatement's own `near` would drop every pixel of interest
        if c.shape == TC.BASE and c.masks == ("random", "random") and c.camera in TC.CAMERAS and c.params["max_history"] > 0:
            assert (inherits & ~r["near"]).sum() > 100, c.id
            if c.params["plane_tolerance"] == 0.0:
                assert (why["plane_rejected"] & hit).sum() > 20 and (why["plane_accepted"] & hit).sum() > 100, c.id
    assert n >= 4


def test_the_poisoned_cases():
    cs = [c for c in TC.CASES if c.poison]
    assert len(cs) == 2
    for c in cs:
        r = TC.reference(c)
        p, cur, pg = r["poisoned"], r["cur"], r["prev"]["gbuf"]
        bad = ~(np.isfinite(cur["position"]).all(-1) & np.isfinite(cur["normal"]).all(-1))
        assert p.sum() == 6 and np.array_equal(p, bad) and cur["hit"][p].all()
        assert np.isinf(cur["position"]).any() and np.isnan(cur["normal"]).any() and np.isinf(cur["normal"]).any()
        hbad = ~(np.isfinite(pg["position"]).all(-1) & np.isfinite(pg["normal"]).all(-1))
        assert hbad.sum() == 6 and pg["hit"][hbad].all() and np.isinf(pg["position"]).any() and np.isnan(pg["normal"]).any()
        assert not r["nh"][p].any() and np.array_equal(r["mix"][p], r["c32"][p].astype(np.float64)) and not r["near"][p].any()
        assert np.isfinite(r["nh"]).all() and np.isfinite(r["h"]).all() and np.isfinite(r["mix"]).all()
        for v in (0, 1, 2):                              # and the probe, which does read them, says the same
            q = _probe(c, r, v)
            assert not q["nh"][p].any() and np.array_equal(q["mix"][p], r["c32"][p])


def test_masks_apply_to_either_side_alone():
    for s in TC.MASK_SHAPES:
        r = TC.reference(_first(shape=s, masks=("all_hit", "all_miss")))
        assert r["cur"]["hit"].all() and not r["prev"]["gbuf"]["hit"].any() and not r["nh"].any()
        r = TC.reference(_first(shape=s, masks=("all_hit", "single")))
        assert r["prev"]["gbuf"]["hit"].sum() == 1 and 1 <= (r["nh"] > 0).sum() <= 4
        r = TC.reference(_first(shape=s, masks=("all_hit", "last_tile")))
        # (at 5 x 65 the last tile's one row lies in hist's displaced strip: the plane test rejects it)
        assert (s == (5, 65) or (r["nh"] > 0).any()) and (r["nh"] > 0).sum() <= 4 * r["prev"]["gbuf"]["hit"].sum()


# --- the entry point's refusals --------------------------------------------------------------------------------------------------------


def test_bad_arguments_are_refused_before_the_device_is_looked_for(product):
    pt = product
    c = _first(shape=(5, 65), camera="subpixel", masks=("random", "random"))
    b = c.build()

    def call(variant=0, drop=(), **over):
        args, kw = TC.api_arguments(c, b, variant)
        args = list(args)
        for i in drop:
            args[i] = None
        kw.update(over)
        return pt.reproject_buffers(*args, **kw)

    for what, kw in (("variant", dict(variant=3)), ("variant", dict(variant=-1)), ("spp", dict(spp=0)), ("max_history", dict(max_history=-1)),
                     ("normal_cos", dict(normal_cos=1.5)), ("plane_tolerance", dict(plane_tolerance=-0.5)),
                     ("plane_tolerance", dict(plane_tolerance=float("inf"))), ("scatter6", dict(variant=2, scatter=None)),
                     ("batches >= 2, not 1", dict(variant=2, batches=1)), ("hist_hit", dict(hist=None)),
                     ("resolution is 64 x 5", dict(hist_camera=dict(b["hist_cam"], W=64))), ("device ordinal", dict(device=-1))):
        with pytest.raises(pt.PathTracerError, match=what) as e:
            call(**kw)
        if what != "device ordinal":
            assert "code 1)" in str(e.value), str(e.value)               # PTX_ERR_INVALID
    for i in (1, 2, 3, 4):                               # albedo, normal, position, ids
        with pytest.raises(pt.PathTracerError, match="are required"):
            call(drop=(i,))
    with pytest.raises(TypeError, match="passes"):
        call(passes=3)
    lib = pt.load_library()
    f = np.zeros(12, np.float32)
    p = f.ctypes.data_as(ctypes.c_void_p)
    for w, h in ((0, 1), (1, 0), (1 << 16, 1 << 16)):
        assert lib.ptx_kat_reproject(0, w, h, 0, None, None, 1, p, p, p, p, p, p, p, 1, *[None] * 8, 0, *[None] * 6) == 1
        assert b"bad frame size" in lib.ptx_last_error()
    assert lib.ptx_kat_reproject(0, 1, 1, 0, None, None, 1, p, p, p, p, p, p, None, 2, *[None] * 8, 0, *[None] * 6) == 1
    assert b"nmats = 2" in lib.ptx_last_error()
    assert lib.ptx_kat_reproject(0, 1, 1, 0, None, None, 1, p, p, p, p, p, p, None, -1, *[None] * 8, 0, *[None] * 6) == 1
    if lib.ptx_device_count() < 1:                       # every argument good: the device is the one thing missing
        with pytest.raises(pt.PathTracerError, match="no HIP device"):
            call()
        with pytest.raises(pt.PathTracerError, match="no HIP device"):
            call(variant=2, hist_camera=None)
