"""CPU: the cases of tests/displaycases.py are what they claim to be -- the column frames' block grid as the library computes it, no two
blocks 1024 j apart with one exponent, the threshold blocks on their sides of L_MIN, every W*H mod 4 among the tail sizes, the blocks
of more than 512 pixels -- and map_pixel's tone step restated in numpy float32 on grey and non-grey pixels: the rule's expression as it
stands overflows to black beyond fp32's range, the form the kernel uses follows the float64 rule at every case of the grid."""
import numpy as np
import pytest

import display_ref as dr
import displaycases as dc


@pytest.mark.parametrize("n", dc.METER_BLOCK_COUNTS)
def test_column_frames_are_one_column_of_n_blocks(product, n):
    c = dc.column_frame(n, seed=n)
    rows, cols = product.api.debug_display_blocks(c["w"], c["h"])
    assert len(cols) - 1 == 1 and len(rows) - 1 == n and cols.tolist() == [0, 8]
    assert rows.tolist() == dr.block_grid(c["w"], c["h"])[0]
    d = np.diff(rows)
    assert set(d.tolist()) <= {15, 16} and c["rgb"].shape == (16 * n - 8, 8, 3) and c["w"] * c["h"] <= 8 * 81928
    # every block is constant: the frame's rows between two boundaries hold one value
    per_row = c["rgb"][:, 0, 0]
    assert (c["rgb"] == per_row[:, None, None]).all()
    assert all((per_row[rows[i]:rows[i + 1]] == per_row[rows[i]]).all() for i in range(n))
    want = np.minimum(per_row[rows[:-1]].astype(np.float64), dr.C_MAX) * dr.LUM.sum()       # (2^16 .. 2^18 sanitise to 65504)
    assert np.array_equal(want, c["blocks"]) and (per_row > dr.C_MAX).any()
    # what the restatement's own double loop makes of it, once, at the smallest frame (the device tests use the constants directly)
    if n == dc.METER_BLOCK_COUNTS[0]:
        b = dr.block_means(c["rgb"], 1, c["w"], c["h"])
        assert np.allclose(b[:, 0], c["blocks"], rtol=1e-12, atol=0) and dr.meter(b)["blocks_used"] == c["blocks_used"]
        assert abs(dr.meter(b)["log2_mean"] - c["log2_mean"]) < 1e-12
    zeros = int((np.arange(n) % 53 == 0).sum())
    assert c["blocks_used"] == n - zeros - 1 and (c["blocks"] == 0).sum() == zeros


def test_blocks_a_multiple_of_1024_apart_never_share_an_exponent():
    """so a load from the wrong one of the meter's four slots, or a skipped trip, moves the sum of log2 by at least 1.  (Exponents 16,
    17 and 18 all sanitise to 65504: two of those are one value to the meter, 9 pairs of 37 x 36.  What a misread slot does to the
    whole sum is therefore checked on the luminances the meter sees: slot j read as slot j - 1 moves it by more than 1 wherever
    slot j exists.)"""
    for n in dc.METER_BLOCK_COUNTS:
        e = dc.block_exponents(n)
        assert e.min() >= -18 and e.max() <= 18
        for j in range(1, 5):
            if n > dc.NTM * j:
                assert (e[:-dc.NTM * j] != e[dc.NTM * j:]).all(), (n, j)
        lum = dc.column_frame(n, seed=n)["blocks"]
        l2 = np.where(lum > dr.L_MIN, np.log2(np.maximum(lum, 1e-300)), 0.0)
        for j in range(1, 4):
            k = np.arange(dc.NTM)
            k = k[k + dc.NTM * j < n]
            if len(k):
                moved = abs((l2[k + dc.NTM * (j - 1)] - l2[k + dc.NTM * j]).sum())
                assert moved > 1.0 and moved / n > 1e-4, (n, j, moved)


def test_threshold_blocks_are_on_their_sides_of_l_min():
    f = np.float32
    lum = lambda v: (f(0.2126) * f(v) + f(0.7152) * f(v)) + f(0.0722) * f(v)          # pt_luminance of a grey pixel, in fp32
    assert lum(dc.BELOW_L_MIN) < f(dr.L_MIN) / f(1.3) and lum(dc.ABOVE_L_MIN) > f(dr.L_MIN) * f(1.3)
    assert dc.BELOW_L_MIN * dr.LUM.sum() < dr.L_MIN / 1.3 and dc.ABOVE_L_MIN * dr.LUM.sum() > dr.L_MIN * 1.3
    for n in dc.METER_BLOCK_COUNTS:
        v, below, above = dc.column_blocks(n, n)
        assert v[below] == dc.BELOW_L_MIN and v[above] == dc.ABOVE_L_MIN and below != above and below % 53 and above % 53


def test_tail_sizes_cover_every_remainder():
    assert tuple(w * h % 4 for w, h in dc.TAIL_SIZES) == dc.TAIL_MOD4 and set(dc.TAIL_MOD4) == {0, 1, 2, 3}
    assert sorted(w * h for w, h in dc.TAIL_SIZES if w * h < 4) == [1, 2, 3] and (2, 2) in dc.TAIL_SIZES


def test_only_23_x_23_has_a_block_beyond_512_pixels():
    for (w, h), want in (((23, 23), 529), ((22, 23), 506), ((23, 22), 506)):
        rows, cols = dr.block_grid(w, h)
        assert rows == [0, h] and cols == [0, w] and (rows[1] - rows[0]) * (cols[1] - cols[0]) == want
        rgb = dc.hdr_buffer(w, h)
        lum = dr.luminance(dr.sanitise(rgb, 3).reshape(-1, 3))
        assert lum[512:].sum() > 1e-3 * lum.sum() or want <= 512                      # the third trip's pixels carry weight


def test_the_grid_and_the_sweep_are_what_the_issue_lists():
    g = dc.MAP_GRID
    assert len(g) == len({dc.case_id(c) for c in g}) == 116 and len(dc.map_launches()) == 128 < 200
    core = [c for c in g if c["samples"] == 3.0 and c["white"] == 4.0]
    assert len(core) == 48 and {(c["tone"], c["transfer"], c["exposure"]) for c in core} == {(t, x, e) for t in dc.TONES for x in dc.TRANSFERS
                                                                                           for e in dc.EXPOSURES}
    assert {c["samples"] for c in g} == set(dc.SAMPLES) and {c["white"] for c in g if c["tone"] == "reinhard"} == set(dc.WHITES + dc.HUGE_WHITES)
    assert {q for _, q in dc.map_launches()} == set(dc.QUANTISERS)
    with np.errstate(over="ignore"):
        assert np.float32(65504.0) * np.float32(3e34) == np.inf
    v = dc.sweep_values()
    assert 0 < v[2] < np.finfo(np.float32).tiny and np.signbit(v[1]) and v[1] == 0 and np.isnan(v).sum() == 1 and np.isinf(v).sum() == 1
    fr = dc.sweep_frame()
    assert fr.shape == (67, 64, 3) and 3 * len(v) <= 64 * 67
    flat = fr.reshape(-1, 3)
    grey = (flat[:, 0] == flat[:, 1]) & (flat[:, 1] == flat[:, 2])
    assert grey.sum() >= len(v) - 1 and (~grey).sum() >= 2 * len(v)
    for e in dc.EXPOSURES:                                                            # both sides of the sRGB branch point at every E
        x = v[np.isfinite(v)].astype(np.float64) * float(np.float32(e))
        assert (x <= dc.SRGB_KNEE).any() and ((x > dc.SRGB_KNEE) & (x < dc.SRGB_KNEE * 1.000001)).any(), e


@pytest.mark.parametrize("case", dc.MAP_GRID, ids=dc.case_id)
def test_no_saturation_is_decided_by_rounding(case):
    """the device test asserts z = transfer(1) exactly wherever the float64 y before the clamp is at least 1: no y of the curves lies
    in [1, 1 + 2e-6), 16 fp32 ulps, where fp32 rounding of the curve could land below 1 (tone CLAMP: x = c E is one correctly rounded
    product, so y >= 1 in float64 means y >= 1 in fp32)"""
    if case["tone"] == "clamp":
        return
    y = dc.premapped(case)
    if dc.huge(case):                                                 # (displaycases.saturated: these ask for exactness above the band only)
        return
    assert not ((y >= 1.0) & (y < 1.0 + 2e-6)).any()


def _metric(got, ref):
    return float((np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + 1e-3)).max())


def _sanitised_f32(case):
    return dr.sanitise(dc.sweep_frame() * np.float32(case["samples"]), case["samples"]).astype(np.float32)


@pytest.mark.parametrize("case", [c for c in dc.MAP_GRID if c["transfer"] == "linear"], ids=dc.case_id)
def test_the_float32_restatement_of_map_pixel_follows_the_rule(case):
    """map_pixel's tone step restated operation for operation in numpy float32 (displaycases.tone_f32), on the sweep frame's grey and
    non-grey pixels, against the float64 rule by the GPU suites' metric: within a quarter of the device's bound 1e-4 at every case of
    the grid, a saturated channel exactly 1.  The rule's expression written down as it stands fails both at the cases recorded below."""
    c = _sanitised_f32(case)
    y64 = dc.premapped(case)
    ref = np.clip(y64, 0.0, 1.0)
    y = dc.tone_f32(c, case["exposure"], case["tone"], case["white"])
    assert _metric(y, ref) <= 2.5e-5
    assert (y[dc.saturated(case, y64)] == 1).all() and (y[c == 0] == 0).all()
    plain = dc.tone_f32(c, case["exposure"], case["tone"], case["white"], fixed=False)
    broken = _metric(plain, ref) > 1e-4
    x_max = 65504.0 * case["exposure"]
    want = (case["tone"] == "aces" and x_max > 1.2e19) or (case["tone"] == "reinhard" and (x_max > 3.4e38 or case["white"] == 1e-20
                                                                                         and case["exposure"] == 1.0))
    assert broken == want, (broken, want)
    if x_max < dc.X_CAP and not broken:
        assert np.array_equal(plain, y)                              # where the plain form holds, the fixed one is the same bits


def test_the_fp32_curves_overflow_to_black_and_what_removes_it():
    """Recorded: aces(x) in fp32 is inf / inf = NaN from x of about 1.2e19 (both products overflow), and so is Reinhard at x = inf
    (inf * inf / inf); the device's clamp fminf(fmaxf(NaN, 0), 1) makes that 0 where the rule (the curve, then the clamp) gives 1.
    ACES with x held to 2^60 is exactly 1 on all of [8, +inf] and unchanged below.  Reinhard keeps the ratios between the channels:
    the reviewer's pixels, whose red and blue stay far below 1 beside a saturated green at huge E and white."""
    f = np.float32
    x = 2e19
    y64 = x * (2.51 * x + 0.03) / (x * (2.43 * x + 0.59) + 0.14)
    assert 1.03 < y64 < 1.04
    with np.errstate(all="ignore"):
        y32 = (f(x) * (f(2.51) * f(x) + f(0.03))) / (f(x) * (f(2.43) * f(x) + f(0.59)) + f(0.14))
    assert np.isnan(y32)
    grey = lambda v: np.repeat(np.asarray(v, f)[:, None], 3, 1)
    assert dc.tone_f32(grey([1e19, 2e19, 1e30, np.inf]), 1.0, "aces", fixed=False)[:, 0].tolist() == [1.0, 0.0, 0.0, 0.0]
    for white in dc.WHITES:                                           # x = 65504 * 1.5e25 and x = 65504 * 3e34 = inf
        assert [float(dc.tone_f32(grey([65504.0]), E, "reinhard", white, fixed=False)[0, 0]) for E in (1.5e25, 3e34)] == [1.0, 0.0]
        assert [float(dc.tone_f32(grey([65504.0]), E, "reinhard", white)[0, 0]) for E in (1.5e25, 3e34)] == [1.0, 1.0]
    cap = dc.X_CAP
    assert f(cap) == cap and 2.51 * cap ** 2 < np.finfo(f).max / 16
    xs = np.concatenate([np.geomspace(8.0, cap, 200001), [2e19, 1e30, float(np.finfo(f).max), np.inf]]).astype(f)
    assert (dc.tone_f32(grey(xs), 1.0, "aces") == 1).all()
    below = np.geomspace(1e-8, cap, 20001).astype(f)
    assert np.array_equal(dc.tone_f32(grey(below), 1.0, "aces"), dc.tone_f32(grey(below), 1.0, "aces", fixed=False))
    # non-grey pixels beyond fp32's range: float64 of the rule against the float32 restatement
    for c, white, E in (((2000.0, 65504.0, 10.0), 1e10, 1e15), ((2000.0, 65504.0, 10.0), 1e15, 1e25), ((2000.0, 65504.0, 10.0), 1e19, 1e25),
                        ((2000.0, 65504.0, 10.0), 1e-20, 3e34), ((1e-40, 65504.0, 0.0), 1e-20, 1.0), ((1e-40, 65504.0, 0.0), 1e-30, 1.0),
                        ((3.0, 65504.0, 1e-30), 1e20, 3e34), ((65504.0, 12000.0, 0.0), 1e20, 3e34)):
        c32 = np.array([c], f)
        x = c32.astype(np.float64) * float(f(E))
        L = dr.luminance(x)[..., None]
        w = float(f(white))
        ref = np.clip(x * (1 + L / (w * w)) / (1 + L), 0, 1)
        got = dc.tone_f32(c32, E, "reinhard", white)
        assert _metric(got, ref) <= 2.5e-5, (c, white, E, got, ref)
    got = dc.tone_f32(np.array([[2000.0, 65504.0, 10.0]], f), 1e15, "reinhard", 1e10)[0]
    assert abs(got[0] - 0.0623) < 1e-4 and got[1] == 1 and abs(got[2] - 3.1e-4) < 1e-5
