"""GPU: the opt-in arithmetic levels (ptx_options.arith 1 = CONTRACTED, 2 = FAST: the same kernels as second / third code objects,
csrc/pt_kernels.hip compiled with PT_ARITH = 1 / 2; every level's table reaches the host the same way) against the EXACT level on the same device.

The exact level is bit-identical to the CPU oracle (tests/test_gpu_parity.py) and stays the default and the headline.  The other two
run the kind of arithmetic the reference's REAL build runs (nvcc fuses multiply-adds by default) or a faster one, and promise the
tolerance north_star asks for ("within a stated fp32 tolerance"), which -- because the shading RNG is seeded by stream position, so
one flipped hit/miss re-seeds the rest of its bounce -- can only be statistical at frame level (tests/test_fp_tolerance.py states it
between two CPU builds of the oracle; here the very same bounds are asserted between two GPU code objects) and a stated error bound
per stage on identical inputs:

  stage                      CONTRACTED (1)                               FAST (2)
  generateRayFromCamera      direction within 4 ulp of |d| = 1            4 ulp (16 with depth of field at either level)
  computeIntersections       99 % of the hit distances within 8 ulp,      8 ulp, 1024 ulp
                             all within 256 ulp (relative);
                             99 % of the normals within 32 ulp of unit    64 ulp, 4096 ulp
                             length, all within 4096 ulp (5e-4)
                             -- the tail is conditioning, not the level: a sphere's root and a mesh's barycentrics cancel at grazing
                             incidence (measured maxima: 64 / 170 ulp in t, 7e2 / 1.3e3 ulp in the normal, profiles/round5_arith_levels.txt);
                             hit / miss / geom decisions differ on < 0.2 % of the rays at either level (measured: none of 5 k)
  shadeFakeMaterial          same branch for every path; new direction    2e-5 (measured 1.6e-6); colour 8 ulp
                             within 1e-5 absolute (measured 3e-7),
                             colour within 8 ulp
  sin / cos                  2 ulp of 1 (measured 1)                      1e-5 absolute (v_sin_f32 / v_cos_f32: measured 5e-7)

The bounds above are distances to level 0, set from what was measured.  The rule against the truth stands beside them in
tests/test_gpu_arith_f64.py, on ray families built for the purpose (tests/arithcases.py):

  the three intersection     on the rays where a float64 reference of the     the same with m = 8 (one ulp for the hardware's
  tests against float64      same operation (tests/isect_f64.py), level 0     seeds and 2.5 ulp for a * rcp(b) against half an
                             and this level report the same hit: rms and      ulp: 5, with margin)
                             99th percentile of |level - reference| in t,
                             point and normal <= 2 x max(level 0's, 1 u)
                             (contraction only removes roundings);
                             decisions as the reference's wherever level 0's are, elsewhere at most 2 x level 0's exceptions + 4
"""
import os

import numpy as np
import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

LEVELS = (1, 2)
ULP = float(np.finfo(np.float32).eps)          # 2^-23: one ulp of 1.0


def _tracer(pt, scene, res, depth, **opt):
    s = pt.Scene(os.path.join(ROOT, "scenes", scene), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s, pt.Tracer(s, **opt)


def test_levels_are_separate_code_objects_and_bad_levels_are_refused(gpu_product):
    pt = gpu_product
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"), res=(64, 64), depth=4)
    s.apply_runcuda_camera()
    imgs = {}
    for lv in (0,) + LEVELS:
        with pt.Tracer(s, arith=lv) as T:
            T.render(1, 4)
            imgs[lv] = T.read_image()
            assert T.stats()["fenced"] == 0
    # the exact level does not depend on the others being in the library, and they are not the exact one under another name
    with pt.Tracer(s) as T:
        T.render(1, 4)
        assert np.array_equal(T.read_image().view(np.uint32), imgs[0].view(np.uint32))
    # (a frame this small may well come out bit-identical at every level -- radiance is a product of colours, and no decision need flip
    # in 16 k paths; that the levels ARE different code is shown on the stages below, where hit distances differ in the last places)
    for lv in LEVELS:
        assert abs(float(imgs[lv].mean()) / float(imgs[0].mean()) - 1.0) < 0.05
    for bad in (3, -1):
        with pytest.raises(pt.PathTracerError):
            pt.Tracer(s, arith=bad)


@pytest.mark.parametrize("level", LEVELS)
def test_stage_error_bounds_on_identical_inputs(gpu_product, level):
    """generate / intersect / shade of the exact and of the other level's code object on the same inputs (the per-stage entry points):
    the bounds of the table in this module's docstring."""
    pt = gpu_product
    gen_ulp, t99_ulp, t_ulp, n99_ulp, n_ulp = ((4, 8, 256, 32, 4096), (4, 8, 1024, 64, 4096))[level - 1]
    dir_abs, col_ulp = ((1e-5, 8), (2e-5, 8))[level - 1]
    some_t_differs = False
    for scene, res, depth, opt in (("cornellObj.txt", (96, 54), 8, {}), ("cornellGlass.txt", (96, 54), 12, dict(depth_of_field=1)),
                                   ("cornellSpaceship.txt", (96, 54), 8, {})):
        s, T0 = _tracer(pt, scene, res, depth, **opt)
        T1 = pt.Tracer(s, arith=level, **opt)
        p0, p1 = T0.generate(3), T1.generate(3)
        assert np.array_equal(p0["pixelIndex"], p1["pixelIndex"]) and np.array_equal(p0["origin"], p1["origin"]) or opt.get("depth_of_field")
        assert np.abs(p0["direction"] - p1["direction"]).max() <= gen_ulp * ULP * (4 if opt.get("depth_of_field") else 1)
        if opt.get("depth_of_field"): assert np.abs(p0["origin"] - p1["origin"]).max() <= 1e-5          # (the lens sample: sin / cos)
        i0, i1 = T0.compute_intersections(p0), T1.compute_intersections(p0)
        same = (i0["t"] > 0) == (i1["t"] > 0)
        same &= np.where(i0["t"] > 0, i0["geomId"] == i1["geomId"], True)
        assert 1.0 - same.mean() < 0.002, (scene, 1.0 - same.mean())
        both = same & (i0["t"] > 0)
        terr = np.abs(i0["t"][both] - i1["t"][both]) / np.abs(i0["t"][both]) / ULP
        nerr = np.abs(i0["normal"][both] - i1["normal"][both]).max(axis=1) / ULP
        assert terr.max() <= t_ulp and np.quantile(terr, 0.99) <= t99_ulp, (scene, terr.max(), np.quantile(terr, 0.99))
        assert nerr.max() <= n_ulp and np.quantile(nerr, 0.99) <= n99_ulp, (scene, nerr.max(), np.quantile(nerr, 0.99))
        assert np.array_equal(i0["materialId"][both], i1["materialId"][both])
        some_t_differs |= bool(terr.max() > 0)
        # the tile-cooperative path production intersects with (candidate masks, pair lists, 64-bit minimum) on the same rays
        if scene != "cornellSpaceship.txt":
            k0, k1 = T0.tile_intersect(p0), T1.tile_intersect(p0)
            samek = ((k0["t"] > 0) == (k1["t"] > 0)) & np.where(k0["t"] > 0, k0["geomId"] == k1["geomId"], True)
            assert 1.0 - samek.mean() < 0.002
            bk = samek & (k0["t"] > 0)
            assert (np.abs(k0["t"][bk] - k1["t"][bk]) <= t_ulp * ULP * np.abs(k0["t"][bk])).all()
        idx = np.random.default_rng(9).integers(0, 4_000_000, len(p0)).astype(np.int32)
        s0, s1 = T0.shade(3, idx, i0, p0), T1.shade(3, idx, i0, p0)
        assert np.array_equal(s0["remainingBounces"], s1["remainingBounces"])          # same branch of shadeFakeMaterial for every path
        live = s0["remainingBounces"] > 0
        # (a refraction at the critical angle may take the other side of `IoR1 / IoR2 * sinTheta > 1`: such a path's new direction is
        # another ray altogether -- counted, not bounded)
        ddir = np.abs(s0["direction"][live] - s1["direction"][live]).max(axis=1)
        assert (ddir > dir_abs).mean() < 0.001, (scene, float((ddir > dir_abs).mean()))
        ok = ddir <= dir_abs
        col = np.abs(s0["color"][live][ok] - s1["color"][live][ok])
        assert (col <= col_ulp * ULP * np.maximum(np.abs(s0["color"][live][ok]), 1e-3)).all()
        T0.close(); T1.close()
    assert some_t_differs          # the level's kernels are NOT the exact ones under another name


@pytest.mark.parametrize("level", LEVELS)
def test_sampler_sine_and_cosine(gpu_product, level):
    pt = gpu_product
    s, T0 = _tracer(pt, "sphere.txt", (16, 16), 2)
    T1 = pt.Tracer(s, arith=level)
    rng = np.random.default_rng(2)
    n = 200000
    x = np.concatenate([(rng.random(n - 6) * np.float32(6.2831855)).astype(np.float32), np.float32([0, 6.2831855, 3.1415927, 1.5707964, 0.7853982, 4.712389])])
    pw = rng.uniform(0.0, 1.0, n)
    pxy = np.stack([rng.random(n).astype(np.float32), rng.uniform(0, 60, n).astype(np.float32)], 1)
    a, b = T0.libm(x, pw, pxy), T1.libm(x, pw, pxy)
    bound = 2 * ULP if level == 1 else 1e-5
    assert np.abs(a[0] - b[0]).max() <= bound and np.abs(a[1] - b[1]).max() <= bound
    assert np.array_equal(a[2], b[2])                                             # Schlick's binary64 power: the same at every level
    T0.close(); T1.close()


def _frames(pt, scene, res, depth, aa, level, spp_marks):
    """per-iteration radiance through pathtrace(iter) + read-back; -> {spp: (mean image, per-pixel standard error)}, rays per bounce of iteration 1"""
    s = pt.Scene(os.path.join(ROOT, "scenes", scene), res=res, depth=depth)
    s.apply_runcuda_camera()
    out, counts = {}, None
    with pt.Tracer(s, arith=level, antialiasing=aa) as T:
        prev = s1 = s2 = None
        for it in range(1, max(spp_marks) + 1):
            T.pathtrace(it)
            img = T.read_image().astype(np.float64)
            one = img if prev is None else img - prev
            prev = img
            s1 = one if s1 is None else s1 + one
            s2 = one * one if s2 is None else s2 + one * one
            if it == 1:
                counts = T.stats()["rays_per_bounce"]
            if it in spp_marks:
                var = np.maximum(s2 / it - (s1 / it) ** 2, 0.0) * (it / max(it - 1, 1))
                out[it] = (img / it, np.sqrt(var / it))
        assert T.stats()["fenced"] == 0
    return out, counts


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("config", ["C2", "C3", "C4"])
def test_contracted_arithmetic_stays_within_the_stated_tolerance(gpu_product, config, level):
    """BASELINE configs 2-4 at 480 x 270, exact code object against level 1 / 2 on the same GPU: the bounds tests/test_fp_tolerance.py
    asserts between the oracle and its FMA-contracted build -- fewer than 8 % of the pixels differ at 1 spp; at 16 spp the frame means
    agree within 2 % and 4 standard errors and the per-pixel RMS difference stays below 1.5 x the Monte-Carlo noise; the rays entering
    bounce 1 agree within 0.1 %, later bounces like two samples of one process."""
    import fp_tolerance
    cfg = fp_tolerance.CONFIGS[config]
    res = fp_tolerance.RES
    ra, ca = _frames(gpu_product, cfg["scene"], res, cfg["depth"], cfg["aa"], 0, (1, 16))
    rb, cb = _frames(gpu_product, cfg["scene"], res, cfg["depth"], cfg["aa"], level, (1, 16))
    assert ca[0] == cb[0] and len(ca) == len(cb)
    assert abs(ca[1] - cb[1]) <= 0.001 * ca[1] + 2, (ca, cb)
    for a, b in zip(ca[2:], cb[2:]):
        assert abs(a - b) <= 5.0 * np.sqrt(a + b) + 2, (ca, cb)
    npx = res[0] * res[1]
    a1, b1 = ra[1][0], rb[1][0]
    assert float(np.any(a1 != b1, axis=1).mean()) < 0.08
    (a, sa), (b, sb) = ra[16], rb[16]
    mean_a, mean_b = a.mean(axis=0), b.mean(axis=0)
    se = np.sqrt((sa ** 2).sum(axis=0) + (sb ** 2).sum(axis=0)) / npx
    assert (np.abs(mean_b - mean_a) / np.maximum(np.abs(mean_a), 1e-12)).max() < 0.02
    assert (np.abs(mean_b - mean_a) / np.maximum(se, 1e-30)).max() < 4.0
    noise = float(np.sqrt((sa ** 2).mean()))
    assert float(np.sqrt(((b - a) ** 2).mean())) / max(noise, 1e-30) < 1.5


@pytest.mark.parametrize("level", LEVELS)
def test_split_mesh_search_at_the_other_levels(gpu_product, level):
    """The C5-shaped scene (textured BVH mesh, depth of field; pass 1 / k_mesh / k_finish / pass 2 from the level's code object):
    runs clean (no fenced index), and the frame is the exact level's within Monte-Carlo noise."""
    pt = gpu_product
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornellSpaceship20k.txt"), res=(320, 180), depth=8)
    s.apply_runcuda_camera()
    means = {}
    for lv in (0, level):
        with pt.Tracer(s, arith=lv, depth_of_field=1) as T:
            T.render(1, 24)
            st = T.stats()
            assert st["fenced"] == 0
            means[lv] = (T.read_image().astype(np.float64).mean(axis=0) / 24, st["rays_total"])
    assert np.abs(means[level][0] / means[0][0] - 1.0).max() < 0.03
    assert abs(means[level][1] / means[0][1] - 1.0) < 0.01


@pytest.mark.parametrize("level", LEVELS)
def test_full_size_frames_at_the_other_levels(gpu_product, level):
    """BASELINE config 4 at its own size (1920x1080, depth 8, 24 iterations through ptx_render: three launch sets in flight, the record masks,
    the one-word local index) from the level's code object: no fenced index, the rays entering every bounce within 0.2 % of the exact level's,
    the frame's mean radiance within 0.5 %."""
    pt = gpu_product
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"), res=(1920, 1080), depth=8)
    s.apply_runcuda_camera()
    got = {}
    for lv in (0, level):
        with pt.Tracer(s, arith=lv) as T:
            T.render(1, 24)
            st = T.stats()
            assert st["fenced"] == 0
            got[lv] = (T.read_image().astype(np.float64).mean(axis=0), st["rays_total"], st["rays_per_bounce"])
    assert abs(got[level][1] / got[0][1] - 1.0) < 0.002
    assert all(abs(a - b) <= 0.002 * b + 50 for a, b in zip(got[level][2], got[0][2]))
    assert np.abs(got[level][0] / got[0][0] - 1.0).max() < 0.005
