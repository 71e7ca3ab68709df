"""GPU: arithmetic levels 1 and 2 through the kernel paths that only level 0 had run -- the refilling mesh walk and k_finish (frames of
split scenes), the general k_bounce on scenes without a mesh, sort_by_material = 0, more than 64 material bins, more than 32 geoms, the
unsplit textured and bump-mapped mesh, apps_variant, no_cull, row tiles, the first-bounce cache, the lit-plane gather at other batch
sizes.  tests/test_gpu_arith.py compares three Cornell scenes between levels; a hole in a mesh or a fenced index on one of these paths
would move a frame mean by less than the 2-3 % it allows.

Frames are 64 x 48 to 160 x 120, depth 4-8.  Every case asserts, at level 1 and at level 2:
  exact, any level          nothing fenced; every value finite and >= 0; the rays entering bounce 0 are level 0's; the ray counts do not
                            increase with the bounce.
  exact, within the level   the frame does not depend on how it was launched: image and rays per bounce of 64 iterations are
                            bit-identical between batch = 1 on one lane and batch = 5, 33, 64 (33 and 64 reach the gather's lit planes
                            32-63, partly and fully used), three lanes, and between render-ahead on and off -- the same code object and
                            the same instantiation, only the launch sets differ.  (Nothing is asserted bit for bit between the
                            specialised and the general kernel at these levels: different instantiations may contract differently.)
  statistical, vs level 0   the bounds of tests/test_gpu_arith.py::test_contracted_arithmetic_stays_within_the_stated_tolerance, which are
                            tests/test_fp_tolerance.py's, unchanged, at 1 and 16 spp.

Part a: the frame scenes of tests/test_gpu_mesh_walks.py for the mesh cases of tests/arithcases.py (not the NaN / tie scenes: level 0 covers
those), 64 x 48, depth 4, with and without depth of field, under the four plans with the plan asserted.  Part b: one case per remaining
path, each asserting the variant it is for by the means tests/test_gpu_parity.py uses (the debug switches, the refusal of the forced
specialised kernel, the plan queries, k_mesh's launch count, tile_intersect's refusal of a scene without candidate masks).

The statistical bounds are the oracle pair's, so a frame is a fair case for them only where the oracle and its contracted build meet them
themselves: tests/test_arith_paths_frames_cpu.py asserts that, without a GPU, for the frames of part a (with and without depth of
field) and of part b.  The general kernel and the full last bounce are asked for by their debug switches, as everywhere in the suite:
the library has no query that says which instantiation a launch took."""
import os
import re

import numpy as np
import pytest

import test_gpu_mesh_walks as mw
from arithpaths import MESH_FRAMES, PATHS
from conftest import ROOT, beq
from test_gpu_parity import CAMERA_BLOCK, MAT, O, _scene_from_text, fences_stay_silent      # noqa: F401  (O, fences: fixtures)

pytestmark = pytest.mark.gpu

LEVELS = (1, 2)
ITERS = 64
SWITCHES = ("PTX_DEBUG_NO_FAST", "PTX_DEBUG_FORCE_FAST", "PTX_DEBUG_NO_LAST", "PTX_DEBUG_NO_WIDE_BVH")


def _render(make, iters=ITERS, **opt):
    """-> (image, rays per bounce) of render(1, iters); nothing fenced, everything finite and >= 0, counts not increasing"""
    with make(**opt) as T:
        T.render(1, iters)
        img, st = T.read_image(), T.stats()
    assert st["fenced"] == 0
    assert np.isfinite(img).all() and (img >= 0).all()
    rpb = st["rays_per_bounce"]
    # (an iteration that replays the cached camera bounce traces no ray in bounce 0 and reports 0 there, at every level)
    assert rpb and all(a >= b for a, b in zip(rpb[1:] if rpb[0] == 0 else rpb, rpb[1:] if rpb[0] != 0 else rpb[2:])), rpb
    return img, rpb


def _stepwise(make, ahead, iters=ITERS, **opt):
    with make(**opt) as T:
        T.set_render_ahead(ahead)
        for it in range(1, iters + 1):
            T.pathtrace(it)
        img, st = T.read_image(), T.stats()
    assert st["fenced"] == 0
    return img, st["rays_per_bounce"], st["iterations"]


def _moments(make, level, spp_marks=(1, 16)):
    """per-iteration radiance through pathtrace + read-back (tests/test_gpu_arith.py::_frames, on a tracer factory)"""
    out, counts = {}, None
    with make(arith=level) as T:
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


def _stated_tolerance(ra, ca, rb, cb, npx):
    """tests/test_gpu_arith.py::test_contracted_arithmetic_stays_within_the_stated_tolerance's assertions, on two _moments results"""
    assert ca[0] == cb[0] and len(ca) == len(cb)
    assert abs(ca[1] - cb[1]) <= 0.001 * ca[1] + 2, (ca, cb)
    for a, b in zip(ca[2:], cb[2:]):
        assert abs(a - b) <= 5.0 * np.sqrt(a + b) + 2, (ca, cb)
    a1, b1 = ra[1][0], rb[1][0]
    assert float(np.any(a1 != b1, axis=1).mean()) < 0.08
    (a, sa), (b, sb) = ra[16], rb[16]
    mean_a, mean_b = a.mean(axis=0), b.mean(axis=0)
    se = np.sqrt((sa ** 2).sum(axis=0) + (sb ** 2).sum(axis=0)) / npx
    assert (np.abs(mean_b - mean_a) / np.maximum(np.abs(mean_a), 1e-12)).max() < 0.02
    assert (np.abs(mean_b - mean_a) / np.maximum(se, 1e-30)).max() < 4.0
    noise = float(np.sqrt((sa ** 2).mean()))
    assert float(np.sqrt(((b - a) ** 2).mean())) / max(noise, 1e-30) < 1.5


def check_case(make, npx, check_variant=None, statistical=True, base=None):
    """everything the module's docstring lists, for a tracer factory make(**options); base = the launch shape the others are compared with"""
    base = base or dict(batch=1, lanes=1)
    _, rpb0 = _render(make, arith=0, **base)
    ref = _moments(make, 0) if statistical else None
    for lv in LEVELS:
        if check_variant:
            check_variant(lv)
        img, rpb = _render(make, arith=lv, **base)
        assert rpb[0] == rpb0[0], (lv, rpb, rpb0)
        for opt in (dict(batch=5, lanes=1), dict(batch=33, lanes=1), dict(batch=64, lanes=1), dict(lanes=3)):
            img2, rpb2 = _render(make, arith=lv, **opt)
            assert beq(img2, img) and rpb2 == rpb, (lv, opt, int((img2 != img).any(axis=1).sum()), rpb2, rpb)
        on, off = _stepwise(make, True, arith=lv), _stepwise(make, False, arith=lv)
        assert beq(on[0], off[0]) and on[1:] == off[1:], (lv, on[1:], off[1:])
        assert beq(on[0], img), lv                                  # (one iteration per call: the same sum in the same order)
        if statistical:
            got = _moments(make, lv)
            _stated_tolerance(ref[0], ref[1], got[0], got[1], npx)


# ---- a. mesh frames ------------------------------------------------------------------------------------------------------------------------


def _frame_walk(walk, plan):
    """what a frame takes for a mesh whose walk under the default plan is `walk`, by the rules of tests/test_gpu_mesh_walks.py::expect"""
    if walk == "loop" or plan == "no_bvh":
        return "loop"
    return "skip" if plan in ("no_wide", "no_mesh_split") else walk


@pytest.mark.parametrize("dof", [0, 1])
@pytest.mark.parametrize("plan", list(mw.PLANS))
@pytest.mark.parametrize("name", MESH_FRAMES)
def test_mesh_frames_at_levels_1_and_2(gpu_product, O, monkeypatch, name, plan, dof):
    d, walks = mw.frame_scene(O, name)
    assert d["cam_ints"][0] * d["cam_ints"][1] == 64 * 48 and d["cam_ints"][3] == 4
    trees = any(w != "loop" for w in walks.values()) and plan != "no_bvh"

    def make(**opt):
        return mw.open_tracer(gpu_product, monkeypatch, d, plan, depth_of_field=dof, **opt)

    def check_variant(lv):
        with make(arith=lv) as T:
            for g, w in walks.items():
                pl = T.mesh_plan(g)
                assert pl["frame_walk"] == _frame_walk(w, plan) and bool(pl["split"]) == (trees and plan != "no_mesh_split"), (lv, g, pl)
            T.set_kernel_timing(True)
            T.render(1, 2)
            launches = T.kernel_times()["k_mesh"][1]
            if plan != "no_wide":                # (without four-wide nodes k_mesh has nothing to walk: whether it is launched is the plan's business)
                assert (launches > 0) == (trees and plan != "no_mesh_split"), (lv, launches)

    check_case(make, 64 * 48, check_variant)


# ---- b. one case per remaining path ----------------------------------------------------------------------------------------------------------
def _many_materials_text():
    """tests/test_gpu_parity.py::test_edge_many_materials' scene: 70 materials (more bins than lanes in a wave), 40 geoms (more than the 32
    a candidate mask holds)"""
    rng = np.random.default_rng(12)
    text, nm = "", 70
    for m in range(nm):
        kind = m % 7
        rgb = rng.uniform(0.2, 0.95, 3)
        refl, refr, ior, emit = (1, 0, 0, 0) if kind == 3 else (0, 1, 1.3 + 0.01 * m, 0) if kind == 5 else (0, 0, 0, 4 if kind == 0 else 0)
        text += MAT % ((m,) + tuple(rgb) + tuple(rgb[::-1]) + (refl, refr, ior, emit))
    text += CAMERA_BLOCK
    text += "OBJECT 0\ncube\nmaterial 1\nTRANS 0 0 0\nROTAT 0 0 0\nSCALE 12 .01 12\n\n"
    text += "OBJECT 1\ncube\nmaterial 0\nTRANS 0 10 0\nROTAT 0 0 0\nSCALE 8 .3 8\n\n"
    for k in range(2, 40):
        typ = "sphere" if k % 2 else "cube"
        pos = rng.uniform([-4.5, 0.5, -4.5], [4.5, 8.5, 2.0])
        rot = rng.uniform(0, 90, 3)
        sc = rng.uniform(0.4, 1.6, 3)
        text += "OBJECT %d\n%s\nmaterial %d\nTRANS %g %g %g\nROTAT %g %g %g\nSCALE %g %g %g\n\n" % ((k, typ, int(rng.integers(0, nm))) + tuple(pos) + tuple(rot) + tuple(sc))
    return text


@pytest.mark.parametrize("name", list(PATHS))
def test_remaining_paths_at_levels_1_and_2(gpu_product, monkeypatch, tmp_path, name):
    pt = gpu_product
    scene, res, depth, options, switch, refusal = PATHS[name]
    if scene is None:
        s = _scene_from_text(pt, _many_materials_text(), tmp_path, res=res, depth=depth)
        assert s.num_materials == 70 and s.num_geoms == 40
    else:
        s = pt.Scene(os.path.join(ROOT, "scenes", scene), res=res, depth=depth)
        s.apply_runcuda_camera()
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")          # (PTX_DEBUG_FORCE_FAST: a launch outside the variant's preconditions would be an error)

    def make(**opt):
        kw = dict(options); kw.update(opt)
        return pt.Tracer(s, **kw)

    def check_variant(lv):
        with make(arith=lv) as T:
            mesh = [g for g in range(s.num_geoms) if s.dump()["geom_ints"][g][0] == 3]
            if name.startswith("textured_mesh"):
                split = name.endswith("_split")
                assert all(bool(T.mesh_plan(g)["split"]) == split and T.mesh_plan(g)["root"] >= 0 for g in mesh) and mesh
                assert len(s.dump()["textures"]) == 4
                T.set_kernel_timing(True)
                T.render(1, 2)
                assert (T.kernel_times()["k_mesh"][1] > 0) == split
            if name in ("no_cull", "bins70_geoms40"):
                # (no candidate masks: the production intersect's test entry says so)
                p = T.generate(1)
                with pytest.raises(pt.PathTracerError):
                    T.tile_intersect(p[:256])
            if name == "row_tile":
                assert 0 < T.owned_pixels() < res[0] * res[1]
            if name == "apps_variant":
                T.render(1, 2)
                assert T.read_albedo().any()
        if refusal:
            monkeypatch.setenv("PTX_DEBUG_FORCE_FAST", "1")
            try:
                with make(arith=lv) as T:
                    with pytest.raises(pt.PathTracerError) as e:
                        T.render(1, 2)
                    assert re.search("outside its preconditions.*(%s)" % refusal, str(e.value)), str(e.value)
            finally:
                monkeypatch.delenv("PTX_DEBUG_FORCE_FAST")

    with make(arith=0) as T:
        npx = T.owned_pixels()
    # (one iteration per launch set on one lane adds into the image directly, outside the specialised kernel's preconditions: forced, the
    # comparison's base is one iteration per launch set on two lanes)
    check_case(make, npx, check_variant, base=dict(batch=1, lanes=2) if switch == "PTX_DEBUG_FORCE_FAST" else dict(batch=1, lanes=1))
