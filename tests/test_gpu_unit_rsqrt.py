"""GPU: two routines of pt_device.h that change how a cube / sphere pair is computed and must not change one bit of it.

pt_rsqrt_unit: getPointOnRay's second normalize of an already normalized direction takes 1 / sqrt(s) for s within W ulps of 1 from an integer
mapping of s's bits (tests/test_unit_rsqrt.py: the mapping on the CPU) and pt_rsqrt_glm for everything else.  pt_div_pairs3: the slab test's two
quotients per axis share the reciprocal seed and its Newton step where the compiler's own expansion would neither scale nor fix up, and are
the divisions elsewhere.

Known answers (ptx_kat_unit_rsqrt, on the device): pt_rsqrt_unit against pt_rsqrt_glm on ALL 2^32 operands (so everything within 4 W of 1.0f, every
fall-through and far more than 2^24 random patterns); pt_div_pairs3 against a / d on every pair of exponents for numerator and denominator with
random mantissas, on every triple of zeros, infinities, NaNs, subnormals and the guard's bounds, and on 2^26 random sets from the slab loop's range
(|a| <= 64, 2^-40 <= |d| <= 1).  No operand is excluded; nothing may differ (two NaNs count as equal, as in ptx_kat_fast_exact).

Frames: cornellObj.txt, cornellGlass.txt (spheres, glass) and cornellSpaceship.txt (the split mesh search) at 96 x 64 -- full tiles, a partial
last tile, tiles with and without mesh candidates --, depth 4, two iterations, sorted and unsorted, arithmetic levels 0 and 1, each with the
routines and under PTX_DEBUG_NO_UNIT_RSQRT (the code objects built without them: the arithmetic before this change).  The two runs must agree in
every bit of the frame, the rays per bounce and the fence counter; at level 0 both must also equal the CPU oracle.  (Level 1 promises the
oracle a statistical tolerance only, tests/test_gpu_arith.py: its bit-level reference here is the other variant.)"""
import os

import numpy as np
import pytest

from conftest import ROOT, beq
from test_gpu_parity import O, fences_stay_silent      # noqa: F401  (fixtures; the fence check is autouse)

pytestmark = pytest.mark.gpu
RES, DEPTH, ITERS = (96, 64), 4, 2
SCENES = ["cornellObj", "cornellGlass", "cornellSpaceship"]
_oracle = {}      # (scene, sorted) -> (frame, rays per bounce): computed once, shared by the two levels


def test_unit_rsqrt_and_slab_quotients_equal_what_they_replace_on_every_operand(gpu_product):
    pt = gpu_product
    s = pt.Scene(os.path.join(ROOT, "scenes", "sphere.txt"), res=(32, 32), depth=2)
    s.apply_runcuda_camera()
    with pt.Tracer(s) as T:
        rsqrt_bad, in_window, quot_bad, through_core = T.kat_unit_rsqrt(exponent_reps=64, random_sets=1 << 26)
    print("pt_rsqrt_unit: %d of 2^32 operands differ, %d inside the window; slab quotients: %d differ, %d sets through the shared reciprocal"
          % (rsqrt_bad, in_window, quot_bad, through_core))
    assert rsqrt_bad == 0
    assert in_window == 2 * 14 + 1                       # W = 14 (pt_device.h: PT_UNIT_W): the window is there and as wide as the CPU test says
    assert quot_bad == 0
    assert through_core > 1 << 26                        # every random set is in range, and part of the exponent grid: the core was what ran


def dump(pt, name):
    s = pt.Scene(os.path.join(ROOT, "scenes", name + ".txt"), res=RES, depth=DEPTH)
    s.apply_runcuda_camera()
    return s.dump()


def oracle_frame(O, d, name, sort):
    if (name, sort) not in _oracle:
        O.set_libm(1)
        O.create(d, d["textures"])
        O.set_options(aa=1, dof=0, sort=sort, cache=1)
        O.pt_init()
        for it in range(1, ITERS + 1):
            O.iterate(it)
        img = O.image().copy()
        img.setflags(write=False)
        _oracle[(name, sort)] = (img, O.live_counts().tolist())
    return _oracle[(name, sort)]


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("sort", [1, 0])
@pytest.mark.parametrize("name", SCENES)
def test_frames_with_the_routines_and_without(gpu_product, O, monkeypatch, name, sort, level):
    pt = gpu_product
    d = dump(pt, name)
    assert tuple(d["cam_ints"][:2]) == RES and int(d["cam_ints"][3]) == DEPTH
    assert RES[0] * RES[1] % 256 == 0 and (RES[0] * RES[1] // 256) > 1       # whole tiles, more than one workgroup's worth
    runs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("PTX_DEBUG_NO_UNIT_RSQRT", "1")
        else:
            monkeypatch.delenv("PTX_DEBUG_NO_UNIT_RSQRT", raising=False)
        with pt.Tracer.from_pod(d, arith=level, sort_by_material=sort) as T:
            if name == "cornellSpaceship":
                meshes = [g for g in range(len(d["geom_ints"])) if int(d["geom_ints"][g][0]) == 3]
                assert meshes and all(T.mesh_plan(g)["split"] for g in meshes)      # the split mesh search is what this scene is here for
            T.render(1, ITERS)
            runs.append((T.read_image(), T.stats()))
    monkeypatch.delenv("PTX_DEBUG_NO_UNIT_RSQRT", raising=False)
    (img, st), (img_off, st_off) = runs
    print(name, "sorted" if sort else "unsorted", "level", level, "rays per bounce", st["rays_per_bounce"], "fenced", st["fenced"], st_off["fenced"])
    assert img.any()
    assert beq(img, img_off), "%d of %d pixels differ between the two variants" % (int((img != img_off).any(axis=1).sum()), len(img))
    assert st["rays_per_bounce"] == st_off["rays_per_bounce"]
    assert st["fenced"] == 0 and st_off["fenced"] == 0
    if level == 0:
        want, counts = oracle_frame(O, d, name, sort)
        for how, (im, s_) in zip(("with the routines", "without"), runs):
            assert beq(im, want), "%s: %d of %d pixels differ from the oracle" % (how, int((im != want).any(axis=1).sum()), len(im))
            assert s_["rays_per_bounce"][:len(counts)] == counts and not any(s_["rays_per_bounce"][len(counts):]), (how, s_["rays_per_bounce"], counts)
