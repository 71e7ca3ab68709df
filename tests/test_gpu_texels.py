"""GPU: the texel lookups of the HIP path -- scatterRay's kd / ks / ke, the bump lookup of the mesh normal, the albedo AOV's copy --
against the CPU oracle bit for bit and against the plain-numpy rule (tests/texel_ref.py), at what the stand-in asset set (four
128 x 128 maps, UVs in [0.02, 0.98], one mesh, all maps present) cannot show: odd and non-square sizes, a different size per map, 3
and 4 channels, map subsets, coordinates on texel boundaries, outside [0, 1] and tiled, byte offsets beyond 2^24, a second textured
mesh, more than 32 geoms.  tests/test_texel_cpu.py proves the same inputs reach every class of lookup on the oracle alone;
tests/test_oracle_pin.py pins the oracle's use of widths and heights to the reference.  Arithmetic level 0, the oracle in the kernels'
libm mode."""
import os

import numpy as np
import pytest

import texel_ref as TR
import texelcases as TC
from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

RES, DEPTH = (96, 54), 8


@pytest.fixture()
def O(oracle_lib):
    oracle_lib.set_libm(1)
    yield oracle_lib
    oracle_lib.set_libm(0)


@pytest.fixture(autouse=True)
def fences_stay_silent(gpu_product):
    """As in test_gpu_parity.py: every tracer a test of this module closes must have fenced no index."""
    pt = gpu_product
    orig, seen = pt.Tracer.close, []

    def close(self):
        if getattr(self, "h", None):
            seen.append(self.stats()["fenced"])
        orig(self)
    pt.Tracer.close = close
    yield
    pt.Tracer.close = orig
    assert seen and not any(seen), "the kernels fenced %s indices" % seen


def _dump(pt, scene):
    s = pt.Scene(os.path.join(ROOT, "scenes", scene), res=RES, depth=DEPTH)
    s.apply_runcuda_camera()
    return s.dump()


@pytest.fixture(scope="module")
def ship(gpu_product):
    return _dump(gpu_product, "cornellSpaceship.txt")


@pytest.fixture(scope="module")
def cornell_obj(gpu_product):
    return _dump(gpu_product, "cornellObj.txt")


# --- shade known-answer grid -------------------------------------------------------------------------------------------------

def _shade_case(pt, O, ship, spec, sizes, seed):
    gi = TC.mesh_index(ship)
    uv = TC.uv_grid(sizes, seed)
    TC.grid_conditions(uv, spec)
    maps = TC.make_maps(spec, seed)
    d = TC.with_maps(ship, gi, maps)
    idx, isects, paths = TC.shade_inputs(d, gi, uv, seed + 1)
    O.create(d, d["textures"])
    want = O.shade(3, 1, idx, isects, paths)
    with pt.Tracer.from_pod(d) as T:
        got = T.shade(3, idx, isects, paths)
    material = d["materials"][d["geom_ints"][gi][1]]
    TC.assert_shaded_by_rule(got, paths, uv, maps, material)
    assert beq(got, want)


@pytest.mark.parametrize("name,spec", TC.shade_grid(), ids=[c[0] for c in TC.shade_grid()])
def test_shade_grid(gpu_product, O, ship, name, spec):
    """4096 synthetic intersections on the mesh per case (the inputs test_texel_cpu.py runs through the oracle): whole records equal the
    oracle's, lit lanes carry emission_colour and have ended, the others carry the ks or the kd tint, both on at least 5 % of them."""
    _shade_case(gpu_product, O, ship, spec, sorted({(w, h) for w, h, ch in spec.values()}), TC.case_seed(name))


def test_shade_with_byte_offsets_beyond_2_to_24(gpu_product, O, ship):
    """kd 4096 x 1400 x 3 (17.2 MB, generated, never written anywhere) ahead of a 9 x 5 ke map in the texel blob: ke's offset, and kd's
    last row and last texel, lie beyond 2^24 bytes."""
    assert 4096 * 1400 * 3 > 1 << 24
    _shade_case(gpu_product, O, ship, TC.LARGE_SPEC, [(4096, 1400), (9, 5)], 77)


# --- the bump lookup of the mesh normal -------------------------------------------------------------------------------------------

def _intersections_equal(T, O, d, p):
    """The plain loop, the tile search and the split mesh search against the oracle: distance and material on every ray, normal, geom and
    texcoords on every hit.  Texcoords of a hit on a cube or sphere are compared where they are defined: computeIntersections copies
    tmp_uv along with every new nearest hit (src/pathtrace.cu:314-324), so a cube that wins after a mesh was tested carries that mesh's
    last texcoords -- a value no shader reads, which the plain loop repeats and the tile search leaves at 0.  With every mesh behind
    every cube and sphere there is no such value and all hits are compared."""
    want = O.compute_intersections(p)
    hit = want["t"] > 0
    kinds = np.asarray(d["geom_ints"])[:, 0]
    meshes = np.nonzero(kinds == 3)[0]
    uv_defined = hit if meshes.min() > np.nonzero(kinds != 3)[0].max() else hit & (kinds[want["geomId"]] == 3)
    for name, got in (("loop", T.compute_intersections(p)), ("tile", T.tile_intersect(p, split=False)), ("split", T.tile_intersect(p, split=True))):
        assert beq(got["t"], want["t"]) and beq(got["materialId"], want["materialId"]), name
        for f in ("normal", "geomId"):
            assert beq(got[f][hit], want[f][hit]), (name, f)
        assert beq(got["texcoord"][uv_defined], want["texcoord"][uv_defined]), name
    return want


@pytest.mark.parametrize("tname", list(TC.UV_TRANSFORMS))
@pytest.mark.parametrize("w,h", TC.BUMP_SIZES)
def test_bump_lookup(gpu_product, O, ship, w, h, tname):
    """A bump map alone on the mesh, its face UVs as they are, stretched to [0, 1] exactly, and tiled into [-1, 2]: the plain loop, the
    tile search and the split mesh search give the oracle's distance, material, normal, geom and texcoords on 6000 rays aimed at the
    mesh; tiled, at least 100 of the lookups are clamped and at least 100 are not."""
    gi = TC.mesh_index(ship)
    a, b = TC.UV_TRANSFORMS[tname]
    d = TC.with_uv_transform(TC.with_maps(ship, gi, TC.make_maps({TC.BUMP: (w, h, 3 + (w + len(tname)) % 2)}, w * 100 + h)), gi, a, b)
    O.create(d, d["textures"])
    p = TC.mesh_rays(d, gi, 6000, 77)
    with gpu_product.Tracer.from_pod(d) as T:
        want = _intersections_equal(T, O, d, p)
    mesh = (want["t"] > 0) & (want["geomId"] == gi)
    assert mesh.sum() >= 500
    cls = TR.classes(want["texcoord"][mesh, 0], want["texcoord"][mesh, 1], w, h)
    if tname == "tiled":
        assert TR.clamped(cls).sum() >= 100 and TC.inner_count(cls, w, h) >= 100
    # the map is seen: without it the normals differ
    O.create(TC.without_maps(d), {})
    assert not beq(O.compute_intersections(p)["normal"][mesh], want["normal"][mesh])


@pytest.mark.parametrize("front", [False, True], ids=["appended", "as-geom-0"])
@pytest.mark.parametrize("bumped", ["twin", "ship"])
def test_bump_on_one_of_two_meshes(gpu_product, O, ship, bumped, front):
    """Two instances of the mesh, a bump map on one of them only: the tabulated normal of the one and the per-hit normal of the other
    in one scene, and texcoords carried for a mesh that has no map at all.  The second instance once behind the ship and once as geom 0."""
    gi = TC.mesh_index(ship)
    maps = TC.make_maps({TC.BUMP: (7, 3, 3)}, 21)
    if bumped == "twin":
        d = TC.with_second_mesh(O, TC.without_maps(ship), gi, TC.TWIN_TRS, maps, front)
    else:
        d = TC.with_second_mesh(O, TC.with_maps(ship, gi, maps), gi, TC.TWIN_TRS, {}, front)
    first, second = (0, gi + 1) if front else (gi, gi + 1)
    assert len(d["textures"]) == 1 and [int(k) for k in d["geom_ints"][[first, second], 0]] == [3, 3]
    O.create(d, d["textures"])
    p = np.concatenate([TC.mesh_rays(d, first, 3000, 78), TC.mesh_rays(d, second, 3000, 79)])
    with gpu_product.Tracer.from_pod(d) as T:
        want = _intersections_equal(T, O, d, p)
    for g in (first, second):
        assert ((want["t"] > 0) & (want["geomId"] == g)).sum() >= 500


# --- frames through the production kernels ---------------------------------------------------------------------------------------

def _oracle_frame(O, d, opt, iters=3):
    O.create(d, d["textures"])
    O.set_options(aa=1, dof=opt.get("depth_of_field", 0), sort=opt.get("sort_by_material", 1), cache=1)
    O.pt_init()
    for it in range(1, iters + 1):
        O.iterate(it)
    return O.image(), O.live_counts().tolist()


def _frame_equals_oracle(T, O, d, opt):
    want, counts = _oracle_frame(O, d, opt)
    T.render(1, 3)
    assert beq(T.read_image(), want)
    got = T.stats()["rays_per_bounce"]
    assert got[:len(counts)] == counts and not any(got[len(counts):])
    return want


@pytest.mark.parametrize("name,key,opt", TC.FRAME_CASES, ids=[c[0] for c in TC.FRAME_CASES])
def test_frames(gpu_product, O, ship, cornell_obj, name, key, opt):
    """96 x 54, depth 8, 3 iterations through the production kernels: image and rays per bounce equal the oracle's.  The maps are seen
    (the oracle's frame differs from the untextured scene's), and where the UVs are tiled the first bounce alone holds at least 50
    clamped lookups."""
    d = TC.frame_scene(O, key, ship, cornell_obj)
    if key == "34":
        assert len(d["geom_ints"]) == 34 and (len(d["geom_ints"]) - 1, TC.BUMP) in d["textures"] and (0, TC.BUMP) in d["textures"]
    with gpu_product.Tracer.from_pod(d, **opt) as T:
        want = _frame_equals_oracle(T, O, d, opt)
    plain = TC.without_maps(d)
    assert not beq(_oracle_frame(O, plain, opt)[0], want)
    if key == "tiled":
        O.create(d, d["textures"]); O.pt_init()
        O.pt_generate(1)
        assert TC.clamped_lookups(d, O.compute_intersections(O.paths())) >= 50


# --- the albedo AOV's own copy of the lookup -------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(7, 3), (64, 33)])
@pytest.mark.parametrize("subset", [(TC.KD,), (TC.KE,), (TC.KD, TC.KE)], ids=["kd", "ke", "kd+ke"])
def test_albedo(gpu_product, O, ship, subset, w, h):
    """apps_variant = 1: the albedo buffer and the image equal the oracle's; with kd and ke both, once more with the UVs tiled, so that
    the AOV's own index arithmetic meets coordinates outside the map."""
    gi = TC.mesh_index(ship)
    base = TC.with_maps(ship, gi, TC.make_maps({k: (w, h, 3 + (k + w) % 2) for k in subset}, 40 + w))
    scenes = [base] + ([TC.with_uv_transform(base, gi, *TC.UV_TRANSFORMS["tiled"])] if len(subset) == 2 else [])
    try:
        for d in scenes:
            O.create(d, d["textures"])
            O.set_options(aa=1, dof=0, sort=1, cache=1)
            O.set_apps_variant(1); O.pt_init()
            for it in (1, 2, 3):
                O.iterate(it)
            want_img, want_alb = O.image(), O.albedo()
            with gpu_product.Tracer.from_pod(d, apps_variant=1) as T:
                T.render(1, 3)
                assert beq(T.read_albedo(), want_alb) and beq(T.read_image(), want_img)
            plain = TC.without_maps(d)
            O.create(plain, {})
            O.set_apps_variant(1); O.pt_init()
            O.iterate(1)
            assert not beq(O.albedo(), want_alb)
    finally:
        O.set_apps_variant(0)


# --- from files -------------------------------------------------------------------------------------------------------------------

def test_scene_files_with_maps_of_different_sizes(gpu_product, O, tmp_path):
    """The stand-in ship with kd 64x33 (P6), ks 5x9 (RGBA PNG), ke 31x17 (PNG), bump 12x40 (P6) written to disk and loaded by the
    product's loader: each map arrives with its own (h, w, channels), rows bottom-up as the reference loads them, and the frame equals
    the oracle's."""
    path, written = TC.write_ship_scene(tmp_path, open(os.path.join(ROOT, "scenes", "cornellSpaceship.txt")).read())
    s = gpu_product.Scene(path, res=RES, depth=DEPTH)
    s.apply_runcuda_camera()
    d = s.dump()
    gi = TC.mesh_index(d)
    assert {k: v.shape for k, v in d["textures"].items()} == {(gi, w): img.shape for w, img in written.items()}
    assert all(np.array_equal(d["textures"][(gi, w)], img[::-1]) for w, img in written.items())
    with gpu_product.Tracer(s) as T:
        want = _frame_equals_oracle(T, O, d, {})
    assert not beq(_oracle_frame(O, TC.without_maps(d), {})[0], want)
