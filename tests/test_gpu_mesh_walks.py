"""GPU: the adversarial meshes of the host tier (tests/meshcases.py, tests/test_bvh.py) through EVERY walk the device has for a mesh,
against the oracle's loop over all faces, bit for bit (oracle in libm mode 1, level 0 kernels, no tolerance anywhere).

A mesh can be answered on the device in six ways, and ptx_debug_mesh_plan (Tracer.mesh_plan) says which one a call takes:
  wide_refill   k_mesh's refilling four-wide walk                         frames of a split scene, trees whose wide walk fits bvh_stack
  k_finish      the meshes k_mesh leaves in `rest`: skip links or loop    frames of a split scene, trees too deep / meshes without a tree
  wide          the single-lane four-wide walk (meshKey with a stack)      tile_intersect(split=True)
  ordered       the front-to-back binary walk (meshKey with a stack)       tile_intersect(split=True), wide walk does not fit or is off
  skip          the stackless skip-link walk                              geom_test, compute_intersections, tile_intersect(split=False),
                                                                           frames of an unsplit scene with trees
  loop          the plain loop over the faces                              meshes without a tree: fused in k_bounce (chunked over lanes,
                                                                           from the LDS triangle table or from global memory)
EXPECT below states, per case and plan, the walk each call must take; every test asserts the plan query against it, and the assertion
under the table says that the table reaches all six.  The properties the expectations rest on (chain: wide stack need 34 > 32 with a
binary depth of 29; chain_deep: need 40, depth 35; the duplicates and degenerate triangles never win ...) are asserted on the host, without a
GPU, by the fixture tests of tests/test_bvh.py.

Part a (intersection level): tile_intersect split / unsplit, compute_intersections and geom_test on the case's own rays taken to world
space, the far-origin sweep, axis-parallel rays in object and in world space.  Part b (frame level, the only route into k_mesh's
refilling schedule and k_finish): 64x48 frames, depth 4, 2 iterations, with and without depth of field; image, rays per bounce and the
sorted stream after every bounce.  Every tracer closed must have fenced nothing (test_gpu_parity's fence check)."""
import ctypes as C

import numpy as np
import pytest

import meshcases as mc
from conftest import beq, golden
from cpulibs import PATH_DTYPE
from test_gpu_parity import O, check_sorted_streams, fences_stay_silent      # noqa: F401  (fixtures; the fence check is autouse)

pytestmark = pytest.mark.gpu

PLANS = {"default": {}, "no_mesh_split": dict(no_mesh_split=1), "no_bvh": dict(no_bvh=1), "no_wide": {}}      # no_wide: PTX_DEBUG_NO_WIDE_BVH=1

# transforms (translation, rotation in degrees, scale): rotations about all three axes, non-uniform scales, the cottage's 0.02
TRS_ROT = (0.3, 5.0, -0.5, 25.0, 40.0, -15.0, 1.2, 0.8, 1.0)
TRS_ROT2 = (-0.5, 4.0, 0.5, -70.0, 10.0, 130.0, 0.7, 1.3, 0.9)
TRS_FLAT = (0.2, 5.0, -0.4, 0.0, 0.0, 0.0, 1.25, 0.5, 0.75)       # no rotation: an object-space axis stays an exact axis on the device
TRS_SMALL = (0.5, 5.0, 1.0, 10.0, 20.0, 30.0, 0.02, 0.02, 0.02)
TRS_CHAIN = (0.0, 1.0, 0.0, 15.0, -35.0, 20.0, 1.0, 1.1, 0.9)


def _case(name):
    """-> dict(faces, rays (object space), trs, texture (bool), size = the mesh's extent for the far-origin sweep, None: no sweep)"""
    if name == "hull":
        rng = np.random.default_rng(101)
        return dict(faces=mc.hull(16, 32), rays=np.concatenate([mc.rays_around(rng, 5000, 6.0, 1.5), mc.rays_around(rng, 1500, 0.2, 2.0)]), trs=TRS_ROT, size=3.0)
    if name == "hull_small_scale":
        rng = np.random.default_rng(103)
        return dict(faces=mc.hull(16, 32), rays=mc.rays_around(rng, 6000, 6.0, 1.5), trs=TRS_SMALL, size=3.0)
    if name == "soup":
        rng = np.random.default_rng(11)
        faces, n = mc.soup(rng, 2800)
        return dict(faces=faces, rays=mc.rays_around(rng, 10000, 5.0, 2.0), trs=TRS_ROT, size=4.0)
    if name == "soup_nan":
        faces, rays, n = mc.soup_nan(np.random.default_rng(43), n_rays=10000)
        return dict(faces=faces, rays=rays, trs=TRS_ROT2, texture=True, size=4.0)
    if name in ("flat_grid", "flat_grid_rot"):
        rng = np.random.default_rng(13)
        faces, xs = mc.flat_grid(28)                          # 3136 triangles
        return dict(faces=faces, rays=mc.flat_grid_rays(rng, xs, 2500), trs=TRS_FLAT if name == "flat_grid" else TRS_ROT2, size=4.0)
    if name == "needles":
        rng = np.random.default_rng(17)
        faces, tri = mc.needles(rng, 1500)
        return dict(faces=faces, rays=mc.needles_rays(rng, tri, 5000, 2000, 4000), trs=TRS_ROT, size=2.0)
    if name == "far_soup":
        rng = np.random.default_rng(19)
        return dict(faces=mc.far_soup(rng, 800), rays=mc.rays_around(rng, 6000, 3.0, 1.0), trs=TRS_ROT2, size=2.0)
    if name == "chain":
        faces, rays = mc.chain_case(np.random.default_rng(31))
        return dict(faces=faces, rays=rays, trs=TRS_CHAIN, size=None)
    if name == "chain_deep":
        faces, rays = mc.chain_deep_case(np.random.default_rng(31))
        return dict(faces=faces, rays=rays, trs=TRS_CHAIN, size=None)
    if name == "coincident":
        faces, rays = mc.coincident(np.random.default_rng(41))
        return dict(faces=faces, rays=rays, trs=TRS_ROT, size=2.0)
    if name.startswith("hull_cut"):
        k = int(name[8:])
        return dict(faces=mc.hull_cut(k), rays=mc.hull_cut_rays(np.random.default_rng(47 + k)), trs=TRS_ROT2, size=3.0)
    raise KeyError(name)


CASES = ["hull", "hull_small_scale", "soup", "soup_nan", "flat_grid", "flat_grid_rot", "needles", "far_soup", "chain", "chain_deep", "coincident",
         "hull_cut23", "hull_cut24", "hull_cut25"]
NO_TREE = {"hull_cut23"}                       # fewer than BVH_MIN_FACES faces
WIDE_TOO_DEEP = {"chain", "chain_deep"}        # four-wide stack need > BVH_STACK (tests/test_bvh.py measures 34 and 40)
BINARY_TOO_DEEP = {"chain_deep"}               # binary depth >= BVH_STACK (35)


def expect(case, plan):
    """(split, frame_walk, stack_walk) of a scene whose only mesh is `case`, by the rules of pt_prepare_scene / k_mesh / meshKey"""
    tree = case not in NO_TREE and plan != "no_bvh"
    if not tree:
        return False, "loop", "loop"
    wide = plan != "no_wide" and case not in WIDE_TOO_DEEP
    split = plan != "no_mesh_split"
    return split, ("wide_refill" if split and wide else "skip"), ("wide" if wide else "ordered" if case not in BINARY_TOO_DEEP else "skip")


EXPECT = {(c, p): expect(c, p) for c in CASES for p in PLANS}
# every entry of the list at the top is reached by some (case, plan): the refilling walk, k_finish's fallback with a tree (split, not
# wide_refill) -- its loop is scene 7 of part b --, the single-lane wide walk, the ordered walk natively (chain) and by the switch, the
# skip links with a stack in hand (chain_deep), the skip links of an unsplit frame, the plain loop
assert {e[1:] for e in EXPECT.values()} >= {("wide_refill", "wide"), ("skip", "wide"), ("skip", "ordered"), ("skip", "skip"), ("loop", "loop")}
assert any(e[0] and e[1] == "skip" for e in EXPECT.values()) and EXPECT[("chain", "default")] == (True, "skip", "ordered")
assert any(not e[0] and e[1] == "skip" for e in EXPECT.values())


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def box_geoms():
    """the lit Cornell box of tests/golden/loader_cornell.npz without its sphere: light, floor, ceiling, back, left, right (all cubes)"""
    g = golden("loader_cornell.npz")
    return [("cube", int(g["geom_ints"][i][1]), tuple(float(x) for x in g["geom_trs"][i])) for i in range(6)], g["materials"].copy()


def make_scene(O, geoms, materials, res=(64, 48), depth=4, eye=(0.0, 5.0, 10.5), lookat=(0.0, 5.0, 0.0), textures=None):
    """geoms: ("cube" | "sphere", material, trs9) or ("mesh", material, trs9, faces) -> the POD dict Tracer.from_pod / OracleLib.create take"""
    kind = dict(sphere=0, cube=1, mesh=3)
    gi = np.array([[kind[g[0]], g[1], len(g[3]) if g[0] == "mesh" else 0] for g in geoms], np.int32)
    trs = np.array([g[2] for g in geoms], np.float32)
    gm = np.stack([O.build_transforms(t) for t in trs])
    faces = [np.ascontiguousarray(g[3], np.float32) if g[0] == "mesh" else np.zeros((0, 15), np.float32) for g in geoms]
    cf = O.camera_from_loader(res[0], res[1], 45.0, eye, lookat, (0.0, 1.0, 0.0))
    O.lib.o_runcuda_camera(cf.ctypes.data_as(C.c_void_p))
    return dict(geom_ints=gi, geom_trs=trs, geom_mats=gm, materials=np.ascontiguousarray(materials, np.float32), faces=faces,
                cam_ints=np.array([res[0], res[1], 10, depth], np.int32), cam_floats=cf, textures=textures or {})


def checker_texture(seed):
    return np.random.default_rng(seed).integers(0, 256, size=(8, 8, 3)).astype(np.uint8)


def to_world(d, gi, rays):
    """object-space rays of geom gi -> world space (float64 products, rounded once)"""
    M = d["geom_mats"][gi][:16].astype(np.float64).reshape(4, 4).T
    o = rays[:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    dd = rays[:, 3:6].astype(np.float64) @ M[:3, :3].T
    return np.concatenate([o, dd], axis=1).astype(np.float32)


def reaches_box(d, gi, paths):
    """which rays (PATH_DTYPE records) reach the world box of mesh geom gi: plain slab test in float64"""
    v = d["faces"][gi].reshape(-1, 5)[:, :3]
    w = to_world(d, gi, np.concatenate([v, np.zeros_like(v)], axis=1))[:, :3].astype(np.float64)
    lo, hi = w.min(axis=0), w.max(axis=0)
    o, dd = paths["origin"].astype(np.float64), paths["direction"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / dd, (hi - o) / dd
    tn, tf = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
    return (tf >= tn) & (tf >= 0)


def kat_paths(rays):
    p = np.zeros(len(rays), PATH_DTYPE)
    p["origin"], p["direction"] = rays[:, :3], rays[:, 3:6]
    p["color"] = 1.0
    p["pixelIndex"] = np.arange(len(rays)); p["remainingBounces"] = 4
    return p


@pytest.fixture()
def threads16(O):
    O.set_threads(16)
    try:
        yield
    finally:
        O.set_threads(1)


def oracle_for(O, d, aa=1, dof=0):
    O.set_libm(1)
    O.create(d, d["textures"])
    O.set_options(aa=aa, dof=dof, sort=1, cache=1)
    O.pt_init()


def open_tracer(pt, monkeypatch, d, plan, **opt):
    if plan == "no_wide":
        monkeypatch.setenv("PTX_DEBUG_NO_WIDE_BVH", "1")
    else:
        monkeypatch.delenv("PTX_DEBUG_NO_WIDE_BVH", raising=False)
    kw = dict(PLANS[plan]); kw.update(opt)
    return pt.Tracer.from_pod(d, **kw)


# ---- a. intersection level -------------------------------------------------------------------------------------------------------------
_REF = {}        # per case: the scene, the world-space rays and the oracle's answers, computed once and shared by the four plans (read only)


def reference(O, name):
    if name in _REF:
        return _REF[name]
    c = _case(name)
    assert len(c["faces"]) <= 3520
    box, mats = box_geoms()
    geoms = box + [("mesh", 1, c["trs"], c["faces"])]
    gi = len(geoms) - 1
    tex = {(gi, 0): checker_texture(5)} if c.get("texture") else None
    d = make_scene(O, geoms, mats, textures=tex)
    rng = np.random.default_rng(977)
    f = c["faces"].reshape(-1, 3, 5)[:, :, :3].astype(np.float64)
    f = f[np.isfinite(f).all(axis=(1, 2))]
    lo, hi = f.min(axis=(0, 1)), f.max(axis=(0, 1))
    size = c["size"] or float(np.abs(c["rays"][:, :3]).max())
    obj = [c["rays"], mc.axis_parallel_rays(rng, 150, lo, hi)]                     # the case's own; object-space axes (exact under TRS_FLAT)
    if c["size"]:
        obj.append(mc.far_rays(rng, 400, c["size"]))                               # 10^3 .. 10^6 mesh sizes away
    world = [to_world(d, gi, np.concatenate(obj))]
    wlo, whi = np.array([-5.0, 0.0, -5.0]), np.array([5.0, 10.0, 5.0])
    world.append(mc.axis_parallel_rays(rng, 150, wlo, whi))                        # world-space axes: zero components in the box tests and the candidate masks
    rays = np.concatenate(world).astype(np.float32)
    assert len(rays) <= 40000
    oracle_for(O, d)
    O.set_threads(16)
    try:
        want = O.compute_intersections(kat_paths(rays))
        want_geom = O.geom_test(gi, rays)
    finally:
        O.set_threads(1)
    _REF[name] = dict(d=d, gi=gi, rays=rays, want=want, want_geom=want_geom, size=size)
    return _REF[name]


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("case", CASES)
def test_every_walk_at_intersection_level(gpu_product, O, monkeypatch, case, plan):
    r = reference(O, case)
    d, gi, rays, want, want_geom = r["d"], r["gi"], r["rays"], r["want"], r["want_geom"]
    p = kat_paths(rays)
    hit = want["t"] > 0
    mine = hit & (want["geomId"] == gi)
    ghit = want_geom[:, 0] > 0
    # no case passes vacuously: the mesh itself is hit, and (unless the scale makes it lose every comparison of its object-space distance
    # with the box's world-space ones, the cottage's situation) it wins rays of the whole scene
    assert ghit.sum() > 200, ghit.sum()
    assert mine.sum() > (50 if case != "hull_small_scale" else -1), mine.sum()
    fields = ("t", "normal", "materialId", "geomId") + (("texcoord",) if d["textures"] else ())
    with open_tracer(gpu_product, monkeypatch, d, plan) as T:
        plan_got = T.mesh_plan(gi)
        split, frame_walk, stack_walk = EXPECT[(case, plan)]
        print(case, plan, plan_got, "rays", len(rays), "mesh hit by", int(ghit.sum()), "wins", int(mine.sum()))
        assert (bool(plan_got["split"]), plan_got["frame_walk"], plan_got["stack_walk"]) == (split, frame_walk, stack_walk), plan_got
        assert (plan_got["root"] >= 0) == (frame_walk != "loop")
        if case in WIDE_TOO_DEEP and plan != "no_bvh":
            assert plan_got["depth"] >= 29 and (plan_got["wneed"] > mc.BVH_STACK or plan == "no_wide")
            assert plan_got["bvh_stack"] == (8 if case in BINARY_TOO_DEEP else plan_got["depth"] + 1)
        bad = []

        def same(label, got, ref, rows=None):
            """bitwise; what differs is reported in full (how many rays, which, from how far) after every entry point has run"""
            g, w = (got, ref) if rows is None else (got[rows], ref[rows])
            if not beq(g, w):
                g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
                diff = (g.view(np.uint32).reshape(len(g), -1) != w.view(np.uint32).reshape(len(w), -1)).any(axis=1)
                idx = (np.arange(len(rays)) if rows is None else np.nonzero(rows)[0])[diff]
                bad.append("%s: %d rays differ, first %s, |origin| %s, got %s want %s" % (label, len(idx), idx[:6].tolist(),
                           np.linalg.norm(rays[idx[:6], :3], axis=1).tolist(), g[diff][:3].tolist(), w[diff][:3].tolist()))

        # tileIntersect with the mesh tests inside (skip links, or the loop: chunked / from LDS / from global memory)
        got = T.tile_intersect(p, split=False)
        for f in fields:
            same("tile_intersect(split=False) " + f, got[f], want[f], None if f == "t" else hit)
        # the split search's pieces: pass 1 without meshes, meshKey WITH a stack (wide / ordered / skip as the plan says), decodeKey
        if plan_got["root"] >= 0:
            got = T.tile_intersect(p, split=True)
            for f in fields:
                same("tile_intersect(split=True) [%s] %s" % (stack_walk, f), got[f], want[f], None if f == "t" else hit)
        else:
            with pytest.raises(gpu_product.PathTracerError):
                T.tile_intersect(p[:256], split=True)                  # (no tree anywhere: nothing for the split search to do, said as an error)
        same("compute_intersections t", T.compute_intersections(p)["t"], want["t"])      # intersectScene: one lane per ray, skip links or loop
        out = T.geom_test(gi, rays)                                   # k_kat_geom: meshIntersectionTest with a root and no stack
        same("geom_test t", out[:, 0], want_geom[:, 0])
        same("geom_test hits", out, want_geom, ghit)
        assert not bad, "\n".join(bad)
    # (ties: soup_nan's duplicates carry texcoords of their own, so the texcoords above -- tile_intersect's and columns 7-8 of geom_test --
    # equal the oracle's only if the LOWER face index won every tie, as in the loop; the host tier asserts that ties occur)


# ---- b. frame level --------------------------------------------------------------------------------------------------------------------
FRAME_CAM = dict(eye=(0.0, 5.0, 6.0), lookat=(0.0, 4.0, 0.0))        # inside the room's open side, looking slightly down


def frame_scene(O, name):
    """-> (POD dict, mesh geom indices, {geom: (frame_walk under the default plan)}, extra assertions on the oracle's first hits)"""
    box, mats = box_geoms()
    rng = np.random.default_rng(2024)
    hull = mc.hull(12, 24)                                            # 576 triangles
    if name == "soup_nan":
        faces, _, _ = mc.soup_nan(np.random.default_rng(43), n_rays=1)
        geoms = box + [("mesh", 2, TRS_ROT, faces)]
        return make_scene(O, geoms, mats, textures={(6, 0): checker_texture(5)}, **FRAME_CAM), {6: "wide_refill"}
    if name in ("chain", "chain_deep"):
        faces, _ = (mc.chain_case if name == "chain" else mc.chain_deep_case)(np.random.default_rng(31), 1)
        return make_scene(O, box + [("mesh", 3, TRS_CHAIN, faces)], mats, **FRAME_CAM), {6: "skip"}
    if name == "chain_and_hull":
        faces, _ = mc.chain_case(np.random.default_rng(31), 1)
        geoms = box + [("mesh", 3, TRS_CHAIN, faces), ("mesh", 2, (-1.0, 4.0, -1.0, 20.0, 30.0, 40.0, 2.0, 2.5, 2.0), hull)]
        return make_scene(O, geoms, mats, **FRAME_CAM), {6: "skip", 7: "wide_refill"}
    if name == "grazing_grid":
        faces, _ = mc.flat_grid(28)
        geoms = box + [("mesh", 2, (0.0, 5.0, 0.0, 0.0, 0.0, 0.0, 2.0, 1.0, 2.0), faces)]
        return make_scene(O, geoms, mats, eye=(0.0, 5.03, 6.0), lookat=(0.0, 5.0, 0.0)), {6: "wide_refill"}
    if name == "twins":
        trs = (0.0, 4.0, 0.0, 30.0, 20.0, 10.0, 2.0, 2.5, 2.0)
        return make_scene(O, box + [("mesh", 2, trs, hull), ("mesh", 3, trs, hull)], mats, **FRAME_CAM), {6: "wide_refill", 7: "wide_refill"}
    if name == "geoms32":
        # BVH meshes at geom indices 0 and 31 (the top bit of every per-geom mask), the box and 24 small cubes and spheres in between
        fill = []
        for k in range(24):
            pos = rng.uniform([-4.0, 0.5, -4.0], [4.0, 9.0, 3.0])
            fill.append(("sphere" if k % 3 == 0 else "cube", int(rng.integers(1, 5)), tuple(pos) + tuple(rng.uniform(-90, 90, 3)) + tuple(rng.uniform(0.3, 0.9, 3))))
        geoms = [("mesh", 2, (-2.0, 4.0, 0.0, 20.0, 30.0, 40.0, 1.0, 1.5, 1.0), hull)] + box + fill + \
                [("mesh", 3, (2.0, 5.5, 0.5, -40.0, 10.0, 70.0, 1.2, 1.0, 1.4), mc.hull(10, 20))]
        assert len(geoms) == 32
        return make_scene(O, geoms, mats, **FRAME_CAM), {0: "wide_refill", 31: "wide_refill"}
    if name == "boundary":
        # 23, 24 and 25 faces side by side: the first has no tree and rides through k_mesh's `rest` into k_finish's plain loop
        geoms = box + [("mesh", 2, (-2.5, 5.0, 0.0, 20.0, 30.0, 40.0, 1.0, 1.5, 1.0), mc.hull_cut(23)),
                       ("mesh", 3, (0.0, 5.0, 0.0, 20.0, 30.0, 40.0, 1.0, 1.5, 1.0), mc.hull_cut(24)),
                       ("mesh", 2, (2.5, 5.0, 0.0, 20.0, 30.0, 40.0, 1.0, 1.5, 1.0), mc.hull_cut(25))]
        return make_scene(O, geoms, mats, **FRAME_CAM), {6: "loop", 7: "wide_refill", 8: "wide_refill"}
    if name == "boundary23_alone":
        return make_scene(O, box + [("mesh", 2, (0.0, 5.0, 0.0, 20.0, 30.0, 40.0, 1.5, 2.0, 1.5), mc.hull_cut(23))], mats, **FRAME_CAM), {6: "loop"}
    raise KeyError(name)


FRAME_SCENES = ["soup_nan", "chain", "chain_deep", "chain_and_hull", "grazing_grid", "twins", "geoms32", "boundary", "boundary23_alone"]


def render_pair(pt, monkeypatch, O, d, plan="default", dof=0, iters=2, **opt):
    """2 iterations on the device and in the oracle: image bits and rays per bounce equal; -> (image, tracer still open)"""
    oracle_for(O, d, dof=dof)
    for it in range(1, iters + 1):
        O.iterate(it)
    T = open_tracer(pt, monkeypatch, d, plan, depth_of_field=dof, **opt)
    try:
        T.render(1, iters)
        img = T.read_image()
        assert beq(img, O.image()), "%d of %d pixels differ" % (int((img != O.image()).any(axis=1).sum()), len(img))
        want = O.live_counts().tolist()
        got = T.stats()["rays_per_bounce"]
        assert got[:len(want)] == want and not any(got[len(want):]), (got, want)
    except BaseException:
        T.close()
        raise
    return img, T


@pytest.mark.parametrize("name", FRAME_SCENES)
def test_frames_through_k_mesh_and_k_finish(gpu_product, O, monkeypatch, threads16, name):
    d, walks = frame_scene(O, name)
    depth = int(d["cam_ints"][3])
    assert d["cam_ints"][0] * d["cam_ints"][1] <= 64 * 48 and depth == 4
    splits = any(w != "loop" for w in walks.values())                # (a tree somewhere, candidate masks on: the split mesh search)
    # what the camera sees, from the oracle: every mesh of the scene is some pixel's first hit
    oracle_for(O, d)
    O.pt_generate(1)
    first = O.compute_intersections(O.paths())
    seen = {g: float(((first["t"] > 0) & (first["geomId"] == g)).mean()) for g in walks}
    print(name, "share of pixels whose first hit is geom g:", seen)
    if name == "twins":
        # every hit of the second copy ties with the first: the lower geom index wins all of them (the reference's strict t < tmin)
        assert seen[6] > 0.05 and seen[7] == 0.0
    elif name == "chain_and_hull":
        # rays that reach BOTH world boxes walk the hull in k_mesh and carry the chain in `rest` to k_finish: a share of the camera rays
        # does (slab test in float64 on the oracle's camera rays), and both meshes are somebody's first hit
        cam = O.paths()
        both = reaches_box(d, 6, cam) & reaches_box(d, 7, cam)
        print(name, "share of camera rays that reach both boxes: %.3f" % both.mean())
        assert both.mean() > 0.10
        assert seen[7] > 0.05 and seen[6] > 0.005
    else:
        assert all(v > 0.005 for v in seen.values()), seen
    img, T = render_pair(gpu_product, monkeypatch, O, d)
    with T:
        for g, w in walks.items():
            pl = T.mesh_plan(g)
            print(name, g, pl)
            assert pl["frame_walk"] == w and bool(pl["split"]) == splits, pl
        if name == "chain":
            assert T.mesh_plan(6)["bvh_stack"] == T.mesh_plan(6)["depth"] + 1 and T.mesh_plan(6)["wneed"] > mc.BVH_STACK
        if name == "chain_deep":
            assert T.mesh_plan(6)["bvh_stack"] == 8 and T.mesh_plan(6)["depth"] >= mc.BVH_STACK
        T.set_kernel_timing(True)
        T.reset_image()
        T.render(1, 2)
        launches = T.kernel_times()["k_mesh"][1]
        T.set_kernel_timing(False)
        assert (launches > 0) == splits, launches
        assert beq(T.read_image(), img)
        oracle_for(O, d)
        check_sorted_streams(T, O, d, depth)
    # the same scene with the mesh search inside the bounce kernel, one iteration per launch set
    img2, T2 = render_pair(gpu_product, monkeypatch, O, d, "no_mesh_split", batch=1)
    with T2:
        assert not T2.mesh_plan(list(walks)[0])["split"]
    assert beq(img2, img)
    # ... and with depth of field
    img3, T3 = render_pair(gpu_product, monkeypatch, O, d, dof=1)
    T3.close()
    assert not beq(img3, img)


@pytest.mark.parametrize("name,plan", [("soup_nan", "no_wide"), ("chain", "no_wide"), ("geoms32", "no_wide"), ("soup_nan", "no_bvh"), ("geoms32", "no_bvh"),
                                       ("boundary", "no_bvh")])
def test_frames_under_the_other_plans(gpu_product, O, monkeypatch, threads16, name, plan):
    """No four-wide nodes: k_mesh leaves every mesh to k_finish's skip-link walk.  No tree: the plain loop fused into k_bounce -- chunked
    over lanes, from the LDS triangle table (boundary: 72 triangles) or from global memory (soup: 3511)."""
    d, walks = frame_scene(O, name)
    _, T = render_pair(gpu_product, monkeypatch, O, d, plan)
    with T:
        for g in walks:
            pl = T.mesh_plan(g)
            if plan == "no_bvh":
                assert (pl["frame_walk"], pl["split"], pl["root"]) == ("loop", 0, -1), pl
            else:
                assert pl["frame_walk"] == ("skip" if walks[g] != "loop" else "loop") and pl["split"] == 1 and pl["wroot"] == -1, pl
