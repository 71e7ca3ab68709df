"""Inputs for the texture lookup tests (test_texel_cpu.py, test_gpu_texels.py, test_oracle_pin.py): map sizes, generated maps,
texture coordinates that reach every class of texel_ref.classes, synthetic intersections on a mesh, and edits of a scene's POD dict
(Scene.dump() / RefLib.dump() layout) -- map subsets, transformed face UVs, a second textured mesh, more than 32 geoms.  Everything
is seeded; nothing here calls the oracle or the product."""
import os

import numpy as np

import texel_ref as TR
from cpulibs import ISECT_DTYPE, PATH_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KD, KS, KE, BUMP = range(4)                     # the checkers' order of a geom's maps (cpulibs.py)
SIZES = [(1, 1), (1, 5), (5, 1), (7, 3), (3, 7), (64, 33), (255, 256)]          # (w, h)
SUBSETS = [(KD,), (KS,), (KE,), (KD, KS), (KD, KE)]
LANES = 4096
UV_TRANSFORMS = {"identity": (1.0, 0.0), "unit": (1 / 0.96, -0.02 / 0.96), "tiled": (3.0, -1.0)}
LARGE_SPEC = {KD: (4096, 1400, 3), KE: (9, 5, 3)}          # kd first in the blob: ke's offset lies beyond 2^24 bytes
BUMP_SIZES = [(1, 1), (7, 3), (12, 40)]


def shade_grid():
    """The shade grid's cases as (id, {which: (w, h, ch)}): every size under every subset, 3 and 4 channels alternating so that each size and
    each subset sees both, and all three maps at three different sizes -- 39 launches of 4096 records instead of the 84 of the product."""
    out = []
    for si, (w, h) in enumerate(SIZES):
        for ki, sub in enumerate(SUBSETS):
            ch = 3 + (si + ki) % 2
            out.append(("%dx%dx%d-%s" % (w, h, ch, "+".join("kd ks ke".split()[k] for k in sub)), {k: (w, h, ch) for k in sub}))
    for n, trio in enumerate([((64, 33, 3), (5, 1, 4), (7, 3, 3)), ((3, 7, 4), (255, 256, 3), (1, 5, 4)),
                              ((1, 1, 3), (7, 3, 4), (64, 33, 4)), ((255, 256, 4), (1, 5, 3), (1, 1, 4))]):
        out.append(("all-three-%d" % n, dict(zip((KD, KS, KE), trio))))
    return out


def case_seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) & 0x7fffffff


def random_map(rng, w, h, ch, which):
    """(h, w, ch) uint8.  kd / ks: any bytes.  ke: about 30 % of the texels black (colour bytes; a fourth channel stays random), at least
    one black and one lit texel when the map has two; a one-texel ke map is (r, 0, 0[, 0]): lit where the lookup lands inside the map and
    dark where the clamp makes all three channels read the last byte.  bump: bytes >= 1, so that no normal is 0 / 0."""
    img = rng.integers(1 if which == BUMP else 0, 256, (h, w, ch), dtype=np.uint8)
    if which == KE:
        flat = img.reshape(-1, ch)
        if len(flat) == 1:
            flat[0, 1:] = 0
            flat[0, 0] |= 1
        else:
            black = rng.random(len(flat)) < 0.3
            black[0], black[1] = True, False
            flat[~black, int(rng.integers(0, 3))] |= 1
            flat[black, :3] = 0
    return img


def make_maps(spec, seed):
    """{which: (w, h, ch)} -> {which: image}"""
    rng = np.random.default_rng(seed)
    return {k: random_map(rng, *spec[k], k) for k in sorted(spec)}


def _edges(n):
    """the texel boundaries k / n of a small map and their float32 neighbours"""
    k = np.arange(n + 1, dtype=np.float32) / np.float32(n)
    return np.concatenate([k, np.nextafter(k, np.float32(-np.inf)), np.nextafter(k, np.float32(np.inf))])


def _cell(rng, c, n, count):
    """coordinates that truncate to the integer c on an n-wide axis (trunc goes towards zero: the cell of c < 0 is (c - 1, c])"""
    f = rng.uniform(0.05, 0.95, count)
    return np.clip(np.where(c < 0, c - f, c + f) / n, -0.5, 1.5)


def uv_grid(sizes, seed, n=LANES):
    """(n, 2) float32 in [-0.5, 1.5]: for every (w, h) of `sizes` the structured points -- all pairs of +-0, 1, nextafter(1, 0) and -0.1
    (the corners among them), each of those and, for maps of at most 7 texels across, each texel boundary k / w and its two float32
    neighbours on one axis with the other axis random -- and 48 lookups aimed at each class the size admits; the rest random, 60 % from
    U(-0.5, 1.5)^2 and 40 % from U(0, 1)^2 (the wide draw alone leaves under 25 % inside a large map)."""
    rng = np.random.default_rng(seed)
    one = np.float32(1)
    base = np.array([0.0, -0.0, 1.0, np.nextafter(one, np.float32(0)), -0.1], np.float32)
    parts = [np.stack(np.meshgrid(base, base), -1).reshape(-1, 2)]
    for w, h in sizes:
        su = np.concatenate([base, _edges(w)]) if w <= 7 else base
        sv = np.concatenate([base, _edges(h)]) if h <= 7 else base
        reps = 6 if len(sizes) == 1 else 3
        parts.append(np.stack([np.repeat(su, reps), rng.uniform(-0.5, 1.5, reps * len(su))], -1))
        parts.append(np.stack([rng.uniform(-0.5, 1.5, reps * len(sv)), np.repeat(sv, reps)], -1))
        cu, cv = TR.lattice(w, h)
        labels = TR.classes_of_coords(cu, cv, w, h)
        for c in sorted(TR.admitted(w, h)):
            pick = rng.choice(np.nonzero(labels == c)[0], 48)
            parts.append(np.stack([_cell(rng, cu[pick], w, 48), _cell(rng, cv[pick], h, 48)], -1))
    fixed = np.concatenate(parts).astype(np.float32)
    assert len(fixed) <= n * 3 // 5, len(fixed)
    rest = n - len(fixed)
    wide = rng.uniform(-0.5, 1.5, (rest - rest * 2 // 5, 2))
    inside = rng.uniform(0.0, 1.0, (rest * 2 // 5, 2))
    uv = np.concatenate([fixed, wide, inside]).astype(np.float32)
    assert uv.shape == (n, 2) and np.isfinite(uv).all() and np.abs(uv).max() <= 1.5
    return uv


def shade_inputs(dump, gi, uv, seed):
    """Synthetic intersections on geom gi with the given texcoords: (idx, isects, paths) for shade().  Every record hits the mesh's own
    material with 4 bounces left, arrives at 17 to 73 degrees from the normal (the Schlick term then sends a good share to either side of
    the specular / diffuse draw for any index of refraction) and carries a random colour in [0.1, 1]."""
    rng = np.random.default_rng(seed)
    n = len(uv)
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tan = np.cross(nrm, rng.normal(size=(n, 3))); tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    c = rng.uniform(0.3, 0.95, (n, 1))
    p = np.zeros(n, PATH_DTYPE)
    p["direction"] = -(nrm * c + tan * np.sqrt(1 - c * c))
    p["origin"] = rng.uniform(-4, 4, (n, 3)) + [0, 5, 0]
    p["color"] = rng.uniform(0.1, 1.0, (n, 3))
    p["pixelIndex"] = np.arange(n)
    p["remainingBounces"] = 4
    i = np.zeros(n, ISECT_DTYPE)
    i["t"] = rng.uniform(1.0, 5.0, n)
    i["normal"] = nrm
    i["materialId"] = int(dump["geom_ints"][gi][1])
    i["geomId"] = gi
    i["texcoord"] = uv
    idx = rng.integers(0, 4_000_000, n).astype(np.int32)
    return idx, i, p


def mesh_rays(dump, gi, n, seed):
    """Rays aimed at mesh gi, origins around it (seeded like test_oracle_pin.test_random_stage_inputs)."""
    rng = np.random.default_rng(seed)
    f = np.asarray(dump["faces"][gi], np.float64).reshape(-1, 15)
    xf = np.asarray(dump["geom_mats"][gi][:16], np.float64).reshape(4, 4).T           # column-major, as glm stores it
    v = f[:, [0, 1, 2, 5, 6, 7, 10, 11, 12]].reshape(-1, 3, 3)
    pick = rng.integers(0, len(v), n)
    b = rng.dirichlet([1, 1, 1], n)
    obj = np.einsum("nk,nkc->nc", b, v[pick])
    target = obj @ xf[:3, :3].T + xf[:3, 3]
    centre = target.mean(axis=0)
    o = centre + rng.uniform(-4.5, 4.5, (n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = np.zeros(n, PATH_DTYPE)
    p["origin"], p["direction"] = o, d
    p["color"] = rng.uniform(0, 1, (n, 3))
    p["pixelIndex"] = np.arange(n)
    p["remainingBounces"] = rng.integers(2, 9, n)
    return p


# --- edits of a scene's POD dict: none changes its argument ----------------------------------------------------------------------

def _geoms(dump):
    tex = dump.get("textures") or {}
    return [dict(ints=np.array(dump["geom_ints"][i], np.int32), trs=np.array(dump["geom_trs"][i], np.float32),
                 mats=np.array(dump["geom_mats"][i], np.float32), faces=np.array(dump["faces"][i], np.float32).reshape(-1, 15),
                 tex={w: tex[(g, w)] for (g, w) in tex if g == i}) for i in range(len(dump["geom_ints"]))]


def _scene(dump, geoms, materials=None):
    out = dict(dump)
    out["geom_ints"] = np.stack([g["ints"] for g in geoms]).astype(np.int32)
    out["geom_trs"] = np.stack([g["trs"] for g in geoms]).astype(np.float32)
    out["geom_mats"] = np.stack([g["mats"] for g in geoms]).astype(np.float32)
    out["faces"] = [g["faces"] for g in geoms]
    out["textures"] = {(i, w): img for i, g in enumerate(geoms) for w, img in g["tex"].items()}
    if materials is not None:
        out["materials"] = np.asarray(materials, np.float32)
    return out


def mesh_index(dump):
    """the scene's (last) OBJ geom"""
    return int(np.nonzero(np.asarray(dump["geom_ints"])[:, 0] == 3)[0][-1])


def with_maps(dump, gi, maps):
    """geom gi carries exactly `maps` ({which: image}); every other geom keeps what it has"""
    g = _geoms(dump)
    g[gi]["tex"] = dict(maps)
    return _scene(dump, g)


def without_maps(dump):
    g = _geoms(dump)
    for x in g:
        x["tex"] = {}
    return _scene(dump, g)


def with_uv_transform(dump, gi, a, b):
    """uv' = a * uv + b on the face texcoords of geom gi (words 3,4 / 8,9 / 13,14 of each 15-float face), in float32"""
    g = _geoms(dump)
    f = g[gi]["faces"]
    for k in (3, 4, 8, 9, 13, 14):
        f[:, k] = np.float32(a) * f[:, k] + np.float32(b)
    return _scene(dump, g)


def _moved(O, geom, trs):
    out = dict(geom, trs=np.asarray(trs, np.float32), tex=dict(geom["tex"]))
    out["mats"] = O.build_transforms(out["trs"])
    return out


def with_second_mesh(O, dump, gi, trs, maps, front=True):
    """a copy of mesh gi with translation / rotation / scale `trs` (its matrices from the oracle's loader arithmetic) and its own maps,
    inserted as geom 0 (the scene then holds two meshes and the first of them is not the last geom) or, front=False, appended"""
    g = _geoms(dump)
    twin = _moved(O, g[gi], trs)
    twin["tex"] = dict(maps)
    return _scene(dump, [twin] + g if front else g + [twin])


def with_cubes_before_last(O, dump, total, seed):
    """small diffuse cubes (material 1) inserted before the last geom until the scene has `total` geoms"""
    rng = np.random.default_rng(seed)
    g = _geoms(dump)
    cubes = []
    for _ in range(total - len(g)):
        trs = np.concatenate([rng.uniform([-4.0, 0.6, -4.0], [4.0, 8.5, 3.0]), rng.uniform(-90, 90, 3), rng.uniform(0.2, 0.5, 3)])
        cubes.append(dict(ints=np.array([1, 1, 0], np.int32), trs=trs.astype(np.float32), mats=O.build_transforms(trs),
                          faces=np.zeros((0, 15), np.float32), tex={}))
    return _scene(dump, g[:-1] + cubes + g[-1:])


def with_face_uvs(dump, gi, seed):
    """random texcoords in [0, 1] written into the faces of a mesh that has none (models/cube.obj)"""
    rng = np.random.default_rng(seed)
    g = _geoms(dump)
    f = g[gi]["faces"]
    f[:, [3, 4, 8, 9, 13, 14]] = rng.uniform(0, 1, (len(f), 6)).astype(np.float32)
    return _scene(dump, g)


# --- whole frames: which scene, under which options -------------------------------------------------------------------------------

ALL_FOUR = {KD: (64, 33, 3), KS: (5, 9, 4), KE: (31, 17, 3), BUMP: (12, 40, 4)}           # four different non-square sizes
TWIN_MAPS = {KD: (7, 3, 4), KS: (3, 7, 3), KE: (9, 5, 4), BUMP: (5, 12, 3)}               # the second mesh's own
TWIN_TRS = (-2.0, 3.0, 2.0, 0.0, -25.0, 180.0, 1.0, 1.0, 1.0)
FRAME_CASES = [("kd", "kd", {}), ("ke", "ke", {}), ("bump", "bump", {}), ("ks+bump", "ks+bump", {}), ("all-four", "all", {}),
               ("all-four-no_mesh_split", "all", dict(no_mesh_split=1)), ("all-four-no_bvh", "all", dict(no_bvh=1)),
               ("all-four-depth_of_field", "all", dict(depth_of_field=1)), ("all-four-unsorted", "all", dict(sort_by_material=0)),
               ("all-four-no_lds_triangles", "all", dict(no_lds_triangles=1)),
               ("tiled", "tiled", {}), ("tiled-no_mesh_split", "tiled", dict(no_mesh_split=1)),
               ("two-meshes", "two", {}), ("two-meshes-no_mesh_split", "two", dict(no_mesh_split=1)),
               ("34-geoms", "34", {}), ("cube-kd", "cube", {})]


def frame_scene(O, key, ship, cornell_obj):
    """The scene of a FRAME_CASES key from the POD dicts of cornellSpaceship.txt and cornellObj.txt (O: the oracle, for the matrices of
    the geoms a case adds)."""
    gi = mesh_index(ship)
    subset = {"kd": (KD,), "ke": (KE,), "bump": (BUMP,), "ks+bump": (KS, BUMP)}
    if key in subset:
        return with_maps(ship, gi, make_maps({k: ALL_FOUR[k] for k in subset[key]}, 11))
    every = with_maps(ship, gi, make_maps(ALL_FOUR, 12))
    if key == "all":
        return every
    if key == "tiled":          # (the ship at twice its size: at 96 x 54 it otherwise meets 46 first-bounce rays, too few to show 50 clamped)
        g = _geoms(with_uv_transform(every, gi, *UV_TRANSFORMS["tiled"]))
        g[gi] = _moved(O, g[gi], np.concatenate([g[gi]["trs"][:6], [2.0, 2.0, 2.0]]))
        return _scene(every, g)
    if key in ("two", "34"):
        two = with_second_mesh(O, every, gi, TWIN_TRS, make_maps(TWIN_MAPS, 13))
        return two if key == "two" else with_cubes_before_last(O, two, 34, 14)
    assert key == "cube"
    ci = mesh_index(cornell_obj)
    return with_maps(with_face_uvs(cornell_obj, ci, 15), ci, make_maps({KD: (7, 3, 3)}, 16))


def clamped_lookups(dump, isects):
    """how many mesh hits of `isects` index some map of their geom outside it"""
    n = 0
    for (gi, which), img in dump["textures"].items():
        m = (isects["t"] > 0) & (isects["geomId"] == gi)
        cls = TR.classes(isects["texcoord"][m, 0], isects["texcoord"][m, 1], img.shape[1], img.shape[0])
        n = max(n, int(TR.clamped(cls).sum()))
    return n


# --- a scene on disk: the stand-in ship with four maps of different, non-square sizes, PPM and PNG mixed -------------------------

FILE_MAPS = {KD: (64, 33, 3, "ppm"), KS: (5, 9, 4, "png"), KE: (31, 17, 3, "png"), BUMP: (12, 40, 3, "ppm")}      # (w, h, ch, format)
_MTL_KEY = {KD: "map_Kd", KS: "map_Ks", KE: "map_Ke", BUMP: "map_Bump"}


def write_ship_scene(tmp_path, scene_text, seed=31):
    """Writes scenes/ship.txt (scene_text, its OBJ line pointing at ../models/standin_ship.obj), a copy of the mesh, an .mtl naming four
    generated maps and the maps themselves under tmp_path.  Returns (path of the scene file, {which: image as written, top row first})."""
    import re
    import shutil
    import pngcases
    for d in ("scenes", "models/materials", "textures"):
        os.makedirs(tmp_path / d)
    shutil.copy(os.path.join(ROOT, "models", "standin_ship.obj"), tmp_path / "models")
    rng = np.random.default_rng(seed)
    mtl = [l for l in open(os.path.join(ROOT, "models", "materials", "standin_ship.mtl")).read().splitlines() if not l.startswith("map_")]
    written = {}
    for which, (w, h, ch, fmt) in FILE_MAPS.items():
        img = random_map(rng, w, h, ch, which)
        name = "odd_%s.%s" % (_MTL_KEY[which][4:].lower(), fmt)
        if fmt == "ppm":
            (tmp_path / "textures" / name).write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
        else:
            (tmp_path / "textures" / name).write_bytes(pngcases.make_png(w, h, {3: 2, 4: 6}[ch], 8, img.astype(int), rng=rng))
        mtl.append("%s ../textures/%s" % (_MTL_KEY[which], name))
        written[which] = img
    (tmp_path / "models" / "materials" / "standin_ship.mtl").write_text("\n".join(mtl) + "\n")
    text, n = re.subn(r"^\.\./models/.*\.obj\s*$", "../models/standin_ship.obj", scene_text, flags=re.M)
    assert n == 1
    path = tmp_path / "scenes" / "ship.txt"
    path.write_text(text)
    return str(path), written


# --- what both tiers assert of a shaded batch ------------------------------------------------------------------------------------

def inner_count(cls, w, h):
    """lookups labelled interior; where the size has no interior (a single row is all `last row`), lookups inside the map"""
    if TR.INTERIOR in TR.admitted(w, h):
        return int((cls == TR.INTERIOR).sum())
    return int(np.isin(cls, (TR.INTERIOR, TR.LAST_ROW, TR.LAST_TEXEL)).sum())


def grid_conditions(uv, spec):
    """The caps of the shade grid, per map of a case: every class the size admits on [-0.5, 1.5] has at least 32 lanes, at least 25 % of
    the lanes are interior (inside the map, where the size has no interior: a single row is all `last row`), at least 10 % are clamped."""
    for which, (w, h, ch) in spec.items():
        cls = TR.classes(uv[:, 0], uv[:, 1], w, h, ch)
        count = np.bincount(cls, minlength=7)
        for c in TR.admitted(w, h):
            assert count[c] >= 32, (which, w, h, TR.CLASS_NAMES[c], int(count[c]))
        inner = inner_count(cls, w, h)
        assert inner >= 0.25 * len(uv), (which, w, h, "interior", int(inner))
        assert TR.clamped(cls).sum() >= 0.10 * len(uv), (which, w, h, "clamped", int(TR.clamped(cls).sum()))


def assert_shaded_by_rule(shaded, paths, uv, maps, material):
    """shaded = shade(paths) of shade_inputs(): on the lanes the rule says a ke texel lights, the colour is emission_colour bit for bit
    and the path has ended; on the others it is tint with the ks bytes (the material's specular colour without a ks map) or tint with the
    kd bytes (the material's colour without a kd map), each on at least 5 % of them, and the path goes on with 3 bounces."""
    from conftest import beq
    c_in = paths["color"]
    lit = TR.lit(TR.fetch(maps[KE], uv[:, 0], uv[:, 1])) if KE in maps else np.zeros(len(uv), bool)
    if KE in maps:
        assert lit.any() and (~lit).any(), "both sides of the emissive test must occur"
        assert beq(shaded["color"][lit], TR.emission_colour(c_in[lit], TR.fetch(maps[KE], uv[lit, 0], uv[lit, 1])))
        assert not shaded["remainingBounces"][lit].any()
    rest = ~lit
    spec = TR.tint(c_in, TR.fetch(maps[KS], uv[:, 0], uv[:, 1])) if KS in maps else c_in * material[4:7].astype(np.float32)
    diff = TR.tint(c_in, TR.fetch(maps[KD], uv[:, 0], uv[:, 1])) if KD in maps else c_in * material[0:3].astype(np.float32)
    same = lambda a, b: (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(axis=1)
    is_spec, is_diff = same(shaded["color"], spec) & rest, same(shaded["color"], diff) & rest
    assert (is_spec | is_diff)[rest].all(), "a lane's colour is neither the specular nor the diffuse texel's"
    assert (shaded["remainingBounces"][rest] == 3).all()
    n = int(rest.sum())
    assert (is_spec & ~is_diff).sum() >= 0.05 * n and (is_diff & ~is_spec).sum() >= 0.05 * n, (n, int(is_spec.sum()), int(is_diff.sum()))
    return lit

