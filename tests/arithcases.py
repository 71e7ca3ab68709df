"""Ray families for the float64 tests of the arithmetic levels, shared by the host tier (tests/test_arith_f64_cpu.py: the float64
reference against the oracle and its contracted build) and the device tier (tests/test_gpu_arith_f64.py: levels 0, 1 and 2 against the
reference).  Every ray is finite; every family has N = 4096 rays; a seed names a family.

A SUBJECT is one geom under one transform: a cube or a sphere under each of TRANSFORMS, or one of the mesh cases of
tests/test_gpu_mesh_walks.py under the case's own transform.  Its families are generated in the geom's object space (the unit cube, the
sphere of radius 1/2: "size" = 1; a mesh: its case's extent), taken to world space in float64 and rounded once to the fp32 rays every
build then sees -- the margins the tests quote are recomputed from those fp32 rays by tests/isect_f64.py, not taken from the recipe.

  cube     random      from a sphere of 3 sizes towards the cube
           inside      origins inside, any direction
           axis        one non-zero direction component in object space (an exact axis on the device under TRS_FLAT, the wall and the
                       identity; under a rotation the object-space direction is only nearly one)
           edge_d      aimed d inside / d outside a silhouette edge, d = 1e-2, 1e-4, 1e-6 sizes (first half inside, second half outside)
           corner_d    the same about a silhouette corner
           far_r       origins r = 1e2, 1e3, 1e5 sizes away
  sphere   random, inside, far_r as above; graze_d = impact parameter r (1 -+ d).  The non-uniform scales are TRS_ROT, TRS_FLAT and the wall.
  mesh     own         the case's own rays (an even subset of N)
           far         the far-origin sweep, 1e3 .. 1e6 mesh sizes (cases with a size)
"""
import numpy as np

import meshcases as mc
import test_gpu_mesh_walks as mw

N = 4096
DELTAS = (1e-2, 1e-4, 1e-6)
FAR = (1e2, 1e3, 1e5)
# the sphere's root formula takes b^2 - (|o|^2 - 1/4) with b ~ |o| = R sizes: an absolute error of about R^2 u in a radicand of at most
# 1/4.  At R = 2^11 the error IS the radicand -- the operation has no digit left in any arithmetic -- so the sphere's far families stop
# a decade before that
FAR_SPHERE = (30.0, 100.0, 300.0)

IDENT = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
WALL = (0.0, 5.0, 0.0, 0.0, 0.0, 0.0, 12.0, 0.01, 12.0)
TRANSFORMS = {"identity": IDENT, "rot": mw.TRS_ROT, "small": mw.TRS_SMALL, "flat": mw.TRS_FLAT, "wall": WALL}
MESH_CASES = ["hull", "hull_small_scale", "soup", "needles", "far_soup", "chain", "chain_deep", "hull_cut24", "hull_cut25"]
SUBJECTS = [("cube", t) for t in TRANSFORMS] + [("sphere", t) for t in TRANSFORMS] + [("mesh", c) for c in MESH_CASES]


def _seed(*words):
    return np.random.default_rng([sum(ord(c) * (k + 1) for k, c in enumerate(w)) if isinstance(w, str) else int(w) for w in words])


def _signed_permutations(rng, pts):
    """each (n, k, 3) row group under a random axis permutation and random signs: the cube's symmetries"""
    n = len(pts)
    perm = np.argsort(rng.random((n, 3)), axis=1)
    sign = rng.choice([-1.0, 1.0], size=(n, 3))
    return np.take_along_axis(pts, np.broadcast_to(perm[:, None, :], pts.shape), axis=2) * sign[:, None, :]


def _silhouette(rng, delta, corner):
    """rays past the edge x = 1/2 of the top face y = 1/2, coming from above and from -x, so that the face x = 1/2 faces away: the target
    lies in the top face's plane, delta inside the edge (a hit with that margin) or delta beyond it (a miss by that much)"""
    n = N
    side = np.where(np.arange(n) < n // 2, -1.0, 1.0)
    tgt = np.stack([0.5 + side * delta, np.full(n, 0.5), rng.uniform(-0.4, 0.4, n)], axis=1)
    d = np.stack([rng.uniform(0.2, 1.0, n), -rng.uniform(0.2, 1.0, n), rng.uniform(-0.3, 0.3, n)], axis=1)
    if corner:
        tgt[:, 2] = 0.5 + side * delta
        d[:, 2] = rng.uniform(0.2, 1.0, n)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = tgt - d * rng.uniform(2.0, 4.0, (n, 1))
    pts = _signed_permutations(rng, np.stack([o, d], axis=1))
    return np.concatenate([pts[:, 0], pts[:, 1]], axis=1)


def _random_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def cube_families(tname):
    fam = {}
    fam["random"] = mc.rays_around(_seed("cube", "random"), N, 3.0, 0.6)
    rng = _seed("cube", "inside")
    fam["inside"] = np.concatenate([rng.uniform(-0.45, 0.45, (N, 3)), _random_dirs(rng, N)], axis=1)
    if tname in ("flat", "rot"):
        fam["axis"] = mc.axis_parallel_rays(_seed("cube", "axis"), N // 6 + 1, [-0.5] * 3, [0.5] * 3)[:N]
    for dl in DELTAS:
        fam["edge_%g" % dl] = _silhouette(_seed("cube", "edge", int(-np.log10(dl))), dl, False)
        fam["corner_%g" % dl] = _silhouette(_seed("cube", "corner", int(-np.log10(dl))), dl, True)
    for r in FAR:
        fam["far_%g" % r] = mc.rays_around(_seed("cube", "far", int(np.log10(r))), N, r, 0.4)
    return fam


def sphere_families(tname):
    fam = {}
    fam["random"] = mc.rays_around(_seed("sphere", "random"), N, 3.0, 0.4)
    rng = _seed("sphere", "inside")
    fam["inside"] = np.concatenate([_random_dirs(rng, N) * rng.uniform(0.0, 0.45, (N, 1)), _random_dirs(rng, N)], axis=1)
    for dl in DELTAS:
        rng = _seed("sphere", "graze", int(-np.log10(dl)))
        d = _random_dirs(rng, N)
        e = np.cross(d, _random_dirs(rng, N))
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        side = np.where(np.arange(N) < N // 2, -1.0, 1.0)[:, None]
        fam["graze_%g" % dl] = np.concatenate([e * 0.5 * (1.0 + side * dl) - d * rng.uniform(2.0, 4.0, (N, 1)), d], axis=1)
    for r in FAR_SPHERE:
        fam["far_%g" % r] = mc.rays_around(_seed("sphere", "far", int(r)), N, r, 0.3)
    return fam


def mesh_families(case):
    c = mw._case(case)
    rays = c["rays"]
    fam = {"own": rays[np.linspace(0, len(rays) - 1, N).astype(np.int64)]}
    if c["size"]:
        fam["far"] = mc.far_rays(_seed("mesh", "far", case), N // 4, c["size"])
    return fam


def family_delta(name):
    """the d of a near-silhouette family, None for the others"""
    return float(name.split("_")[1]) if name.split("_")[0] in ("edge", "corner", "graze") else None


def family_far(name):
    """how many sizes away a family's origins are at most (the mesh sweep: 1e6)"""
    if name == "far":
        return 1e6
    return float(name.split("_")[1]) if name.startswith("far_") else 10.0


def subject(O, kind, which):
    """-> dict(kind, which, d = the one-geom scene (POD dict), gm = its matrices, faces (mesh) or None, families = {name: (N, 6) fp32 world rays})"""
    _, mats = mw.box_geoms()
    if kind == "mesh":
        c = mw._case(which)
        geoms, faces, fam = [("mesh", 1, c["trs"], c["faces"])], np.ascontiguousarray(c["faces"], np.float32), mesh_families(which)
    else:
        geoms, faces, fam = [(kind, 1, TRANSFORMS[which])], None, (cube_families if kind == "cube" else sphere_families)(which)
    d = mw.make_scene(O, geoms, mats)
    world = {}
    for name, rays in fam.items():
        w = mw.to_world(d, 0, np.asarray(rays, np.float64))
        assert w.shape == (N, 6) and np.isfinite(w).all(), (kind, which, name)
        world[name] = w
    return dict(kind=kind, which=which, d=d, gm=d["geom_mats"][0], faces=faces, families=world)


# ---- the rules both tiers assert -------------------------------------------------------------------------------------------------------
BOUND_U = 64.0            # |oracle - reference| on well-conditioned rays, in u of the quantity's scale (isect_f64.scales)
CAP, CAP_ILL = 0.98, 0.50
QUANTITIES = ("t", "point", "normal")


def ill_conditioned(kind, name):
    """the families whose usable subset S need only be half of the reference's hits: those aimed within 1e-4 sizes of a silhouette, and
    the far-origin sweep of a MESH.  From 1e3 .. 1e6 sizes away the fp32 origin is only known to 6e-5 .. 6e-2 sizes while a face is 0.1
    sizes across and smaller, so the oracle itself keeps 56-89 % of the reference's hits there (the host tier prints it).  A cube or a sphere
    seen from afar keeps its one silhouette: their far families hold 98 % like every other family."""
    d = family_delta(name)
    return (d is not None and d <= 1e-4) or (kind == "mesh" and name == "far")


def well_conditioned(kind, name):
    """the families on which the oracle must BE the reference to 64 u: aimed no closer than 1e-2, origins within 100 sizes.  The
    sphere's far families are left out at every distance: the root formula the oracle restates loses R^2 u of a radicand of at most 1/4
    (FAR_SPHERE above), which is the formula's error and not the reference's -- the host test prints it."""
    d = family_delta(name)
    return (d is None or d >= 1e-2) and family_far(name) <= 100.0 and not (kind == "sphere" and name.startswith("far"))


# needles (1e-3 sizes wide) seen from 1e3 .. 1e6 sizes away through fp32 coordinates that resolve 6e-5 .. 6e-2 sizes there: the oracle
# itself keeps fewer than half of the reference's hits, so no arithmetic can be held to an accuracy on them.  The decision counts and
# the per-walk rule still run on this family.
ACCURACY_NOT_ASSERTED = {("mesh", "needles", "far")}


def spread(x):
    """(rms, 99th percentile, maximum) of an error sample, in u"""
    import isect_f64 as f64
    x = np.asarray(x, np.float64)
    if not len(x):
        return 0.0, 0.0, 0.0
    return float(np.sqrt((x * x).mean()) / f64.U), float(np.quantile(x, 0.99) / f64.U), float(x.max() / f64.U)


def accuracy_ratios(e_base, e_level):
    """{quantity: (rms ratio, 99th-percentile ratio)} of a build's errors over max(the base build's, 1 u of the scale)"""
    out = {}
    for q in QUANTITIES:
        b, l = spread(e_base[q]), spread(e_level[q])
        out[q] = (l[0] / max(b[0], 1.0), l[1] / max(b[1], 1.0))
    return out
