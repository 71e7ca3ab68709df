"""CPU: the candidate pre-test's OBJECT-space boxes of the small meshes (cullMask / objBoxReach in pt_device.h; the table and its derived
margins: objcull_entry in pt_scene.hip, handed out device-free by ptx_debug_cull_objboxes).  A box that rejects a ray the exact test would
accept loses a hit silently, so the device's arithmetic on the table -- restated here in binary32, one rounding per product, sum and fused
multiply-add -- must accept every ray that hits a face in exact arithmetic (binary64 here, both orientations of a face, a face's edge
counted in), and every ray the oracle's binary32 test accepts.  Rays aimed at faces, edges and vertices, grazing the box, starting on a
face and inside the box, parallel to an object and to a world axis; meshes: models/cube.obj, a single quad (a box without thickness) and
the adversarial meshes of tests/meshcases.py at sizes that keep the face-by-ray products small; uniform scales 0.01 .. 300, non-uniform
scales, rotations, and the unrotated TRS_FLAT (an object axis is an exact world axis).  With the margins taken out (margin = 0) the same
rays must lose hits: the test can fail."""
import os

import numpy as np
import pytest

import meshcases as mc
from conftest import ROOT
import mygpuraytracer_amd as pt

f32 = np.float32
FAR = 1000.0                     # origins stay inside CULL_FAR_ORIGIN = 1024: rays from beyond it are never pre-tested (cull == 2)

TRS = {
    "cornell": (-2.0, 4.0, -3.0, 0.0, 45.0, 0.0, 2.0, 2.0, 2.0),
    "rot": (0.3, 5.0, -0.5, 25.0, 40.0, -15.0, 1.2, 0.8, 1.0),
    "rot2": (-0.5, 4.0, 0.5, -70.0, 10.0, 130.0, 0.7, 1.3, 0.9),
    "flat": (0.2, 5.0, -0.4, 0.0, 0.0, 0.0, 1.25, 0.5, 0.75),
    "tiny": (0.5, 5.0, 1.0, 10.0, 20.0, 30.0, 0.01, 0.01, 0.01),
    "huge": (20.0, -30.0, 10.0, 33.0, -20.0, 70.0, 300.0, 300.0, 300.0),
    "uneven": (1.0, 2.0, 3.0, 50.0, 15.0, -80.0, 3.0, 0.05, 0.6),
    "turned": (0.0, 5.0, 0.0, 90.0, 0.0, 45.0, 1.0, 1.0, 1.0),
}


def _cube():
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"))
    return s.dump()["faces"][6].copy()


def _quad():
    p = np.array([[[-1, 0, -1], [1, 0, 1], [1, 0, -1]], [[-1, 0, -1], [-1, 0, 1], [1, 0, 1]]], f32)
    return mc.with_uv(p)


def _mesh(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "cube":
        return _cube()
    if name == "quad":
        return _quad()
    if name == "hull_cut23":
        return mc.hull_cut(23)
    if name == "soup":
        return mc.soup(rng, 150, dup=((0, 20),))[0]
    if name == "flat_grid":
        return mc.flat_grid(6)[0]
    if name == "needles":
        return mc.needles(rng, 80)[0]
    if name == "far_soup":
        return mc.far_soup(rng, 100)
    if name == "chain":
        return mc.chain(rng, 40, 1.6, 12)[0]
    if name == "coincident":
        return mc.coincident(rng, 32, 1)[0]
    raise KeyError(name)


CASES = [("cube", t) for t in TRS] + [("quad", t) for t in TRS] + [(m, t) for m in ("hull_cut23", "soup", "flat_grid", "needles", "far_soup", "chain", "coincident")
                                                                   for t in ("rot", "flat", "tiny", "uneven")]


# ---- the device's arithmetic, restated ---------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    # one rounding of a * b + c (binary32 operands: the product is exact in binary64, the sum is off by <= 2^-53 relative before the rounding)
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def device_objbox(T, o, d):
    """objBoxReach (pt_device.h) for rays (n, 3) + (n, 3) float32 against one table entry T (16 floats): True = candidate"""
    T = T.astype(f32)
    o = o.astype(f32); d = d.astype(f32)
    p = [(o[:, m] - T[4 * m + 3]).astype(f32) for m in range(3)]
    q = [_fma(T[4 * r + 2], p[2], _fma(T[4 * r + 1], p[1], (T[4 * r] * p[0]).astype(f32))) for r in range(3)]
    e = [_fma(T[4 * r + 2], d[:, 2], _fma(T[4 * r + 1], d[:, 1], (T[4 * r] * d[:, 0]).astype(f32))) for r in range(3)]
    a = [np.abs(x) for x in q]
    f = [np.abs(x) for x in e]
    s = (T[15] * ((a[0] + a[1]).astype(f32) + a[2]).astype(f32)).astype(f32)
    h = [(T[12 + r] + s).astype(f32) for r in range(3)]
    floor = np.full(len(o), 2.0 ** -100, f32)
    out = np.zeros(len(o), bool)
    for r in range(3):
        same_sign = (q[r].view(np.int32) ^ e[r].view(np.int32)) >= 0
        out |= (a[r] > h[r]) & same_sign
    for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        L = np.abs(_fma(q[j], e[k], (-(q[k] * e[j]).astype(f32)).astype(f32)))
        R = _fma(h[j], f[k], _fma(h[k], f[j], floor))
        with np.errstate(invalid="ignore"):
            out |= L > R
    return ~out


# ---- exact arithmetic ----------------------------------------------------------------------------------------------------------------------
def exact_hits(inv16, faces, o, d):
    """does the ray hit some face?  The exact test's object space (the geom's inverse transform as it is stored), binary64, Moeller-Trumbore
    on both orientations, a face's edges and vertices counted in (1e-12: the rounding of binary64 itself)"""
    M = inv16.astype(np.float64).reshape(4, 4).T
    oo = o.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    dd = d.astype(np.float64) @ M[:3, :3].T
    v = faces.astype(np.float64).reshape(-1, 3, 5)[:, :, :3]
    v = v[np.isfinite(v).all(axis=(1, 2))]
    v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    hit = np.zeros(len(o), bool)
    for lo in range(0, len(o), 2048):
        O, D = oo[lo:lo + 2048, None, :], dd[lo:lo + 2048, None, :]
        P = np.cross(D, e2[None])
        det = (e1[None] * P).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            S = O - v0[None]
            bu = (S * P).sum(-1) * inv
            Q = np.cross(S, e1[None])
            bv = (D * Q).sum(-1) * inv
            t = (e2[None] * Q).sum(-1) * inv
            eps = 1e-12
            ok = (np.abs(det) > 0) & (bu >= -eps) & (bv >= -eps) & (bu + bv <= 1 + eps) & (t >= 0)
        hit[lo:lo + 2048] = ok.any(axis=1)
    return hit


# ---- rays ------------------------------------------------------------------------------------------------------------------------------------
def _unit(x):
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-300)


def world_rays(rng, xf16, faces, n=350):
    """world-space rays (o, d float32, |d| = 1) for one mesh under one transform"""
    X = xf16.astype(np.float64).reshape(4, 4).T
    v = faces.astype(np.float64).reshape(-1, 3, 5)[:, :, :3]
    v = v[np.isfinite(v).all(axis=(1, 2))]
    lo, hi = v.min(axis=(0, 1)), v.max(axis=(0, 1))
    to_w = lambda p: p @ X[:3, :3].T + X[:3, 3]
    centre_w = to_w(0.5 * (lo + hi)[None])[0]
    size_w = max(float(np.linalg.norm(to_w(hi[None])[0] - to_w(lo[None])[0])), 1e-6)

    def origins(k, near=1.0, far=6.0):
        o = centre_w + _unit(rng.normal(size=(k, 3))) * size_w * rng.uniform(near, far, (k, 1))
        return np.clip(o, -FAR, FAR)

    def face_points(k, kind):
        f = v[rng.integers(0, len(v), k)]
        if kind == "face":
            b = rng.dirichlet((1, 1, 1), k)
        elif kind == "edge":
            b = np.zeros((k, 3)); a = rng.uniform(0, 1, k); i = rng.integers(0, 3, k)
            b[np.arange(k), i] = a; b[np.arange(k), (i + 1) % 3] = 1 - a
        else:
            b = np.zeros((k, 3)); b[np.arange(k), rng.integers(0, 3, k)] = 1
        return (f * b[:, :, None]).sum(axis=1)

    rays = []
    for kind in ("face", "edge", "vertex"):                                   # aimed at faces, edges and vertices, from near and far
        tgt = to_w(face_points(n, kind)); o = origins(n, 0.6, 50.0 if kind == "face" else 6.0)
        rays.append((o, tgt - o))
    box_pts = lo + (hi - lo) * rng.integers(0, 2, (n, 3))                      # grazing: at the box's corners, along its edges and just past them
    free = rng.integers(0, 3, n); box_pts[np.arange(n), free] = (lo + (hi - lo) * rng.uniform(-0.05, 1.05, (n, 3)))[np.arange(n), free]
    o = origins(n); rays.append((o, to_w(box_pts) - o))
    fo = to_w(face_points(n, "face")); rays.append((fo, rng.normal(size=(n, 3))))                      # starting on a face, any direction
    ins = to_w(lo + (hi - lo) * rng.uniform(0, 1, (n, 3))); rays.append((ins, rng.normal(size=(n, 3))))      # starting inside the box
    for axes in (np.eye(3), X[:3, :3].T / np.linalg.norm(X[:3, :3].T, axis=1, keepdims=True)):       # parallel to a world axis / to an object axis
        k = rng.integers(0, 3, n); sg = rng.choice([-1.0, 1.0], n)
        dd = axes[k] * sg[:, None]
        tgt = to_w(face_points(n, "face"))
        rays.append((np.clip(tgt - dd * size_w * rng.uniform(0.5, 4.0, (n, 1)), -FAR, FAR), dd))
    o = np.concatenate([r[0] for r in rays]).astype(f32)
    d = _unit(np.concatenate([r[1] for r in rays])).astype(f32)
    d[np.abs(d) < 1e-7] = 0                                                   # (the axis-parallel rays: exact zeros where the rotation leaves them)
    return o, d


def _pod(O, trs, faces):
    gm = O.build_transforms(np.array(trs, f32))
    mats = np.zeros((1, 11), f32); mats[0, :3] = 0.8
    cf = O.camera_from_loader(8, 8, 45.0, (0.0, 5.0, 10.5), (0.0, 5.0, 0.0), (0.0, 1.0, 0.0))
    return dict(geom_ints=np.array([[3, 0, len(faces)]], np.int32), geom_trs=np.array([trs], f32), geom_mats=gm[None].copy(), materials=mats,
                faces=[np.ascontiguousarray(faces, f32)], cam_ints=np.array([8, 8, 1, 2], np.int32), cam_floats=cf, textures={})


def _lost(oracle_lib, mesh, trs, margin):
    """-> (exact hits, exact hits the table rejects, oracle hits, oracle hits it rejects, rays it rejects at all, rays)"""
    O = oracle_lib
    faces = _mesh(mesh)
    d = _pod(O, TRS[trs], faces)
    tab, bits = pt.api.debug_cull_objboxes(d["geom_ints"], d["geom_mats"], d["faces"], margin=margin, no_bvh=1)
    assert bits == 1, "no entry for %s under %s" % (mesh, trs)
    o, dr = world_rays(np.random.default_rng(len(mesh) * 131 + len(trs)), d["geom_mats"][0][:16], faces)
    cand = device_objbox(tab[0], o, dr)
    exact = exact_hits(d["geom_mats"][0][16:32], faces, o, dr)
    O.set_libm(1)
    try:
        O.create(d, {})
        seen = O.geom_test(0, np.concatenate([o, dr], axis=1))[:, 0] > 0
    finally:
        O.set_libm(0)
    return int(exact.sum()), int((exact & ~cand).sum()), int(seen.sum()), int((seen & ~cand).sum()), int((~cand).sum()), len(o)


@pytest.mark.parametrize("mesh,trs", CASES, ids=["%s-%s" % c for c in CASES])
def test_no_hit_is_rejected(oracle_lib, mesh, trs):
    nx, lost_x, no, lost_o, rejected, n = _lost(oracle_lib, mesh, trs, 1.0)
    print(mesh, trs, "rays", n, "exact hits", nx, "lost", lost_x, "oracle hits", no, "lost", lost_o, "rejected", rejected)
    assert nx > n // 8 and no > 0, "the rays do not reach the mesh: the case is empty"
    assert lost_x == 0 and lost_o == 0
    assert rejected > 0, "the box rejects nothing: it is not a pre-test"


@pytest.mark.parametrize("trs", list(TRS))
def test_the_box_is_no_larger_than_its_margins(oracle_lib, trs):
    """the other direction: six separating axes decide a ray against a box exactly, so every candidate reaches -- in binary64, slab by
    slab -- the table's own box H + k |q|_1 widened by one part in 10^4, and most rays that point anywhere are rejected"""
    faces = _cube()
    d = _pod(oracle_lib, TRS[trs], faces)
    tab, bits = pt.api.debug_cull_objboxes(d["geom_ints"], d["geom_mats"], d["faces"])
    T = tab[0].astype(np.float64)
    rng = np.random.default_rng(77)
    o, _ = world_rays(rng, d["geom_mats"][0][:16], faces)
    dr = _unit(rng.normal(size=o.shape)).astype(f32)
    cand = device_objbox(tab[0], o, dr)
    M = T[:12].reshape(3, 4)
    q = (o.astype(np.float64) - M[:, 3]) @ M[:, :3].T
    e = dr.astype(np.float64) @ M[:, :3].T
    h = (T[12:15] + T[15] * np.abs(q).sum(axis=1, keepdims=True)) * (1 + 1e-4)
    tn = np.zeros(len(o)); tf = np.full(len(o), np.inf); ok = np.ones(len(o), bool)
    for k in range(3):
        with np.errstate(divide="ignore", invalid="ignore"):
            t0 = (-h[:, k] - q[:, k]) / e[:, k]; t1 = (h[:, k] - q[:, k]) / e[:, k]
        z = e[:, k] == 0
        ok &= np.where(z, np.abs(q[:, k]) <= h[:, k], True)
        tn = np.where(z, tn, np.maximum(tn, np.minimum(t0, t1))); tf = np.where(z, tf, np.minimum(tf, np.maximum(t0, t1)))
    reach = ok & (tn <= tf)
    print(trs, "rays", len(o), "candidates", int(cand.sum()), "reach the widened box", int(reach.sum()))
    assert not np.any(cand & ~reach)
    assert (~cand).sum() > len(o) // 4


def test_without_the_margins_hits_are_lost(oracle_lib):
    """the same rays against the bare boxes (margin = 0): rays aimed at vertices and edges and rays along a flat box fall to either side
    of the bare box by rounding, so some hit must be rejected -- what the margins are for, and the proof that the test above can fail"""
    lost = {}
    for mesh, trs in (("cube", "cornell"), ("cube", "rot"), ("quad", "rot2"), ("quad", "flat"), ("flat_grid", "rot")):
        nx, lost_x, no, lost_o, _, _ = _lost(oracle_lib, mesh, trs, 0.0)
        lost[(mesh, trs)] = (lost_x, lost_o)
    print(lost)
    assert sum(v[0] for v in lost.values()) > 0
    assert any(v[0] > 0 for k, v in lost.items() if k[0] != "cube"), "a flat box without margins must lose hits"


def test_which_geoms_get_an_entry(oracle_lib):
    """only meshes, only in a scene where no mesh has a BVH (24 faces and more, unless no_bvh), never a mesh without faces, with a
    non-finite vertex or a singular matrix; a geom without an entry has a table of zeros"""
    O = oracle_lib
    cube, hull = _cube(), mc.hull(4, 6)                        # 12 and 48 faces
    gm = np.stack([O.build_transforms(np.array(TRS[t], f32)) for t in ("cornell", "rot", "flat")])
    gi = np.array([[1, 0, 0], [3, 0, 12], [3, 0, 12]], np.int32)
    none = np.zeros((0, 15), f32)
    tab, bits = pt.api.debug_cull_objboxes(gi, gm, [none, cube, cube])
    assert bits == 0b110 and not tab[0].any() and tab[1].any() and tab[2].any()
    assert np.all(tab[1:, 12:15] > 1.0) and np.all(tab[1:, 12:15] < 1.01) and np.all(tab[1:, 15] > 2.0 ** -13) and np.all(tab[1:, 15] < 2.0 ** -12)
    tab, bits = pt.api.debug_cull_objboxes(np.array([[1, 0, 0], [3, 0, 12], [3, 0, 48]], np.int32), gm, [none, cube, hull])
    assert bits == 0 and not tab.any()                          # a mesh with a BVH in the scene: the split mesh search, no pair-list entries
    tab, bits = pt.api.debug_cull_objboxes(np.array([[1, 0, 0], [3, 0, 12], [3, 0, 48]], np.int32), gm, [none, cube, hull], no_bvh=1)
    assert bits == 0b110
    bad = cube.copy(); bad[3, 5] = np.nan
    flat = gm.copy(); flat[2, 16:32] = 0; flat[2, 31] = 1       # singular inverse
    tab, bits = pt.api.debug_cull_objboxes(np.array([[3, 0, 0], [3, 0, 12], [3, 0, 12]], np.int32), flat, [none, bad, cube])
    assert bits == 0 and not tab.any()
    quad_tab, bits = pt.api.debug_cull_objboxes(np.array([[3, 0, 2]], np.int32), gm[:1], [_quad()])
    assert bits == 1 and quad_tab[0, 13] > 0 and quad_tab[0, 13] < 1e-2      # a flat box keeps a positive thickness
