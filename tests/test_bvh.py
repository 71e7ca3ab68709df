"""Mesh BVH (csrc/pt_bvh.h) against the reference's loop over all faces (src/intersections.h:213-233), on the CPU.

The tree only decides WHICH triangles are looked at; the per-triangle arithmetic and the choice of the winner (nearest
distance, lowest face index on ties) are the loop's.  ptx_debug_bvh_check runs both on the host with the library's own
code (the traversal is the function the kernels inline), so face and distance must agree bit for bit -- including
duplicate triangles (ties), axis-parallel rays (zero direction components), grazing rays and far origins.

What is covered where.  HERE, on the host: the skip-link walk, the front-to-back binary walk (trees shallower than BVH_STACK), the
single-ray four-wide walk and the four-wide steps under their finest schedule (one node or ONE triangle per turn), each against the
loop.  ON THE DEVICE, tests/test_gpu_mesh_walks.py: the same meshes (tests/meshcases.py) through every walk the kernels take -- k_mesh's
refilling four-wide walk, k_finish's fallback (skip links or loop), the single-lane four-wide walk and the ordered walk of meshKey with
a stack, the skip-link walk of k_kat_geom, the plain loop fused, chunked and from LDS -- against the oracle's loop, bit for bit, with
ptx_debug_mesh_plan saying which walk ran.  The fixture tests at the end of this file assert, without a GPU, that every case added for
the device tier agrees with the loop on the host and HAS the property it exists for (a tree deeper than the stacks, ties, NaNs ...), so
a failure there points at the device and no device case passes vacuously."""
import ctypes as C

import numpy as np
import pytest

from conftest import beq
import meshcases as mc
from meshcases import hull, rays_around


def run_check(product, faces, rays):
    L = product.load_library()
    faces = np.ascontiguousarray(faces, np.float32).reshape(-1, 15)
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = len(rays)
    fl, fb = np.zeros(n, np.int32), np.zeros(n, np.int32)
    tl, tb = np.zeros(n, np.float32), np.zeros(n, np.float32)
    st = np.zeros(4, np.int64)
    vp = C.c_void_p
    L.ptx_debug_bvh_check.restype = C.c_int
    L.ptx_debug_bvh_check.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
    rc = L.ptx_debug_bvh_check(faces.ctypes.data, len(faces), rays.ctypes.data, n, fl.ctypes.data, tl.ctypes.data,
                               fb.ctypes.data, tb.ctypes.data, st.ctypes.data)
    assert rc == 0
    return fl, tl, fb, tb, st


def assert_same(res):
    fl, tl, fb, tb, st = res
    assert beq(fl, fb), "faces differ at %s" % np.nonzero(fl != fb)[0][:8]
    assert beq(tl, tb)
    assert st[3] == 0, "the front-to-back walk or the walk over the four-wide quantised nodes disagrees with the skip-link walk on %d rays (>= 1e6: the wide walk overran its stack bound)" % st[3]
    return fl, st


def test_hull_random_rays(product):
    rng = np.random.default_rng(7)
    faces = hull(48, 96)                      # 9216 triangles
    rays = np.concatenate([rays_around(rng, 20000, 6.0, 1.5), rays_around(rng, 5000, 0.2, 2.0), rays_around(rng, 5000, 1000.0, 1.5)])
    fl, st = assert_same(run_check(product, faces, rays))
    assert (fl >= 0).mean() > 0.3
    assert st[1] == len(faces) and st[0] < 2 * len(faces)
    assert st[2] / len(rays) < 400            # the tree is actually pruning (the loop would visit 9216 triangles per ray)


def test_walk_statistics_of_the_last_check(product):
    """ptx_debug_bvh_visits: what the three walks cost on the rays of the last check -- the figures k_mesh's traversal was tuned
    by.  The four-wide walk visits fewer nodes than the binary front-to-back walk, that one fewer than the skip-link walk; its
    stack bound is inside what k_mesh provides; leaves hold at most four triangles, so a walk tests a handful, not hundreds."""
    rng = np.random.default_rng(17)
    faces = hull(32, 64)                      # 4096 triangles
    rays = rays_around(rng, 6400, 5.0, 1.2)
    assert_same(run_check(product, faces, rays))
    L = product.load_library()
    v = np.zeros(8, np.int64)
    L.ptx_debug_bvh_visits.restype = C.c_int
    L.ptx_debug_bvh_visits.argtypes = [C.c_void_p]
    assert L.ptx_debug_bvh_visits(v.ctypes.data) == 0
    skip, ordered, wide, need, group_max, groups, tris = (int(x) for x in v[:7])
    assert 0 < wide < ordered < skip
    assert 1 <= need <= 32
    assert groups == 100 and wide <= 64 * group_max          # (per 64 rays the longest walk bounds the sum)
    assert 0 < tris < 40 * len(rays)


def test_triangle_soup_and_ties(product):
    rng = np.random.default_rng(11)
    faces, n = mc.soup(rng, 3000)                                     # + exact duplicates: the lower face index must win
    rays = rays_around(rng, 30000, 5.0, 2.0)
    fl, st = assert_same(run_check(product, faces, rays))
    hit = fl[fl >= 0]
    assert len(hit) > 1000 and hit.max() < n                          # a duplicate never wins over its original


def test_axis_parallel_and_grazing(product):
    rng = np.random.default_rng(13)
    # a flat grid in the plane y = 0 (boxes of zero thickness) plus a vertical wall; rays straight down, along -z, down from the grid
    # lines, grazing
    faces, xs = mc.flat_grid(40)
    n = 8000
    rays = mc.flat_grid_rays(rng, xs, n)
    fl, st = assert_same(run_check(product, faces, rays))
    assert (fl >= 0).sum() > n


def test_needles_tiny_and_far(product):
    rng = np.random.default_rng(17)
    faces, tri = mc.needles(rng, 2000)
    rays = mc.needles_rays(rng, tri)
    fl, st = assert_same(run_check(product, faces, rays))
    assert (fl >= 0).sum() > 3000


@pytest.mark.parametrize("ratio", [1e3, 1e4, 1e5, 1e6])
def test_far_origin_sweep(product, ratio):
    """Origins 10^3 ... 10^6 mesh sizes away (binary32 barycentrics are then accurate to 1e-4 ... 1e-1 of an edge: the loop's
    own hits and misses are partly rounding noise).  The traversal's per-ray slack grows with the distance (pt_bvh.h, "Why the
    tree equals the loop"), so the tree still looks at every triangle the loop can accept: zero disagreements, on a
    well-shaped hull and on a soup with needles."""
    rng = np.random.default_rng(int(ratio) % 9973)
    faces = hull(24, 48)                      # 2304 triangles, size ~ 3
    n = 6000
    rays = rays_around(rng, n, 3.0 * ratio, 1.6)
    fl, st = assert_same(run_check(product, faces, rays))
    assert (fl >= 0).sum() > n // 20
    soup = mc.far_soup(rng, 800)
    assert_same(run_check(product, soup, rays_around(rng, 4000, 2.0 * ratio, 1.0)))


def test_near_rays_still_prune(product):
    """The slack must not cost the tree its point: from ordinary viewing distances (2-4 mesh sizes) a ray still visits a
    small fraction of a 9216-triangle hull."""
    rng = np.random.default_rng(23)
    faces = hull(48, 96)
    rays = rays_around(rng, 8000, 8.0, 1.5)
    fl, st = assert_same(run_check(product, faces, rays))
    assert st[2] / len(rays) < 450


# ---- the fixtures of the device tier (tests/test_gpu_mesh_walks.py): right on the host, and what they claim to be --------------------
def bvh_visits(product):
    L = product.load_library()
    v = np.zeros(8, np.int64)
    L.ptx_debug_bvh_visits.restype = C.c_int
    L.ptx_debug_bvh_visits.argtypes = [C.c_void_p]
    assert L.ptx_debug_bvh_visits(v.ctypes.data) == 0
    return dict(wide_need=int(v[3]), depth=int(v[7]))


def test_fixture_chain_is_deeper_than_the_wide_stack(product):
    """chain: the four-wide walk needs more than BVH_STACK entries (k_mesh must refuse it), the binary tree is still shallower than
    BVH_STACK (the ordered walk fits), and at least 25 distinct triangles are hit."""
    faces, rays = mc.chain_case(np.random.default_rng(31))
    assert len(faces) <= 3500 and len(rays) <= 40000
    fl, st = assert_same(run_check(product, faces, rays))
    v = bvh_visits(product)
    print("chain: wide stack need %d, binary depth %d, %d distinct faces hit, %.3f of the rays hit" % (v["wide_need"], v["depth"], len(np.unique(fl[fl >= 0])), (fl >= 0).mean()))
    assert v["wide_need"] > mc.BVH_STACK
    assert v["depth"] < mc.BVH_STACK
    assert len(np.unique(fl[fl >= 0])) >= 25


def test_fixture_chain_deep_is_deeper_than_every_stack(product):
    """chain_deep: a binary depth of at least BVH_STACK -- neither stack walk fits, only the skip links remain -- and still hit."""
    faces, rays = mc.chain_deep_case(np.random.default_rng(31))
    assert len(faces) <= 3500 and len(rays) <= 40000
    fl, st = assert_same(run_check(product, faces, rays))
    v = bvh_visits(product)
    print("chain_deep: wide stack need %d, binary depth %d, %d distinct faces hit" % (v["wide_need"], v["depth"], len(np.unique(fl[fl >= 0]))))
    assert v["wide_need"] > mc.BVH_STACK and v["depth"] >= mc.BVH_STACK
    assert len(np.unique(fl[fl >= 0])) >= 25


def test_fixture_coincident_centroids(product):
    faces, rays = mc.coincident(np.random.default_rng(41))
    assert len(faces) == 64
    cent = faces.reshape(-1, 3, 5)[:, :, :3].astype(np.float64).mean(axis=1)
    assert np.abs(cent - cent[0]).max() < 1e-6                          # one centroid, to float32 rounding of the vertices
    fl, st = assert_same(run_check(product, faces, rays))
    assert (fl >= 0).mean() > 0.10
    assert len(np.unique(fl[fl >= 0])) > 32


def test_fixture_soup_with_nan_and_zero_area_triangles(product):
    faces, rays, n = mc.soup_nan(np.random.default_rng(43))
    assert len(faces) <= 3520 and np.isnan(faces).any()
    tri = faces.reshape(-1, 3, 5)[:, :, :3]
    assert (np.all(tri[:, 1] == tri[:, 2], axis=1)).sum() == 10        # the zero-area ones
    fl, st = assert_same(run_check(product, faces, rays))
    assert (fl >= 0).mean() > 0.10
    assert fl.max() < n                                                 # neither a duplicate nor a degenerate triangle ever wins
    # ... and ties exist: some winner has an exact copy further down the list
    assert np.isin(fl[fl >= 0], np.arange(0, 500)).any()


@pytest.mark.parametrize("k", [23, 24, 25])
def test_fixture_hull_cut_to_the_loop_tree_boundary(product, k):
    faces = mc.hull_cut(k)
    assert len(faces) == k and (k >= mc.BVH_MIN_FACES) == (k >= 24)
    fl, st = assert_same(run_check(product, faces, mc.hull_cut_rays(np.random.default_rng(47 + k))))
    assert (fl >= 0).mean() > 0.10
    assert len(np.unique(fl[fl >= 0])) > k // 2


def test_mesh_plan_refuses_a_null_tracer(product):
    """ptx_debug_mesh_plan is host-only and says so with an error code, not a crash, when there is no tracer to ask."""
    L = product.load_library()
    out = np.zeros(8, np.int32)
    assert L.ptx_debug_mesh_plan(None, 0, out.ctypes.data) != 0
