"""Meshes and ray sets for the mesh-search tests, shared by the host tier (tests/test_bvh.py: ptx_debug_bvh_check, tree against loop on the
CPU) and the device tier (tests/test_gpu_mesh_walks.py: every walk of the device against the oracle's loop).

A mesh is an (n, 15) float32 array, three vertices of x, y, z, u, v (the loader's face layout); a ray set is (n, 6) float32, origin and
direction in the mesh's object space (the direction need not be normalised: meshIntersectionTest normalises it).  Every generator takes
its numpy Generator and draws from it in a fixed order, so a seed names a mesh.

The cases and what each one is for:
  hull             a closed, well-shaped surface: balanced tree, the ordinary case
  soup             triangle soup with exact duplicates: ties, the lower face index must win
  flat_grid        a zero-thickness grid plus a wall: node boxes without extent; axis-parallel rays (zero direction components),
                   rays from the grid lines (shared edges), grazing rays
  needles          needles and tiny triangles
  far_soup         the soup of needles the far-origin sweep (10^3 .. 10^6 mesh sizes) runs on
  chain            a geometric progression of triangles on a line: binned SAH peels them off one at a time, so the tree is as deep
                   as the mesh is long -- deeper than the walks' stacks (BVH_STACK = 32)
  chain_deep       a longer chain: a binary depth of at least 32 with the margin to spare
  coincident       triangles with ONE common centroid: the builder finds no extent to bin and splits by list position
  soup_nan         the soup, plus a triangle with a NaN vertex and ten zero-area triangles
  hull_cut(k)      the first k faces of a small hull, k = 23, 24, 25: either side of BVH_MIN_FACES = 24 (loop / tree)
"""
import numpy as np

BVH_MIN_FACES = 24          # csrc/pt_bvh.h
BVH_STACK = 32              # csrc/pt_bvh.h


def hull(rings, segs, rng=None):
    """closed UV-mapped ellipsoid-like hull, outward CCW, as 15-float faces"""
    v = []
    for r in range(rings + 1):
        th = np.pi * r / rings
        for s in range(segs + 1):
            ph = 2 * np.pi * s / segs
            b = 1.0 + 0.25 * np.sin(3 * th) * np.cos(2 * ph)
            v.append((1.6 * np.sin(th) * np.cos(ph) * b, 0.7 * np.cos(th), np.sin(th) * np.sin(ph) * b, s / segs, r / rings))
    v = np.array(v, np.float32)
    idx = lambda r, s: r * (segs + 1) + s
    f = []
    for r in range(rings):
        for s in range(segs):
            a, b, c, d = idx(r, s), idx(r, s + 1), idx(r + 1, s + 1), idx(r + 1, s)
            f.append(np.concatenate([v[a], v[c], v[d]]))
            f.append(np.concatenate([v[a], v[b], v[c]]))
    return np.array(f, np.float32)


def rays_around(rng, n, radius, target_scale=1.0):
    o = rng.normal(size=(n, 3)).astype(np.float32)
    o *= (radius / np.linalg.norm(o, axis=1, keepdims=True)).astype(np.float32)
    tgt = (rng.uniform(-1, 1, size=(n, 3)) * target_scale).astype(np.float32)
    return np.concatenate([o, tgt - o], axis=1).astype(np.float32)


def with_uv(tri, uv=None):
    """(n, 3, 3) vertex positions (+ (n, 3, 2) texcoords, default 0) -> (n, 15) faces"""
    tri = np.asarray(tri, np.float32)
    uv = np.zeros((len(tri), 3, 2), np.float32) if uv is None else np.asarray(uv, np.float32)
    return np.concatenate([tri, uv], axis=2).reshape(len(tri), 15)


def aimed_rays(rng, targets, distance):
    """rays towards the given points from random directions, origins `distance` (scalar or per ray) away"""
    n = len(targets)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (targets + d * np.reshape(distance, (-1, 1))).astype(np.float32)
    return np.concatenate([o, targets.astype(np.float32) - o], axis=1).astype(np.float32)


def soup(rng, n=3000, dup=((0, 500), (100, 300))):
    """n random triangles in [-2, 2]^3 followed by exact copies of the face ranges `dup`: returns (faces, n); faces n.. are the copies"""
    c = rng.uniform(-2, 2, size=(n, 1, 3))
    tri = (c + rng.normal(scale=0.15, size=(n, 3, 3))).astype(np.float32)
    uv = rng.uniform(0, 1, size=(n, 3, 2)).astype(np.float32)
    faces = np.concatenate([tri, uv], axis=2).reshape(n, 15)
    return np.concatenate([faces] + [faces[a:b] for a, b in dup]), n


def flat_grid(g=40):
    """a flat g x g grid in the plane y = 0 (boxes of zero thickness) plus a vertical wall: returns (faces, xs = the grid lines)"""
    xs = np.linspace(-2, 2, g + 1, dtype=np.float32)
    f = []
    for i in range(g):
        for j in range(g):
            a = (xs[i], 0, xs[j], 0, 0); b = (xs[i + 1], 0, xs[j], 1, 0); c = (xs[i + 1], 0, xs[j + 1], 1, 1); d = (xs[i], 0, xs[j + 1], 0, 1)
            f.append(np.array(a + d + c, np.float32)); f.append(np.array(a + c + b, np.float32))     # facing +y
    for i in range(g):
        for j in range(g):
            a = (xs[i], xs[j] + 2, -1, 0, 0); b = (xs[i + 1], xs[j] + 2, -1, 1, 0); c = (xs[i + 1], xs[j + 1] + 2, -1, 1, 1); d = (xs[i], xs[j + 1] + 2, -1, 0, 1)
            f.append(np.array(a + b + c, np.float32)); f.append(np.array(a + c + d, np.float32))     # facing +z
    return np.array(f, np.float32), xs


def flat_grid_rays(rng, xs, n):
    """4 n rays for flat_grid: straight down (two zero components), along -z, straight down from the grid lines (edges shared by
    triangles: ties between neighbours), grazing (almost inside the plane)"""
    g = len(xs) - 1
    o = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    o[:, 1] = rng.uniform(0.5, 3, size=n)
    rays = []
    down = np.tile(np.array([0, -1, 0], np.float32), (n, 1))                       # two zero components
    rays.append(np.concatenate([o, down], axis=1))
    o2 = o.copy(); o2[:, 2] = 3
    rays.append(np.concatenate([o2, np.tile(np.array([0, 0, -1], np.float32), (n, 1))], axis=1))
    # origins on the grid lines (edges shared by triangles), axis-parallel: ties between neighbours
    og = np.stack([xs[rng.integers(0, g + 1, n)], np.full(n, 1.0, np.float32), xs[rng.integers(0, g + 1, n)]], axis=1).astype(np.float32)
    rays.append(np.concatenate([og, down], axis=1))
    # grazing: almost inside the plane
    dg = rng.normal(size=(n, 3)).astype(np.float32); dg[:, 1] = -np.abs(rng.normal(scale=1e-4, size=n)).astype(np.float32)
    og2 = o.copy(); og2[:, 1] = rng.uniform(1e-4, 1e-2, size=n)
    rays.append(np.concatenate([og2, dg], axis=1))
    return np.concatenate(rays).astype(np.float32)


def needles(rng, n=2000):
    """n needles (two long edges, one of 1e-3) and n tiny triangles (1e-4) in [-1, 1]^3: returns (faces, (2n, 3, 3) vertex positions)"""
    base = rng.uniform(-1, 1, size=(n, 3))
    dirs = rng.normal(size=(n, 3))
    tri = np.stack([base, base + dirs * rng.uniform(0.5, 2.0, size=(n, 1)), base + rng.normal(scale=1e-3, size=(n, 3))], axis=1)   # needles
    tiny = rng.uniform(-1, 1, size=(n, 1, 3)) + rng.normal(scale=1e-4, size=(n, 3, 3))
    tri = np.concatenate([tri, tiny]).astype(np.float32)
    return with_uv(tri), tri


def needles_rays(rng, tri, near=20000, far=10000, aimed=10000):
    rays = np.concatenate([rays_around(rng, near, 3.0, 1.0), rays_around(rng, far, 2000.0, 1.0)])
    # aim a share of the rays straight at triangle centroids so that tiny ones are hit
    cent = tri.mean(axis=1)[rng.integers(0, len(tri), aimed)]
    o = rays_around(rng, aimed, 4.0)[:, :3]
    return np.concatenate([rays, np.concatenate([o, cent - o], axis=1)]).astype(np.float32)


def far_soup(rng, m=800):
    """m needle-like triangles (one edge of 2e-2) in [-1, 1]^3: the far-origin sweep's second mesh"""
    base = rng.uniform(-1, 1, size=(m, 3))
    tri = np.stack([base, base + rng.normal(size=(m, 3)) * rng.uniform(0.3, 1.5, size=(m, 1)), base + rng.normal(scale=2e-2, size=(m, 3))], axis=1).astype(np.float32)
    return with_uv(tri)


# ---- the cases added for the device tier ---------------------------------------------------------------------------------------------
CHAIN_AXIS = np.array([0.8, 0.48, 0.36])        # (unit length; not an axis of the boxes)
# count, ratio, exponent of the first triangle.  Measured by ptx_debug_bvh_check / ptx_debug_bvh_visits (tests/test_bvh.py asserts the
# inequalities): CHAIN wide stack need 34, binary depth 29; CHAIN_DEEP need 40, depth 35; 55 distinct triangles hit in both.
CHAIN = (110, 1.6, 40)
CHAIN_DEEP = (140, 1.6, 40)


def chain(rng, count, ratio, first_exp):
    """`count` triangles, triangle k around the point ratio^(first_exp - k) * CHAIN_AXIS with vertex scatter a quarter of that distance:
    every triangle is as far from the rest of the chain as it is large, so binned SAH splits ONE triangle off per level.  Returns
    (faces, centroids, scales).  (rayTriangle accepts a hit only if its determinant is >= FLT_EPSILON: triangles smaller than about
    1e-3 cannot be hit at all -- the tail of a chain only deepens the tree.)"""
    x = np.float64(ratio) ** (first_exp - np.arange(count))
    tri = (x[:, None, None] * CHAIN_AXIS[None, None, :] + 0.25 * x[:, None, None] * rng.normal(size=(count, 3, 3))).astype(np.float32)
    return with_uv(tri), tri.mean(axis=1).astype(np.float64), x


def chain_rays(rng, cent, scales, n, hittable=1e-3):
    """n rays aimed at jittered centroids of the triangles that can be hit, origins one to three times the target's own scale away"""
    k = rng.integers(0, int((scales >= hittable).sum()), n)
    tgt = cent[k] + 0.05 * scales[k][:, None] * rng.normal(size=(n, 3))
    return aimed_rays(rng, tgt, scales[k] * rng.uniform(1.0, 3.0, size=n))


def chain_case(rng, n_rays=8000):
    """stack need of the four-wide walk above BVH_STACK, at least 25 distinct triangles hit (asserted in tests/test_bvh.py)"""
    faces, cent, x = chain(rng, *CHAIN)
    return faces, chain_rays(rng, cent, x, n_rays)


def chain_deep_case(rng, n_rays=8000):
    """binary depth of at least BVH_STACK: not even the front-to-back binary walk fits (asserted in tests/test_bvh.py)"""
    faces, cent, x = chain(rng, *CHAIN_DEEP)
    return faces, chain_rays(rng, cent, x, n_rays)


def coincident(rng, n=64, n_rays=6000):
    """n triangles with one common centroid, each a random rotation (and size) of an equilateral triangle about it"""
    c = np.array([0.3, -0.2, 0.1])
    tri = np.zeros((n, 3, 3))
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        r = rng.uniform(0.5, 1.5)
        for j in range(3):
            a = 2 * np.pi * j / 3
            tri[k, j] = r * (np.cos(a) * q[:, 0] + np.sin(a) * q[:, 1])
    tri -= tri.mean(axis=1, keepdims=True)          # (centroids exactly equal before the float32 rounding of c + v)
    faces = with_uv(tri + c, rng.uniform(0, 1, size=(n, 3, 2)))
    tgt = c + rng.uniform(-1, 1, size=(n_rays, 3)) * 0.8
    return faces, aimed_rays(rng, tgt, rng.uniform(2.0, 6.0, size=n_rays))


def soup_nan(rng, n=2800, n_rays=12000):
    """soup with duplicates + one triangle with a NaN vertex + ten zero-area triangles (two equal vertices), spread through the list:
    returns (faces, rays, n) -- faces n.. are duplicates (in position; each with texcoords of its own, so that the winner of a tie can be
    told from the hit's texcoords) or degenerate and must never win"""
    faces, n = soup(rng, n)
    faces[n:, [3, 4, 8, 9, 13, 14]] = rng.uniform(0, 1, size=(len(faces) - n, 6))      # same triangle, texcoords of its own: who won a tie shows
    bad = faces[rng.integers(0, n, 11)].copy()
    bad[0, 5:8] = np.nan                                     # second vertex NaN
    bad[1:, 10:15] = bad[1:, 5:10]                           # third vertex = second: zero area
    faces = np.concatenate([faces[:n + 350], bad[:6], faces[n + 350:], bad[6:]])
    return faces.astype(np.float32), rays_around(rng, n_rays, 5.0, 2.0), n


def hull_cut(k):
    """the first k faces of a 48-face hull (an open surface)"""
    return hull(4, 6)[:k].copy()


def hull_cut_rays(rng, n=4000):
    return np.concatenate([rays_around(rng, n, 5.0, 1.2), rays_around(rng, n // 4, 0.1, 1.5)])


def axis_parallel_rays(rng, n, lo, hi):
    """n rays per axis and sign, origins on the far side of the box [lo, hi]: one non-zero direction component"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = np.maximum(hi - lo, 1e-3)
    rays = []
    for ax in range(3):
        for sg in (-1.0, 1.0):
            o = rng.uniform(lo, hi, size=(n, 3))
            o[:, ax] = (hi[ax] + ext[ax]) if sg < 0 else (lo[ax] - ext[ax])
            d = np.zeros((n, 3)); d[:, ax] = sg
            rays.append(np.concatenate([o, d], axis=1))
    return np.concatenate(rays).astype(np.float32)


def far_rays(rng, n, size, ratios=(1e3, 1e4, 1e5, 1e6)):
    """n rays per ratio from `ratio` mesh sizes away towards the mesh (far-origin sweep)"""
    return np.concatenate([rays_around(rng, n, size * r, 0.5 * size) for r in ratios])
