"""A float64 reference of the three per-geom intersection tests (numpy, no device, no oracle), written from the mathematics.

What each test computes, as ptx_kat_geom_test / o_geom_test report it (out10 = t, point, normal, u, v, outside):

  every primitive   the world ray (o, d; d need not be a unit vector) is taken to object space by the geom's inverse matrix, the direction
                    normalised there; the hit point goes back through the geom's matrix and the object-space normal through the
                    inverse transpose, then normalised.
  cube              the unit cube [-1/2, 1/2]^3: slab test.  Entering parameter tn = the largest of the three near planes', leaving
                    parameter tf = the smallest of the far planes'; a hit if tf >= tn and tf > 0; from outside (tn > 0) the hit is at
                    tn, from inside at tf.  The normal is the hit plane's axis, pointing against the ray on that axis (so from inside it
                    points inwards); t = the WORLD distance |o - point|.
  sphere            radius 1/2: the roots -b -+ sqrt(b^2 - c) of |o + t d|^2 = 1/4.  Both positive: the smaller one, outside; one
                    positive: that one, from inside, the normal reversed; t = the world distance.
  mesh              a loop over ALL faces with single-sided Moeller-Trumbore (a face counts if its determinant e1 . (d x e2) is at least
                    FLT_EPSILON, 0 <= u <= 1, 0 <= v, u + v <= 1, t >= 0); the face with the smallest distance wins, the lowest index
                    among equals; t = that OBJECT-space distance (meshIntersectionTest returns it as it is, which is why a scaled mesh
                    loses or wins comparisons with the world distances of the other primitives); u, v = the interpolated texcoords;
                    outside = normal . d < 0.  `t_world` is reported beside it.

Inputs are the fp32 rays and the fp32 matrices exactly as the tracer holds them (geom_mats of Scene.dump(): transform, inverse, inverse
transpose, column-major), widened to float64: their rounding is not part of any error measured against this module.

Extras for the tests: `side` (cube: axis * 2 + (normal component > 0); sphere: outside; mesh: the face), `margin` (mesh: the smallest
barycentric of the winner; cube: the distance from the hit to the nearest edge of its face in units of the cube's size; sphere:
1 - impact parameter / radius, negative for a miss), and for a mesh the K nearest faces hit with their distances (`near_face`,
`near_t`; near_t[:, 1] is the runner-up's distance, inf without one); `clear` (the decision has a margin of CLEAR, a miss too) and `away`
(how many sizes from the geom's centre the ray starts; a mesh's size is its largest extent)."""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
U = 2.0 ** -24                                  # the unit roundoff of binary32
NEAR_K = 4
CLEAR = 1e-2                                    # the margin from which a decision counts as well-conditioned
NUDGE = float(np.float32(0.0001))               # getPointOnRay reports the point at t - .0001f along the unit direction, not at t


def matrices(gm48):
    """geom_mats row of Scene.dump() -> (transform, inverse, inverse transpose) as 4x4 float64, M @ column vector"""
    gm = np.asarray(gm48, np.float32).astype(np.float64)
    return tuple(gm[k:k + 16].reshape(4, 4).T for k in (0, 16, 32))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _object_ray(Ti, rays):
    r = np.asarray(rays, np.float32).astype(np.float64)
    o, d = r[:, :3], r[:, 3:6]
    return o, d, o @ Ti[:3, :3].T + Ti[:3, 3], _unit(d @ Ti[:3, :3].T)


def _finish(T, TiT, o_world, hit, t_obj, qo, qd, n_obj):
    """object-space hit -> world point, unit world normal, world distance (NaN where there is no hit)"""
    p_obj = qo + (t_obj - NUDGE)[:, None] * qd
    point = p_obj @ T[:3, :3].T + T[:3, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        normal = _unit(n_obj @ TiT[:3, :3].T)
    t_world = np.linalg.norm(o_world - point, axis=1)
    bad = ~hit
    point[bad], normal[bad], t_world[bad] = np.nan, np.nan, np.nan
    return p_obj, point, normal, t_world


def _out10(hit, t, point, normal, uv, outside):
    out = np.zeros((len(hit), 10))
    out[:, 0] = np.where(hit, t, -1.0)
    out[:, 1:4], out[:, 4:7], out[:, 7:9] = np.where(hit[:, None], point, 0.0), np.where(hit[:, None], normal, 0.0), np.where(hit[:, None], uv, 0.0)
    out[:, 9] = np.where(hit, outside, 1.0)
    return out


def cube(gm48, rays):
    T, Ti, TiT = matrices(gm48)
    o, d, qo, qd = _object_ray(Ti, rays)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-0.5 - qo) / qd, (0.5 - qo) / qd
    ta, tb = np.minimum(t1, t2), np.maximum(t1, t2)
    # (a direction component of exactly 0: the planes are at -+inf, or NaN when the origin lies in one of them -- such an axis never
    # decides anything, so it is taken out of both extremes)
    ta, tb = np.where(np.isnan(ta), -np.inf, ta), np.where(np.isnan(tb), np.inf, tb)
    an, af = ta.argmax(axis=1), tb.argmin(axis=1)
    tn, tf = ta.max(axis=1), tb.min(axis=1)
    hit = (tf >= tn) & (tf > 0)
    outside = tn > 0
    axis = np.where(outside, an, af)
    t_obj = np.where(outside, tn, tf)
    n_obj = np.zeros_like(qo)
    rows = np.arange(len(qo))
    n_obj[rows, axis] = -np.sign(qd[rows, axis])
    p_obj, point, normal, t_world = _finish(T, TiT, o, hit, np.where(hit, t_obj, np.nan), qo, qd, n_obj)
    side = axis * 2 + (n_obj[rows, axis] > 0)
    others = np.abs(qo + np.where(hit, t_obj, np.nan)[:, None] * qd)              # (the hit itself, not the reported point .0001 before it)
    others[rows, axis] = -np.inf
    margin = 0.5 - others.max(axis=1)
    half = 0.5 + CLEAR                                   # a miss is clear if the cube grown by CLEAR is missed too
    with np.errstate(divide="ignore", invalid="ignore"):
        g1, g2 = (-half - qo) / qd, (half - qo) / qd
    ga, gb = np.minimum(g1, g2), np.maximum(g1, g2)
    ga, gb = np.where(np.isnan(ga), -np.inf, ga), np.where(np.isnan(gb), np.inf, gb)
    grown_hit = (gb.min(axis=1) >= ga.max(axis=1)) & (gb.min(axis=1) > 0)
    clear = np.where(hit, margin >= CLEAR, ~grown_hit)
    return dict(away=np.linalg.norm(qo, axis=1), clear=clear, hit=hit, t=np.where(hit, t_world, -1.0), t_world=t_world, point=point, normal=normal, uv=np.zeros((len(hit), 2)),
                outside=outside & hit | ~hit, side=np.where(hit, side, -1), margin=np.where(hit, margin, np.nan),
                out10=_out10(hit, t_world, point, normal, np.zeros((len(hit), 2)), outside))


def sphere(gm48, rays):
    T, Ti, TiT = matrices(gm48)
    o, d, qo, qd = _object_ray(Ti, rays)
    b = (qo * qd).sum(axis=1)
    perp = qo - b[:, None] * qd                                    # the origin's component across the ray: its length is the impact parameter
    imp2 = (perp * perp).sum(axis=1)
    rad = 0.25 - imp2                                              # = b^2 - (|o|^2 - 1/4) without the cancellation
    root = np.sqrt(np.maximum(rad, 0.0))
    r1, r2 = -b + root, -b - root
    hit = (rad >= 0) & ~((r1 < 0) & (r2 < 0))
    outside = (r1 > 0) & (r2 > 0)
    t_obj = np.where(outside, np.minimum(r1, r2), np.maximum(r1, r2))
    p0 = qo + (t_obj - NUDGE)[:, None] * qd               # (the normal is taken at the reported point)
    _, point, normal, t_world = _finish(T, TiT, o, hit, np.where(hit, t_obj, np.nan), qo, qd, np.where(outside[:, None], p0, -p0))
    margin = 1.0 - np.sqrt(imp2) / 0.5
    # (a ray that starts within CLEAR of the surface, or whose sphere lies within CLEAR behind it, is not a clear decision either)
    clear = (np.abs(margin) >= CLEAR) & (np.abs(np.linalg.norm(qo, axis=1) - 0.5) >= CLEAR * 0.5)
    return dict(away=np.linalg.norm(qo, axis=1), clear=clear, hit=hit, t=np.where(hit, t_world, -1.0), t_world=t_world, point=point, normal=normal, uv=np.zeros((len(hit), 2)),
                outside=outside & hit | ~hit, side=np.where(hit, outside.astype(np.int64), -1), margin=margin,
                out10=_out10(hit, t_world, point, normal, np.zeros((len(hit), 2)), outside))


def mesh_face_distances(faces15, qo, qd, chunk=128):
    """every face against every ray: (n, F) distances, inf where the face is not hit (the winner's barycentrics are recomputed by the
    caller) -- the brute-force loop, vectorised over rays and `chunk` faces at a time -- and per ray `grazed`: some face is missed by
    less than CLEAR (in a barycentric or in the determinant's threshold) or hit with a determinant that close to the threshold"""
    f = np.asarray(faces15, np.float32).astype(np.float64).reshape(-1, 3, 5)
    out = np.full((len(qo), len(f)), np.inf)
    grazed = np.zeros(len(qo), bool)
    for c in range(0, len(f), chunk):
        v0, v1, v2 = (f[None, c:c + chunk, k, :3] for k in range(3))
        e1, e2 = v1 - v0, v2 - v0
        p = np.cross(qd[:, None, :], e2)
        a = (e1 * p).sum(axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / a
            s = qo[:, None, :] - v0
            u = inv * (s * p).sum(axis=2)
            q = np.cross(s, e1)
            v = inv * (qd[:, None, :] * q).sum(axis=2)
            t = inv * (e2 * q).sum(axis=2)
            ok = (a >= FLT_EPSILON) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= 0)
            near = (a >= FLT_EPSILON * (1 - CLEAR)) & (u >= -CLEAR) & (v >= -CLEAR) & (u + v <= 1 + CLEAR) & (t >= 0)
            thin = ok & (a < FLT_EPSILON * (1 + CLEAR))
        out[:, c:c + chunk] = np.where(ok, t, np.inf)
        grazed |= (near & ~ok).any(axis=1) | thin.any(axis=1)
    return out, grazed


def mesh(gm48, faces15, rays):
    T, Ti, TiT = matrices(gm48)
    o, d, qo, qd = _object_ray(Ti, rays)
    f = np.asarray(faces15, np.float32).astype(np.float64).reshape(-1, 3, 5)
    dist, grazed = mesh_face_distances(faces15, qo, qd)
    rows = np.arange(len(qo))
    near, near_t = np.full((len(qo), NEAR_K), -1), np.full((len(qo), NEAR_K), np.inf)
    for k in range(min(NEAR_K, dist.shape[1])):                                 # (argmin: the lowest index among equal distances first)
        j = dist.argmin(axis=1)
        near_t[:, k] = dist[rows, j]
        near[:, k] = np.where(np.isfinite(near_t[:, k]), j, -1)
        dist[rows, j] = np.inf
    face, t_obj = near[:, 0], near_t[:, 0]
    hit = face >= 0
    w = f[np.maximum(face, 0)]
    v0, v1, v2 = w[:, 0, :3], w[:, 1, :3], w[:, 2, :3]
    e1, e2 = v1 - v0, v2 - v0
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.cross(qd, e2)
        inv = 1.0 / (e1 * p).sum(axis=1)
        s = qo - v0
        bu = inv * (s * p).sum(axis=1)
        bv = inv * (qd * np.cross(s, e1)).sum(axis=1)
        n_obj = _unit(np.cross(e1, e2))
    bw = 1.0 - bu - bv
    uv = bw[:, None] * w[:, 0, 3:5] + bu[:, None] * w[:, 1, 3:5] + bv[:, None] * w[:, 2, 3:5]
    _, point, normal, t_world = _finish(T, TiT, o, hit, np.where(hit, t_obj, np.nan), qo, qd, n_obj)
    with np.errstate(invalid="ignore"):
        outside = (normal * d).sum(axis=1) < 0
    margin = np.minimum(np.minimum(bu, bv), bw)
    with np.errstate(invalid="ignore", divide="ignore"):
        face_normal = _unit(_unit(np.cross(f[:, 1, :3] - f[:, 0, :3], f[:, 2, :3] - f[:, 0, :3])) @ TiT[:3, :3].T)      # (F, 3), world
    with np.errstate(invalid="ignore"):
        clear = np.where(hit, (margin >= CLEAR) & ~(near_t[:, 1] <= t_obj * (1 + 64 * U)), True) & ~grazed
    size = float((f[:, :, :3].max(axis=(0, 1)) - f[:, :, :3].min(axis=(0, 1))).max())
    return dict(away=np.linalg.norm(qo, axis=1) / size, clear=clear, near_normal=np.where((near >= 0)[:, :, None], face_normal[np.maximum(near, 0)], 0.0), hit=hit, t=np.where(hit, t_obj, -1.0), t_world=t_world, point=point, normal=normal, uv=np.where(hit[:, None], uv, 0.0),
                outside=outside & hit | ~hit, side=face, margin=np.where(hit, margin, np.nan), near_face=near, near_t=near_t,
                out10=_out10(hit, t_obj, point, normal, uv, outside))


def intersect(kind, gm48, rays, faces15=None):
    if kind == "cube":
        return cube(gm48, rays)
    if kind == "sphere":
        return sphere(gm48, rays)
    return mesh(gm48, faces15, rays)


# ---- reading a build's out10 against the reference ---------------------------------------------------------------------------------------
def cube_side_normals(gm48):
    """the six world normals a cube can report, index = axis * 2 + (sign > 0)"""
    _, _, TiT = matrices(gm48)
    n = np.zeros((6, 3))
    for s in range(6):
        n[s, s // 2] = 1.0 if s % 2 else -1.0
    return _unit(n @ TiT[:3, :3].T)


def side_of(kind, gm48, A, out10):
    """which face / side a build's answer is: cube = the tabulated normal nearest to the reported one; sphere = its outside flag;
    mesh = the one of the reference's NEAR_K nearest faces that lies at the reported distance and has the reported normal, both
    within 2^-10 (the lowest index among exact copies), -2 if none does: a face the reference does not know among its nearest.
    -1 = a miss."""
    out10 = np.asarray(out10, np.float64)
    got_hit = out10[:, 0] > 0
    if kind == "sphere":
        side = (out10[:, 9] != 0).astype(np.int64)
    elif kind == "cube":
        side = (out10[:, 4:7] @ cube_side_normals(gm48).T).argmax(axis=1)
    else:
        with np.errstate(invalid="ignore"):
            gap = np.abs(A["near_t"] - out10[:, :1])
            cand = np.isfinite(gap) & (gap <= 2.0 ** -10 * np.abs(out10[:, :1]))
            cand &= np.linalg.norm(A["near_normal"] - out10[:, None, 4:7], axis=2) <= 2.0 ** -10
        # (distances alone cannot tell neighbours apart from far away: among the faces at the reported distance, the one whose normal
        # is the reported one; exact copies of a face share both, and argmax takes the first, the lower index)
        match = np.where(cand, (A["near_normal"] * out10[:, None, 4:7]).sum(axis=2), -np.inf)
        j = match.argmax(axis=1)
        rows = np.arange(len(out10))
        side = np.where(cand[rows, j], A["near_face"][rows, j], -2)
    return np.where(got_hit, side, -1)


def decisions(kind, gm48, A, out10):
    """-> (agree: the build reports A's hit or miss, A's face or side and A's outside flag; same_hit: both hit, same face or side)"""
    side = side_of(kind, gm48, A, out10)
    got_hit = np.asarray(out10)[:, 0] > 0
    same_hit = A["hit"] & got_hit & (side == A["side"])
    agree = np.where(A["hit"], same_hit & ((np.asarray(out10)[:, 9] != 0) == A["outside"]), ~got_hit)
    return agree, same_hit


def scales(kind, gm48, A, rays):
    """What each reported quantity is computed FROM, per ray: the yardstick a rounding error of u is multiplied by.  Worked out from
    the inputs and the reference alone:
      obj     the terms the object-space origin is a sum of, |inverse| |o| + |inverse's translation| (a small geom far from the world's
              origin has an object-space origin that is the difference of large numbers);
      pos     the world origin's and the world point's size plus `obj` carried back through the matrix (its largest singular value): the reported point, and a
              distance taken between two such points;
      normal  1, times the matrix's anisotropy (largest / smallest singular value: normalising after a non-uniform scale divides by a
              length the small axis dominates);
      sphere  its hit moves along the ray by (error across the ray) / cos(incidence), cos = sqrt(1 - (impact / r)^2): t, point and
              normal take that factor, and the normal is the object-space point over r = 1/2, so it takes (obj + r) / r as well.
    -> dict(t, point, normal)"""
    T, Ti, TiT = matrices(gm48)
    o = np.asarray(rays, np.float32).astype(np.float64)[:, :3]
    obj = np.linalg.norm(np.abs(o) @ np.abs(Ti[:3, :3]).T + np.abs(Ti[:3, 3]), axis=1)
    sv = np.linalg.svd(T[:3, :3], compute_uv=False)
    pos = np.linalg.norm(o, axis=1) + np.where(A["hit"], np.linalg.norm(np.nan_to_num(A["point"]), axis=1), 0.0) + sv.max() * obj
    normal = np.full(len(o), sv.max() / sv.min())
    if kind == "sphere":
        with np.errstate(invalid="ignore", divide="ignore"):
            kappa = 1.0 / np.sqrt(np.maximum(1.0 - (1.0 - A["margin"]) ** 2, 0.0))
        return dict(t=kappa * pos, point=kappa * pos, normal=normal * kappa * (obj + 0.5) / 0.5)
    return dict(t=obj if kind == "mesh" else pos, point=pos, normal=normal)


def errors(A, out10, rays, rows, sc):
    """|build - A| on `rows`: t relative to |t_A|; t_fwd, point and normal against `sc` = scales(...) -- t_fwd against the larger of
    |t_A| and its scale.  -> dict(t, t_fwd, point, normal)"""
    out10 = np.asarray(out10, np.float64)[rows]
    t, p, n = A["t"][rows], A["point"][rows], A["normal"][rows]
    et = np.abs(out10[:, 0] - t)
    return dict(t=et / np.abs(t), t_fwd=et / np.maximum(sc["t"][rows], np.abs(t)), point=np.linalg.norm(out10[:, 1:4] - p, axis=1) / sc["point"][rows],
                normal=np.linalg.norm(out10[:, 4:7] - n, axis=1) / sc["normal"][rows])
