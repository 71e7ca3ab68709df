"""float64 restatement of the denoiser's temporal reuse (include/mi355x_pathtracer.h: ptx_denoise_temporal), written from
the definition and nothing else: tests/test_temporal_cpu.py checks it by hand, tests/test_gpu_temporal.py holds the device to it.

    every hit pixel p of the current G-buffer, P = the previous (hist) camera:
        solve x_p - P.position = s (view - right pl.x (u - W/2) - up pl.y (v - H/2)) for (s, s u, s v); s <= 0: nothing
        taps (floor(u) + i, floor(v) + j) of bilinear weight w_q > 0, accepted when inside the frame, a hit in hist, same geom and
        material id, dot(n_p, n_q) >= normal_cos and |dot(n_p, x_q - x_p)| <= plane_tolerance |x_p - P.position|;
        specular materials accept nothing unless specular_history
        S = sum of accepted w_q > 0: n_h = min(sum w_q n_q / S, max_history); n_h > 0: h = sum w_q D_q / S * max(a_p, 1e-3)
    c = rgb / spp (fp32 division); miss or n_h == 0: mix = c, n = spp; else mix = (spp c + n_h h) / (spp + n_h), n = spp + n_h
    the state a call leaves: D = mix / max(albedo, 1e-3) on hit pixels (mix on misses) and n
"""
import numpy as np

EPS = 1e-4          # what counts as "near a threshold" for the comparison with the fp32 device (tests/test_gpu_temporal.py)


def camera_dict(cam):
    """the fields of a ctypes ptx_camera (Scene.camera) the reprojection reads, copied"""
    f = lambda a: np.array(list(a), np.float64)
    return dict(position=f(cam.position), view=f(cam.view), right=f(cam.right), up=f(cam.up), pl=f(cam.pixelLength),
                W=int(cam.resolution[0]), H=int(cam.resolution[1]))


def specular_flags(materials):
    """per material: hasReflective > 0 or hasRefractive > 0 (Scene.dump()['materials'], 11 floats each)"""
    m = np.asarray(materials, np.float64).reshape(-1, 11)
    return (m[:, 7] > 0) | (m[:, 8] > 0)


def project(cam, x):
    """(s, u, v) of world points x (..., 3) in camera `cam` (camera_dict): the linear system in (s, s u, s v)"""
    R = cam["right"] * cam["pl"][0]
    U = cam["up"] * cam["pl"][1]
    A = cam["view"] + R * (cam["W"] / 2.0) + U * (cam["H"] / 2.0)
    M = np.stack([A, -R, -U], axis=1)                     # columns
    d = np.asarray(x, np.float64).reshape(-1, 3) - cam["position"]
    sol = np.linalg.solve(M, d.T)                         # (3, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        s, u, v = sol[0], sol[1] / sol[0], sol[2] / sol[0]
    shp = np.shape(x)[:-1]
    return s.reshape(shp), u.reshape(shp), v.reshape(shp)


def state(gbuf, mix, n):
    """D and n of the state a call leaves, from its G-buffer, mix (H, W, 3) and n (H, W)"""
    hit = np.asarray(gbuf["hit"]) != 0
    mix = np.asarray(mix, np.float64)
    a = np.maximum(np.asarray(gbuf["albedo"], np.float64), 1e-3)
    return dict(gbuf=gbuf, D=np.where(hit[..., None], mix / a, mix), n=np.asarray(n, np.float64))


def reproject(prev_cam, cur, prev, spec, max_history=16, specular_history=0, normal_cos=0.9, plane_tolerance=0.01, reasons=None):
    """cur: the current G-buffer (Tracer.gbuffer()); prev: state() of the previous segment, prev_cam its camera_dict.
    Returns h (H, W, 3), n_h (H, W) and `near` (H, W): pixels where a decision of the definition is within EPS (relative) of its
    threshold, or u or v within EPS pixels of an integer -- where fp32 and float64 may decide differently.
    reasons: a dict that receives `near` by reason, "s", "grid" (u or v), "normal" and "plane" (H, W) each; their union is `near`.  It
    also receives what tests/temporalcases.py asks of a case: "u", "v" (NaN where there is no projection), "capped" (sum w n / S above
    max_history), and per test "normal_rejected", "normal_accepted", "plane_rejected", "plane_accepted": pixels with such a tap."""
    hit = np.asarray(cur["hit"]) != 0
    H, W = hit.shape
    xp = np.asarray(cur["position"], np.float64)
    npn = np.asarray(cur["normal"], np.float64)
    mat, geom = np.asarray(cur["material"]), np.asarray(cur["geom"])
    pg = prev["gbuf"]
    phit = np.asarray(pg["hit"]) != 0
    pxq, pnq = np.asarray(pg["position"], np.float64), np.asarray(pg["normal"], np.float64)
    pmat, pgeom = np.asarray(pg["material"]), np.asarray(pg["geom"])
    spec = np.asarray(spec, bool)
    is_spec = (mat >= 0) & (mat < len(spec)) & spec[np.clip(mat, 0, len(spec) - 1)]
    considered = hit if specular_history else hit & ~is_spec
    s, u, v = project(prev_cam, xp)
    ok = considered & (s > 0) & np.isfinite(u) & np.isfinite(v)
    smax = np.abs(np.where(considered, s, 0.0)).max() if considered.any() else 1.0
    near_s = considered & (np.abs(s) <= EPS * smax)
    uu, vv = np.where(ok, u, -10.0), np.where(ok, v, -10.0)
    u0, v0 = np.floor(uu), np.floor(vv)
    fu, fv = uu - u0, vv - v0
    near_grid = ok & ((fu <= EPS) | (fu >= 1 - EPS) | (fv <= EPS) | (fv >= 1 - EPS))
    near_normal, near_plane = np.zeros((H, W), bool), np.zeros((H, W), bool)
    taps = {k: np.zeros((H, W), bool) for k in ("normal_rejected", "normal_accepted", "plane_rejected", "plane_accepted")}
    dist = np.linalg.norm(xp - prev_cam["position"], axis=-1)
    lim = plane_tolerance * dist
    sw, sn, sd = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W, 3))
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = u0.astype(np.int64) + i, v0.astype(np.int64) + j
            wt = (fu if i else 1 - fu) * (fv if j else 1 - fv)
            inside = ok & (wt > 0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            same = inside & phit[cy, cx] & (pmat[cy, cx] == mat) & (pgeom[cy, cx] == geom)
            dn = (npn * pnq[cy, cx]).sum(-1)
            pl = np.abs((npn * (pxq[cy, cx] - xp)).sum(-1))
            near_normal |= same & (np.abs(dn - normal_cos) <= EPS * max(abs(normal_cos), 1e-3))
            near_plane |= same & (dn >= normal_cos) & (np.abs(pl - lim) <= EPS * lim + 1e-9)
            acc = same & (dn >= normal_cos) & (pl <= lim)
            taps["normal_rejected"] |= same & ~(dn >= normal_cos)
            taps["normal_accepted"] |= same & (dn >= normal_cos)
            taps["plane_rejected"] |= same & (dn >= normal_cos) & ~(pl <= lim)
            taps["plane_accepted"] |= acc
            w = np.where(acc, wt, 0.0)
            sw += w
            sn += w * prev["n"][cy, cx]
            sd += w[..., None] * prev["D"][cy, cx]
    safe = np.where(sw > 0, sw, 1.0)
    nh = np.where(sw > 0, np.minimum(sn / safe, float(max_history)), 0.0)
    a = np.maximum(np.asarray(cur["albedo"], np.float64), 1e-3)
    h = np.where((nh > 0)[..., None], sd / safe[..., None] * a, 0.0)
    near = near_s | near_grid | near_normal | near_plane
    if reasons is not None:
        reasons.update(taps, s=near_s, grid=near_grid, normal=near_normal, plane=near_plane, u=np.where(ok, u, np.nan),
                       v=np.where(ok, v, np.nan), capped=(sw > 0) & (sn / safe > float(max_history)))
    return h, nh, near


def mix(rgb, spp, hit, h, nh):
    """the mix and the new sample count; rgb (H, W, 3) the accumulation buffer (float32), spp its iterations.  Also returns c, the
    current frame alone, as the device computes it (float32)."""
    hit = np.asarray(hit) != 0
    c32 = np.asarray(rgb, np.float32) / np.float32(spp)          # the fp32 division of ptx_denoise
    c = c32.astype(np.float64)
    use = hit & (nh > 0)
    m = (spp * c + nh[..., None] * h) / (spp + nh)[..., None]
    out = np.where(use[..., None], m, c)
    n = np.where(use, spp + nh, float(spp))
    return out, n, c32


def synthetic_camera(W=64, H=48, position=(0.0, 0.0, 10.0), pl=0.01):
    """a pinhole looking down -z with an orthonormal basis, pixelLength pl in both axes (camera_dict layout)"""
    return dict(position=np.array(position, np.float64), view=np.array([0.0, 0.0, -1.0]), right=np.array([1.0, 0.0, 0.0]),
                up=np.array([0.0, 1.0, 0.0]), pl=np.array([pl, pl]), W=W, H=H)


def plane_gbuffer(cam, z=0.0, material=1, geom=2, albedo=0.5):
    """G-buffer of the plane z = `z` seen from `cam` through its pixel-centre rays (a hit everywhere)"""
    W, H = cam["W"], cam["H"]
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = (cam["view"][None, None] - cam["right"] * cam["pl"][0] * (x - W / 2.0)[..., None]
         - cam["up"] * cam["pl"][1] * (y - H / 2.0)[..., None])
    t = (z - cam["position"][2]) / d[..., 2]
    pos = cam["position"] + t[..., None] * d
    nrm = np.zeros((H, W, 3)); nrm[..., 2] = 1.0
    return dict(hit=np.ones((H, W), bool), position=pos, normal=nrm, albedo=np.full((H, W, 3), albedo),
                material=np.full((H, W), material, np.int32), geom=np.full((H, W), geom, np.int32))
