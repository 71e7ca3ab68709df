"""float32 conditioning probe of the reprojection: the definitions of tests/temporal_ref.py, tests/variance_ref.py (temporal_variance) and
tests/temporal_measured_ref.py once more, in numpy, with every intermediate rounded to float32 and the operations in the order
pt_temporal.hip's reproject_pixel performs them: hist's camera inverted in double and rounded once (pt_temporal_camera), the projection
as three dot products and two divisions, the taps row by row, the sums accumulated tap by tap, and for the measured variant the weights
of V_h and mu_h from the projection redone in double.

As tests/denoise_f32.py, it is NOT a reference for the device and nothing that ran on a GPU is ever compared with it.  Its one use
(tests/test_temporal_grid_cpu.py) is to measure how far float32 arithmetic alone departs from the float64 restatement in a given case."""
import numpy as np

F = np.float32
FLOOR = F(1e-3)
LUM = (F(0.2126), F(0.7152), F(0.0722))


def lum(r, g, b):
    return LUM[0] * r + LUM[1] * g + LUM[2] * b


def camera(cam):
    """pt_temporal_camera: (pos float32 (3,), minv float32 (9,), valid, pos float64, minv float64); cam: a camera_dict or None"""
    if cam is None:
        return np.zeros(3, F), np.zeros(9, F), False, np.zeros(3), np.zeros(9)
    W, H = float(cam["W"]), float(cam["H"])
    R, U = cam["right"] * cam["pl"][0], cam["up"] * cam["pl"][1]
    A = cam["view"] + R * (W * 0.5) + U * (H * 0.5)
    m = np.stack([A, -R, -U], 1)
    det = (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
           + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.array([m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1], m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1],
                        m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2], m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2],
                        m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0], m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]) / det
        inv32 = inv.astype(F)
    valid = bool(det != 0.0 and np.isfinite(det) and np.isfinite(inv32).all())
    return cam["position"].astype(F), inv32, valid, cam["position"].astype(F).astype(np.float64), inv


def reproject(cur, rgb, spp, spec, cam, prev, variant=0, has_v=True, scatter=None, batches=0, max_history=16, specular_history=0,
              normal_cos=0.9, plane_tolerance=0.01):
    """one call of k_temporal_reproject (variant 0), k_reproject_variance (1) or k_reproject_measured (2) on the arrays of
    tests/temporalcases.py: returns dict(h (H, W, 3), nh, mix, n, D, V), float32"""
    hit = np.asarray(cur["hit"]) != 0
    H, W = hit.shape
    nrm, xp, alb = (np.ascontiguousarray(cur[k], F) for k in ("normal", "position", "albedo"))
    mat, geom = np.asarray(cur["material"]), np.asarray(cur["geom"])
    pg = prev["gbuf"]
    phit = np.asarray(pg["hit"]) != 0
    pn, px = np.ascontiguousarray(pg["normal"], F), np.ascontiguousarray(pg["position"], F)
    pmat, pgeom = np.asarray(pg["material"]), np.asarray(pg["geom"])
    pD, pN = np.ascontiguousarray(prev["D"], F), np.ascontiguousarray(prev["n"], F)
    pV = np.ascontiguousarray(prev["V"], F) if (has_v and variant >= 1) else np.zeros((H, W), F)
    spec = np.asarray(spec) != 0
    spp32, maxh, ncos, tol = F(spp), F(max_history), F(normal_cos), F(plane_tolerance)
    pos, minv, valid, pos64, minv64 = camera(cam)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = np.ascontiguousarray(rgb, F) / spp32
        a = np.where(hit[..., None], np.maximum(alb, FLOOR), F(1))
        q = np.zeros((H, W), F)
        if variant == 2:
            M, B = np.ascontiguousarray(scatter, F), F(batches)
            g = [LUM[k] / a[..., k] for k in range(3)]
            diag = g[0] * g[0] * M[..., 0] + g[1] * g[1] * M[..., 1] + g[2] * g[2] * M[..., 2]
            off = g[0] * g[1] * M[..., 3] + g[0] * g[2] * M[..., 4] + g[1] * g[2] * M[..., 5]
            q = np.where(hit, np.maximum((diag + F(2) * off) / (B - F(1)), F(0)), F(0))
        is_spec = (mat >= 0) & (mat < len(spec)) & spec[np.clip(mat, 0, len(spec) - 1)]
        considered = hit & valid & (bool(specular_history) | ~is_spec)
        dx, dy, dz = xp[..., 0] - pos[0], xp[..., 1] - pos[1], xp[..., 2] - pos[2]
        s = minv[0] * dx + minv[1] * dy + minv[2] * dz
        su = minv[3] * dx + minv[4] * dy + minv[5] * dz
        sv_ = minv[6] * dx + minv[7] * dy + minv[8] * dz
        u, v = su / s, sv_ / s
        ok = considered & (s > 0) & (u > -1) & (u < F(W)) & (v > -1) & (v < F(H))
        uu, vv = np.where(ok, u, F(0)), np.where(ok, v, F(0))
        uf, vf = np.floor(uu), np.floor(vv)
        u0, v0 = uf.astype(np.int64), vf.astype(np.int64)
        fu, fv = uu - uf, vv - vf
        lim = tol * np.sqrt(dx * dx + dy * dy + dz * dz)
        pfu = pfv = None
        if variant == 2:
            e = xp.astype(np.float64) - pos64
            ds = minv64[0] * e[..., 0] + minv64[1] * e[..., 1] + minv64[2] * e[..., 2]
            du = (minv64[3] * e[..., 0] + minv64[4] * e[..., 1] + minv64[5] * e[..., 2]) / ds
            dv = (minv64[6] * e[..., 0] + minv64[7] * e[..., 1] + minv64[8] * e[..., 2]) / ds
            pfu = np.clip(np.where(ok, du, 0.0) - uf.astype(np.float64), 0.0, 1.0).astype(F)
            pfv = np.clip(np.where(ok, dv, 0.0) - vf.astype(np.float64), 0.0, 1.0).astype(F)
        z = lambda: np.zeros((H, W), F)
        sd, sn, sw, sV = [z(), z(), z()], z(), z(), z()
        pd, pw, pv = [z(), z(), z()], z(), z()
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = u0 + i, v0 + j
                wt = (fu if i else F(1) - fu) * (fv if j else F(1) - fv)
                inside = ok & (wt > 0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                nq, xq = pn[cy, cx], px[cy, cx]
                same = inside & phit[cy, cx] & (pmat[cy, cx] == mat) & (pgeom[cy, cx] == geom)
                dn = nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1] + nrm[..., 2] * nq[..., 2]
                pl = (nrm[..., 0] * (xq[..., 0] - xp[..., 0]) + nrm[..., 1] * (xq[..., 1] - xp[..., 1])
                      + nrm[..., 2] * (xq[..., 2] - xp[..., 2]))
                acc = same & (dn >= ncos) & (np.abs(pl) <= lim)
                wa = np.where(acc, wt, F(0))
                dq = pD[cy, cx]
                for k in range(3):
                    sd[k] = sd[k] + np.where(acc, wt * dq[..., k], F(0))
                sn = sn + np.where(acc, wt * pN[cy, cx], F(0))
                sw = sw + wa
                sV = sV + np.where(acc, wt * pV[cy, cx], F(0))
                if variant == 2:
                    pt = (pfu if i else F(1) - pfu) * (pfv if j else F(1) - pfv)
                    for k in range(3):
                        pd[k] = pd[k] + np.where(acc, pt * dq[..., k], F(0))
                    pv = pv + np.where(acc, pt * pV[cy, cx], F(0))
                    pw = pw + np.where(acc, pt, F(0))
        have = sw > 0
        safe = np.where(have, sw, F(1))
        nh = np.where(have, np.minimum(sn / safe, maxh), F(0))
        nh = np.where(nh > 0, nh, F(0))
        use = nh > 0
        h = np.stack([np.where(use, sd[k] / safe * a[..., k], F(0)) for k in range(3)], -1)
        V = np.where(hit, F(-1), F(0))
        if variant == 2:
            V = q.copy()
        if variant >= 1 and has_v:
            precise = (pw > 0) if variant == 2 else np.zeros((H, W), bool)
            psafe = np.where(precise, pw, F(1))
            mu = np.where(precise, lum(pd[0] / psafe, pd[1] / psafe, pd[2] / psafe), lum(sd[0] / safe, sd[1] / safe, sd[2] / safe))
            lc = lum(c[..., 0] / a[..., 0], c[..., 1] / a[..., 1], c[..., 2] / a[..., 2])
            d, tot = lc - mu, nh + spp32
            e = d * d * nh * spp32 / tot
            if variant == 2:
                B = F(batches)
                Vn = (nh * np.where(precise, pv / psafe, sV / safe) + spp32 * (((B - F(1)) * q + e) / B)) / tot
            else:
                Vn = (nh * (sV / safe) + spp32 * e) / tot
            V = np.where(use, Vn, V)
        tot = spp32 + nh
        mix = np.where(use[..., None], (spp32 * c + nh[..., None] * h) / tot[..., None], c)
        n = np.where(use, tot, spp32)
        D = np.where(hit[..., None], mix / a, mix)
        if variant == 0:
            V = np.zeros((H, W), F)
    return dict(h=h, nh=nh, mix=mix, n=n, D=D, V=V.astype(F))
