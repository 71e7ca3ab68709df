#!/usr/bin/env python3
"""CPU only: two counts on the oracle's own rays, taken before the light-only last bounce got its pool and the camera bounce its
wave-uniform shortcuts (profiles/last_pool_wave_uniform_ab.txt).  BASELINE config 4 (scenes/cornellObj.txt, depth 8, AA on, sort on) at
480x270, three iterations, in the manner of tools/objbox_cull_count.py: binary64 slab tests against the inflated world boxes
(make_world_aabb's rule, 1e-3 + 1e-4 |coordinate|) -- a census, not the device's arithmetic.

 (i)  last bounce (depth - 1): the share of its rays that reach the inflated box of an emitting geom, and how many do per tile of 256
      consecutive rays of the sorted stream (what one workgroup's tile holds).
 (ii) camera bounce: of the waves -- 64 consecutive pixels -- those whose rays all have the same candidate mask (and how many candidates),
      and those whose rays all fall into one material bin and are all stored (hit, not a light, not the last bounce).

    python tools/last_pool_census.py [--scene scenes/cornellObj.txt] [--res 480 270] [--iters 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mygpuraytracer_amd as pt  # noqa: E402
from cpulibs import OracleLib  # noqa: E402
from objbox_cull_count import reach  # noqa: E402

G_OBJ = 3


def world_boxes(d):
    """inflated world box per geom: the transformed corners of the unit cube (cubes exactly, spheres conservatively) or the mesh's vertices"""
    out = []
    corners = np.array([[x, y, z] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)], np.float64)
    for g in range(len(d["geom_ints"])):
        xf = d["geom_mats"][g][0:16].astype(np.float64).reshape(4, 4).T
        v = d["faces"][g].astype(np.float64).reshape(-1, 3, 5)[:, :, :3].reshape(-1, 3) if d["geom_ints"][g][0] == G_OBJ else corners
        w = v @ xf[:3, :3].T + xf[:3, 3]
        lo, hi = w.min(0), w.max(0)
        m = 1e-3 + 1e-4 * np.maximum(np.abs(lo), np.abs(hi))
        out.append((lo - m, hi + m))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "cornellObj.txt"))
    ap.add_argument("--res", type=int, nargs=2, default=(480, 270))
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    s = pt.Scene(a.scene, res=tuple(a.res), depth=a.depth)
    s.apply_runcuda_camera()
    d = s.dump()
    O = OracleLib()
    O.set_libm(1)
    O.create(d, d["textures"])
    O.pt_init()
    boxes = world_boxes(d)
    mats = d["materials"]
    emit = [g for g in range(len(boxes)) if mats[d["geom_ints"][g][1], 10] > 0]
    last = a.depth - 1
    n_last = n_reach = 0
    per_tile = []
    waves = uni_mask = uni_bin = uni_both = 0
    cand_hist = np.zeros(33, np.int64)
    for it in range(1, a.iters + 1):
        O.pt_generate(it)
        for b in range(a.depth):
            n = O.num_paths()
            if n == 0:
                break
            p = O.paths()[:n].copy()
            o = p["origin"].astype(np.float64); dr = p["direction"].astype(np.float64)
            if b == 0:
                mask = np.zeros(n, np.int64)
                for g, (lo, hi) in enumerate(boxes):
                    mask |= reach(lo, hi, o, dr).astype(np.int64) << g
                isec = O.compute_intersections(p)
                stored = (isec["t"] > 0) & (mats[isec["materialId"], 10] <= 0) & (a.depth > 1)
                mat = np.where(isec["t"] > 0, isec["materialId"], 0)
                for w0 in range(0, n - 63, 64):           # (the device's waves: 64 consecutive pixel slots; a partial last one never qualifies)
                    mk, mt, stv = mask[w0:w0 + 64], mat[w0:w0 + 64], stored[w0:w0 + 64]
                    um = bool(np.all(mk == mk[0])) and bin(int(mk[0])).count("1") <= 4
                    ub = bool(np.all(mt == mt[0])) and bool(np.all(stv))
                    if mk.any():                          # (a wave that reaches no box at all does no bookkeeping to speak of)
                        waves += 1; uni_mask += um; uni_bin += ub; uni_both += um and ub
                        if np.all(mk == mk[0]):
                            cand_hist[bin(int(mk[0])).count("1")] += 1
            if b == last:
                r = np.zeros(n, bool)
                for g in emit:
                    r |= reach(boxes[g][0], boxes[g][1], o, dr)
                n_last += n; n_reach += int(r.sum())
                per_tile += [int(r[k:k + 256].sum()) for k in range(0, n, 256)]
            O.pt_bounce(it)
        O.pt_final_gather()
    O.set_libm(0)
    pt_ = np.array(per_tile)
    print("scene %s %dx%d depth %d, %d iterations (oracle, own libm); emitting geoms %s" % (os.path.basename(a.scene), a.res[0], a.res[1], a.depth, a.iters, emit))
    print("(i)  bounce %d: %d rays, %d reach an emitter's inflated box (%.2f %%); per tile of 256: mean %.1f, median %d, max %d, tiles %d, "
          "tiles with none %d" % (last, n_last, n_reach, 100.0 * n_reach / max(n_last, 1), pt_.mean(), int(np.median(pt_)), pt_.max(), len(pt_), int((pt_ == 0).sum())))
    print("     GO for the pool if the mean is below 64 per tile: %s" % ("GO" if pt_.mean() < 64 else "NO-GO"))
    print("(ii) camera bounce: %d waves of 64 pixels that reach some box; equal candidate masks (<= 4 candidates) %d (%.1f %%); one bin and all "
          "stored %d (%.1f %%); both %d (%.1f %%)" % (waves, uni_mask, 100.0 * uni_mask / max(waves, 1), uni_bin, 100.0 * uni_bin / max(waves, 1),
                                                     uni_both, 100.0 * uni_both / max(waves, 1)))
    print("     candidates of the waves with equal masks: %s" % {k: int(v) for k, v in enumerate(cand_hist) if v})
    print("     GO for the shortcuts if at least a third of the non-empty waves qualify: slots %s, ranking %s" % (
        "GO" if 3 * uni_mask >= waves else "NO-GO", "GO" if 3 * uni_bin >= waves else "NO-GO"))


if __name__ == "__main__":
    main()
