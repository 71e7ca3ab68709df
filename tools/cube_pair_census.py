#!/usr/bin/env python3
"""CPU only: what the cube pairs of tileIntersect (primKey, pt_device.h) look like.  The oracle traces BASELINE config 4
(scenes/cornellObj.txt, depth 8, AA on, sort on) at 480x270 for two iterations; of the rays entering each bounce the script counts, per
cube, those that reach its inflated world box (make_world_aabb's rule: 1e-3 + 1e-4 |coordinate| around the transformed unit cube) -- the
candidates the pair phase runs primKey on -- and those of them the exact test accepts.  Binary64 slab tests for the boxes: this is a
census, not the device's arithmetic.  Printed per bounce: candidates per ray, the share of candidates that hit (primKey's hit path --
getPointOnRay, the product with the transform, the length -- runs with that share of a cube block's lanes), the share of rays with more
than one cube candidate.

    python tools/cube_pair_census.py [--scene scenes/cornellObj.txt] [--res 480 270] [--iters 2]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mygpuraytracer_amd as pt  # noqa: E402
from cpulibs import OracleLib  # noqa: E402
from objbox_cull_count import reach  # noqa: E402

G_CUBE = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "cornellObj.txt"))
    ap.add_argument("--res", type=int, nargs=2, default=(480, 270))
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--iters", type=int, default=2)
    a = ap.parse_args()
    s = pt.Scene(a.scene, res=tuple(a.res), depth=a.depth)
    s.apply_runcuda_camera()
    d = s.dump()
    O = OracleLib()
    O.set_libm(1)
    O.create(d, d["textures"])
    O.pt_init()
    cubes = [g for g in range(len(d["geom_ints"])) if d["geom_ints"][g][0] == G_CUBE]
    corners = np.array([[x, y, z] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)])
    boxes = {}
    for g in cubes:
        xf = d["geom_mats"][g][0:16].astype(np.float64).reshape(4, 4).T            # column-major mat4
        w = corners @ xf[:3, :3].T + xf[:3, 3]
        lo, hi = w.min(0), w.max(0)
        m = 1e-3 + 1e-4 * np.maximum(np.abs(lo), np.abs(hi))
        boxes[g] = (lo - m, hi + m)
    nb = a.depth
    rays = np.zeros(nb, np.int64); cand = np.zeros(nb, np.int64); hits = np.zeros(nb, np.int64); multi = np.zeros(nb, np.int64)
    for it in range(1, a.iters + 1):
        O.pt_generate(it)
        for b in range(nb):
            n = O.num_paths()
            if n == 0:
                break
            p = O.paths()[:n]
            o = p["origin"].astype(np.float64); dr = p["direction"].astype(np.float64)
            r6 = np.concatenate([p["origin"], p["direction"]], 1)
            per_ray = np.zeros(n, np.int64)
            for g in cubes:
                inw = reach(boxes[g][0], boxes[g][1], o, dr)
                hit = O.geom_test(g, r6)[:, 0] > 0
                assert not np.any(hit & ~inw), "a hit outside a box: the census itself is wrong"
                per_ray += inw
                cand[b] += int(inw.sum()); hits[b] += int(hit.sum())
            rays[b] += n; multi[b] += int((per_ray > 1).sum())
            O.pt_bounce(it)
        O.pt_final_gather()
    print("scene %s %dx%d depth %d, %d iterations (oracle, own libm), %d cubes" % (os.path.basename(a.scene), a.res[0], a.res[1], a.depth, a.iters, len(cubes)))
    print("bounce        rays  cube candidates  per ray   hit  share that hit  rays with > 1 candidate")
    for b in range(nb):
        if rays[b]:
            print("%6d %11d %16d  %7.3f %9d  %12.1f%%  %22.1f%%" % (b, rays[b], cand[b], cand[b] / rays[b], hits[b], 100.0 * hits[b] / max(cand[b], 1),
                                                                  100.0 * multi[b] / rays[b]))
    O.set_libm(0)


if __name__ == "__main__":
    main()
