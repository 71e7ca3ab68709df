#!/usr/bin/env python3
"""CPU only: how many of the small-mesh candidates that the world-box pre-test admits (cullMask, pt_device.h) would an object-space box
reject?  The oracle traces BASELINE config 4 (scenes/cornellObj.txt, depth 8, AA on, sort on) at 480x270 for three iterations; of the
rays entering each bounce the script counts those that reach the mesh's inflated world box (make_world_aabb's rule: 1e-3 + 1e-4
|coordinate|), those of them that reach the faces' object-space box (inflated by 1e-4 of its size here -- the count does not depend
on it), and those the mesh's exact test accepts at all.  Binary64 slab tests: this is a census, not the device's arithmetic.

    python tools/objbox_cull_count.py [--scene scenes/cornellObj.txt] [--res 480 270] [--iters 3]
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

MESH_CHUNK = 4
G_OBJ = 3


def reach(lo, hi, o, d):
    """rays o + t d, t >= 0, against the closed box [lo, hi] (binary64; a zero direction component = inside that slab or not)"""
    tn = np.zeros(len(o)); tf = np.full(len(o), np.inf); ok = np.ones(len(o), bool)
    for k in range(3):
        z = d[:, k] == 0
        with np.errstate(divide="ignore", invalid="ignore"):
            t0 = (lo[k] - o[:, k]) / d[:, k]; t1 = (hi[k] - o[:, k]) / d[:, k]
        a = np.minimum(t0, t1); b = np.maximum(t0, t1)
        ok &= np.where(z, (o[:, k] >= lo[k]) & (o[:, k] <= hi[k]), True)
        tn = np.where(z, tn, np.maximum(tn, a)); tf = np.where(z, tf, np.minimum(tf, b))
    return ok & (tn <= tf)


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
    meshes = [g for g in range(len(d["geom_ints"])) if d["geom_ints"][g][0] == G_OBJ]
    boxes = {}
    for g in meshes:
        xf = d["geom_mats"][g][0:16].astype(np.float64).reshape(4, 4).T            # column-major mat4
        inv = d["geom_mats"][g][16:32].astype(np.float64).reshape(4, 4).T
        v = d["faces"][g].astype(np.float64).reshape(-1, 3, 5)[:, :, :3].reshape(-1, 3)
        w = v @ xf[:3, :3].T + xf[:3, 3]
        wlo, whi = w.min(0), w.max(0)
        m = 1e-3 + 1e-4 * np.maximum(np.abs(wlo), np.abs(whi))
        olo, ohi = v.min(0), v.max(0)
        e = 1e-4 * (ohi - olo).max()
        boxes[g] = (wlo - m, whi + m, olo - e, ohi + e, inv, (len(d["faces"][g]) + MESH_CHUNK - 1) // MESH_CHUNK)
    nb = a.depth
    rays = np.zeros(nb, np.int64)
    world = {g: np.zeros(nb, np.int64) for g in meshes}; both = {g: np.zeros(nb, np.int64) for g in meshes}
    hits = {g: np.zeros(nb, np.int64) for g in meshes}
    for it in range(1, a.iters + 1):
        O.pt_generate(it)
        for b in range(nb):
            n = O.num_paths()
            if n == 0:
                break
            p = O.paths()[:n]
            o = p["origin"].astype(np.float64); dr = p["direction"].astype(np.float64)
            rays[b] += n
            r6 = np.concatenate([p["origin"], p["direction"]], 1)
            for g in meshes:
                wlo, whi, olo, ohi, inv, _ = boxes[g]
                inw = reach(wlo, whi, o, dr)
                oo = o @ inv[:3, :3].T + inv[:3, 3]; od = dr @ inv[:3, :3].T
                ino = reach(olo, ohi, oo, od)
                hit = O.geom_test(g, r6)[:, 0] > 0
                assert not np.any(hit & ~(inw & ino)), "a hit outside a box: the census itself is wrong"
                world[g][b] += int(inw.sum()); both[g][b] += int((inw & ino).sum()); hits[g][b] += int(hit.sum())
            O.pt_bounce(it)
        O.pt_final_gather()
    print("scene %s %dx%d depth %d, %d iterations (oracle, own libm)" % (os.path.basename(a.scene), a.res[0], a.res[1], a.depth, a.iters))
    for g in meshes:
        ch = boxes[g][5]
        print("geom %d: %d faces, %d chunk entries per candidate" % (g, len(d["faces"][g]), ch))
        print("bounce        rays  world-box  +object-box  reject   exact-hit  entries/256 rays: today  with object box")
        for b in range(nb):
            if rays[b]:
                print("%6d %11d %10d %12d  %5.1f%%  %10d  %23.1f  %15.1f" % (
                    b, rays[b], world[g][b], both[g][b], 100.0 * (1 - both[g][b] / max(world[g][b], 1)), hits[g][b],
                    256.0 * ch * world[g][b] / rays[b], 256.0 * ch * both[g][b] / rays[b]))
        for name, sl in (("bounces 0-%d" % (nb - 1), slice(0, nb)), ("bounces 1-%d" % (nb - 1), slice(1, nb))):
            R, Wd, B, H = rays[sl].sum(), world[g][sl].sum(), both[g][sl].sum(), hits[g][sl].sum()
            print("%s: rays %d, world-box %d (%.3f per ray), +object-box %d, REJECT SHARE %.1f%%, exact hits %d (%.1f%% of the world-box "
                  "candidates); entries per 256 rays %.1f -> %.1f" % (name, R, Wd, Wd / R, B, 100.0 * (1 - B / max(Wd, 1)), H,
                                                                     100.0 * H / max(Wd, 1), 256.0 * ch * Wd / R, 256.0 * ch * B / R))
    O.set_libm(0)


if __name__ == "__main__":
    main()
