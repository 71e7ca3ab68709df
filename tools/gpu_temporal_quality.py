"""How the temporal reuse's defaults were chosen: cornell.txt and cornellObj.txt at 256x256, depth 8, 8 frames of 2 spp
along a small orbit (left drag 2, 0.5 px per frame, a new accumulation per frame as the reference's loop), against a 1024-spp ground
truth at the final camera.  MSE over hit pixels of the last frame's mix / the current frame alone, and of the temporal denoised frame /
the spatial-only denoised one (ptx_denoise), over a grid of max_history x normal_cos x plane_tolerance.  One JSON line per setting, then
the best settings by the larger of the two scenes' denoised ratios.
    python tools/gpu_temporal_quality.py"""
import ctypes
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

MAX_HISTORY = (4, 8, 16, 32)
NORMAL_COS = (0.8, 0.9, 0.97)
PLANE_TOL = (0.003, 0.01, 0.03)
W = H = 256
FRAMES, SPP = 8, 2


def run(T, s, base, tparams):
    """the orbit sequence from the start camera `base` (bytes of a ptx_camera); returns mix, temporal denoised, current frame, spatial
    denoised and n_h of the last frame"""
    ctypes.memmove(ctypes.addressof(s.camera), base, len(base))
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))
    with pt.Temporal(0, W, H) as tm:
        for f in range(FRAMES):
            if f:
                s.orbit_events(o, [("left", 2.0, 0.5)])
            T.set_camera(s)
            T.reset_image()
            T.render(1, SPP)
            den = T.denoise_temporal(tm, SPP, **tparams).astype(np.float64)
        r = tm.read()
    cur = (T.read_image().reshape(H, W, 3) / np.float32(SPP)).astype(np.float64)
    return r["mix"].astype(np.float64), den, cur, T.denoise(SPP).astype(np.float64), r["count"]


def main():
    results = {}
    for scene in ("cornell.txt", "cornellObj.txt"):
        s = pt.Scene(os.path.join(ROOT, "scenes", scene), res=(W, H), depth=8)
        base = bytes(s.camera)
        with pt.Tracer(s) as T:
            run(T, s, base, dict(max_history=0))              # leaves the final camera set
            hit = T.gbuffer()["hit"]
            T.reset_image()
            T.render(1, 1024)
            gt = (T.read_image().reshape(H, W, 3) / np.float32(1024)).astype(np.float64)
            mse = lambda a: float(((a - gt)[hit] ** 2).mean())
            for mh, nc, tol in itertools.product(MAX_HISTORY, NORMAL_COS, PLANE_TOL):
                prm = dict(max_history=mh, normal_cos=nc, plane_tolerance=tol)
                m, den, cur, sden, cnt = run(T, s, base, prm)
                row = dict(scene=scene, **prm, mix_ratio=round(mse(m) / mse(cur), 4), denoised_ratio=round(mse(den) / mse(sden), 4),
                           inherit_fraction=round(float((cnt[hit] > 0).mean()), 4))
                results[(scene, mh, nc, tol)] = row
                print(json.dumps(row), flush=True)
    best = sorted(((max(results[(sc, *k)]["denoised_ratio"] for sc in ("cornell.txt", "cornellObj.txt")), k)
                   for k in itertools.product(MAX_HISTORY, NORMAL_COS, PLANE_TOL)))
    for worst_ratio, (mh, nc, tol) in best[:8]:
        print(json.dumps(dict(best_max_history=mh, normal_cos=nc, plane_tolerance=tol, worst_denoised_ratio=worst_ratio)))


if __name__ == "__main__":
    main()
