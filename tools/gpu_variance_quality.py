"""How the variance guidance's phi_luminance was chosen: cornell.txt and cornellObj.txt at 256x256, depth 8.
Orbit: 8 frames of 2 spp along a small orbit (left drag 2, 0.5 px per frame, a new accumulation per frame as the reference's loop)
against a 1024-spp ground truth at the final camera: MSE over hit pixels of ptx_denoise_variance with the handle over phi_luminance x
max_history, beside ptx_denoise_temporal's (the fixed phi_color) at the same max_history.  Stopped camera: 1024 spp accumulated against
16384 spp: ptx_denoise_variance without a handle over phi_luminance, beside ptx_denoise's and the unfiltered frame's.  One JSON line per
setting.
    python tools/gpu_variance_quality.py"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

PHI = (1.0, 2.0, 4.0, 8.0, 16.0)
MAX_HISTORY = (4, 16)
W = H = 256
FRAMES, SPP = 8, 2


def orbit(scene):
    s = pt.Scene(os.path.join(ROOT, "scenes", scene), res=(W, H), depth=8)
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))
    settings = [(phi, mh) for phi in PHI for mh in MAX_HISTORY]
    with pt.Tracer(s) as T:
        tv = [pt.Temporal(0, W, H) for _ in settings]
        tt = [pt.Temporal(0, W, H) for _ in MAX_HISTORY]
        for f in range(FRAMES):
            if f:
                s.orbit_events(o, [("left", 2.0, 0.5)])
                T.set_camera(s)
                T.reset_image()
            T.render(1, SPP)
            vden = [T.denoise_variance(SPP, h, phi_luminance=phi, max_history=mh).astype(np.float64) for h, (phi, mh) in zip(tv, settings)]
            tden = [T.denoise_temporal(h, SPP, max_history=mh).astype(np.float64) for h, mh in zip(tt, MAX_HISTORY)]
        hit = T.gbuffer()["hit"]
        T.render(SPP + 1, 1024 - SPP)
        gt = (T.read_image().reshape(H, W, 3) / np.float32(1024)).astype(np.float64)
        for h in tv + tt:
            h.close()
    mse = lambda a: float(((a - gt)[hit] ** 2).mean())
    fixed = {mh: mse(d) for mh, d in zip(MAX_HISTORY, tden)}
    for (phi, mh), d in zip(settings, vden):
        print(json.dumps(dict(case="orbit", scene=scene, phi_luminance=phi, max_history=mh, mse_variance=round(mse(d), 6),
                              mse_fixed=round(fixed[mh], 6), ratio=round(mse(d) / fixed[mh], 3),
                              ratio_to_fixed_at_4=round(mse(d) / fixed[4], 3))), flush=True)


def stopped(scene):
    s = pt.Scene(os.path.join(ROOT, "scenes", scene), res=(W, H), depth=8)
    s.apply_runcuda_camera()
    with pt.Tracer(s) as T:
        T.render(1, 1024)
        cur = (T.read_image().reshape(H, W, 3) / np.float32(1024)).astype(np.float64)
        vden = [T.denoise_variance(1024, phi_luminance=phi).astype(np.float64) for phi in PHI]
        sden = T.denoise(1024).astype(np.float64)
        hit = T.gbuffer()["hit"]
        T.render(1025, 16384 - 1024)
        gt = (T.read_image().reshape(H, W, 3) / np.float32(16384)).astype(np.float64)
    mse = lambda a: float(((a - gt)[hit] ** 2).mean())
    for phi, d in zip(PHI, vden):
        print(json.dumps(dict(case="stopped", scene=scene, phi_luminance=phi, mse_variance=round(mse(d), 7), mse_fixed=round(mse(sden), 7),
                              mse_unfiltered=round(mse(cur), 7), ratio=round(mse(d) / mse(sden), 3),
                              ratio_to_unfiltered=round(mse(d) / mse(cur), 3))), flush=True)


if __name__ == "__main__":
    for scene in ("cornell.txt", "cornellObj.txt"):
        orbit(scene)
        stopped(scene)
