"""How the denoiser's defaults were chosen: cornell.txt and cornellObj.txt at 256x256, depth 8, a 4-spp frame against
a 1024-spp ground truth; MSE over hit pixels of the denoised frame / MSE of the noisy one, over a grid of phi_color x phi_normal x
phi_position (5 passes, demodulated).  Prints one JSON line per setting and the best settings by the larger of the two ratios.
    python tools/gpu_denoise_quality.py"""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

PHI_C = (0.25, 1.0, 4.0, 16.0, 64.0)
PHI_N = (0.01, 0.1, 1.0)
PHI_X = (0.05, 0.5, 5.0)


def main():
    tracers, frames = [], []
    for name in ("cornell.txt", "cornellObj.txt"):
        s = pt.Scene(os.path.join(ROOT, "scenes", name), res=(256, 256), depth=8)
        s.apply_runcuda_camera()
        T = pt.Tracer(s)
        T.render(1, 4)
        noisy = (T.read_image() / np.float32(4)).reshape(256, 256, 3).astype(np.float64)
        hit = T.gbuffer()["hit"]
        G = pt.Tracer(s)                              # the ground truth from its own tracer: independent of the 4 samples
        G.render(1001, 1024)
        gt = (G.read_image() / np.float32(1024)).reshape(256, 256, 3).astype(np.float64)
        G.close()
        tracers.append(T)
        frames.append((name, noisy, gt, hit))
    results = []
    for pc, pn, px in itertools.product(PHI_C, PHI_N, PHI_X):
        ratios = []
        for T, (name, noisy, gt, hit) in zip(tracers, frames):
            den = T.denoise(4, phi_color=pc, phi_normal=pn, phi_position=px).astype(np.float64)
            ratios.append(float(((den - gt)[hit] ** 2).mean() / ((noisy - gt)[hit] ** 2).mean()))
        results.append(dict(phi_color=pc, phi_normal=pn, phi_position=px, ratio_cornell=round(ratios[0], 4), ratio_obj=round(ratios[1], 4)))
        print(json.dumps(results[-1]), flush=True)
    results.sort(key=lambda r: max(r["ratio_cornell"], r["ratio_obj"]))
    print("best:", json.dumps(results[:5]))
    p = pt.default_denoise_params()
    print("defaults:", json.dumps([r for r in results if (r["phi_color"], r["phi_normal"], r["phi_position"]) ==
                                   (p.phi_color, float(np.float32(p.phi_normal)), p.phi_position)]))
    for T in tracers:
        T.close()


if __name__ == "__main__":
    main()
