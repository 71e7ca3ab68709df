"""Device time of the a-trous denoiser (ptx_denoise) at 1920x1080 and 3840x2160 on cornellObj.txt, 4 spp: hipEvents on the tracer's
stream around back-to-back denoise calls (the filter alone, G-buffer current), and around the first denoise after a camera change
(G-buffer + filter).  The bytes model is what the filter has to move at least: k_atrous_prep reads the frame (12 B), the normal / hit
record (16 B) and the albedo (16 B) and writes the colour (16 B) per pixel; every pass reads the pixel's own normal, position and colour
records (48 B) and writes its colour (16 B; the last pass writes 12 B and reads the albedo, 16 B) -- the 24 other taps come from the
caches.  Fraction = model bytes / 8 TB/s over the measured time.
    python tools/gpu_denoise_time.py [--reps N]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

HBM_PEAK = 8.0e12


def model_bytes(n, passes):
    return n * (12 + 16 + 16 + 16 + (passes - 1) * 64 + (48 + 16 + 12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    rows = []
    for W, H in ((1920, 1080), (3840, 2160)):
        s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"), res=(W, H), depth=8)
        s.apply_runcuda_camera()
        with pt.Tracer(s) as T:
            T.render(1, 4)
            T.synchronize()
            st = torch.cuda.ExternalStream(T.stream_ptr())
            T.denoise(4, read=False)                 # warm-up: code objects, buffers, G-buffer
            T.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(args.reps):
                T.denoise(4, read=False)
            e1.record(st)
            e1.synchronize()
            ms = e0.elapsed_time(e1) / args.reps
            # the first denoise after a camera change: G-buffer + filter (two cameras in turn, each set_camera is a real change)
            o = s.orbit_init()
            first = []
            for k in range(6):
                s.orbit_events(o, [("left", 3.0 if k % 2 == 0 else -3.0, 0.0)])
                T.set_camera(s)
                e0.record(st)
                T.denoise(4, read=False)
                e1.record(st)
                e1.synchronize()
                first.append(e0.elapsed_time(e1))
            passes = pt.default_denoise_params().passes
            b = model_bytes(W * H, passes)
            rows.append(dict(res="%dx%d" % (W, H), passes=passes, filter_ms=round(ms, 4), gbuffer_plus_filter_ms=round(float(np.median(first)), 4),
                             model_bytes=b, model_ms_at_8TBs=round(b / HBM_PEAK * 1e3, 4), bytes_model_fraction=round(b / HBM_PEAK * 1e3 / ms, 3)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


if __name__ == "__main__":
    main()
