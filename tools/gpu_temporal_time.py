"""Device time of the temporal reuse (ptx_denoise_temporal) at 1920x1080 and 3840x2160 on cornellObj.txt, 4 spp, after one orbit step
(so that most pixels reproject): hipEvents on the tracer's stream around back-to-back calls with the camera unchanged (reprojection +
filter, G-buffer current) and around back-to-back ptx_denoise calls (the filter alone); the reprojection kernel's time is their
difference.  Bytes model of k_temporal_reproject per pixel: the current G-buffer record it reads (normal / hit 16 B, position 16 B,
albedo 16 B, ids 8 B), the frame (12 B), the new state (56 B), the mix (12 B) and (h, n_h) (16 B) it writes, and one 56-B previous
state record (the other bilinear taps come from the caches).  Fraction = model bytes / 8 TB/s over the measured time.
    python tools/gpu_temporal_time.py [--reps N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

HBM_PEAK = 8.0e12
BYTES_PER_PIXEL = 16 + 16 + 16 + 8 + 12 + 56 + 12 + 16 + 56


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    rows = []
    for W, H in ((1920, 1080), (3840, 2160)):
        s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"), res=(W, H), depth=8)
        s.apply_runcuda_camera()
        with pt.Tracer(s) as T, pt.Temporal(0, W, H) as tm:
            T.render(1, 4)
            T.denoise_temporal(tm, 4, read=False)
            o = s.orbit_init()
            s.orbit_events(o, [("left", 4.0, 0.0)])
            T.set_camera(s)
            T.reset_image()
            T.render(1, 4)
            T.denoise_temporal(tm, 4, read=False)    # warm-up: G-buffer of the new view, code objects
            T.denoise(4, read=False)
            T.synchronize()
            inherit = float((tm.read()["count"] > 0).mean())
            st = torch.cuda.ExternalStream(T.stream_ptr())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed(fn):
                e0.record(st)
                for _ in range(args.reps):
                    fn()
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1) / args.reps

            both, filt = [], []
            for _ in range(3):                       # alternated
                both.append(timed(lambda: T.denoise_temporal(tm, 4, read=False)))
                filt.append(timed(lambda: T.denoise(4, read=False)))
            both_ms, filt_ms = sorted(both)[1], sorted(filt)[1]
            rep_ms = both_ms - filt_ms
            b = BYTES_PER_PIXEL * W * H
            rows.append(dict(res="%dx%d" % (W, H), reproject_plus_filter_ms=round(both_ms, 4), filter_ms=round(filt_ms, 4),
                             reproject_ms=round(rep_ms, 4), inherit_fraction=round(inherit, 3), model_bytes=b,
                             model_ms_at_8TBs=round(b / HBM_PEAK * 1e3, 4),
                             bytes_model_fraction=round(b / HBM_PEAK * 1e3 / rep_ms, 3) if rep_ms > 0 else None))
            print(json.dumps(rows[-1]), flush=True)
    return rows


if __name__ == "__main__":
    main()
