"""Device time of the variance-guided denoiser (ptx_denoise_variance) beside ptx_denoise_temporal and ptx_denoise at 1920x1080 and
3840x2160 on cornellObj.txt, 4 spp: hipEvents on the tracer's stream around back-to-back calls with the camera unchanged (G-buffer
current), alternated, median of three.  Two frames: after one orbit step, where most pixels have history (the spatial estimate leaves
at once in most workgroups), and a first frame (handle reset before every call) where every hit pixel takes the spatial estimate.
Bytes model per pixel beside each, at 8 TB/s:
  a pass of either filter: 48 B read (normal / hit, position, colour) + 16 B written (last pass: + 16 B albedo, 12 B written): 64 B
  the filter: prep (12 + 16 + 16 read, 16 written = 60 B; from the state 48 + 16 = 64 B) + passes x 64 B (+ 8 B of v0 and v out)
  the reprojection: tools/gpu_temporal_time.py's 208 B (V rides in the D record)
  the spatial estimate where it runs: 16 + 16 + 12 + 8 B read per tile pixel x 700 / 256 (tile + apron) + 4 B written = 146 B
    python tools/gpu_variance_time.py [--reps N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

HBM_PEAK = 8.0e12
PASSES = 5
FILTER_FIXED = 60 + PASSES * 64
FILTER_VAR = 64 + PASSES * 64 + 8
REPROJECT = 208
SPATIAL = 52 * 700 / 256 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    for W, H in ((1920, 1080), (3840, 2160)):
        s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"), res=(W, H), depth=8)
        s.apply_runcuda_camera()
        with pt.Tracer(s) as T, pt.Temporal(0, W, H) as tv, pt.Temporal(0, W, H) as tt, pt.Temporal(0, W, H) as t1:
            T.render(1, 4)
            T.denoise_variance(4, tv, read=False)
            T.denoise_temporal(tt, 4, read=False)
            o = s.orbit_init()
            s.orbit_events(o, [("left", 4.0, 0.0)])
            T.set_camera(s)
            T.reset_image()
            T.render(1, 4)
            T.denoise_variance(4, tv, read=False)        # warm-up: G-buffer of the new view, code objects
            T.denoise_temporal(tt, 4, read=False)
            T.denoise_variance(4, read=False)
            T.denoise(4, read=False)
            T.synchronize()
            inherit = float((tv.read()["count"] > 0).mean())
            hit = float(T.gbuffer()["hit"].mean())
            st = torch.cuda.ExternalStream(T.stream_ptr())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed(fn):
                e0.record(st)
                for _ in range(args.reps):
                    fn()
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1) / args.reps

            def first_frame():
                t1.reset()
                T.denoise_variance(4, t1, read=False)

            calls = dict(variance_with_history=lambda: T.denoise_variance(4, tv, read=False),
                         temporal=lambda: T.denoise_temporal(tt, 4, read=False),
                         variance_first_frame=first_frame,
                         variance_no_handle=lambda: T.denoise_variance(4, read=False),
                         denoise=lambda: T.denoise(4, read=False))
            ms = {k: [] for k in calls}
            for _ in range(3):                           # alternated
                for k, fn in calls.items():
                    ms[k].append(timed(fn))
            med = {k: sorted(v)[1] for k, v in ms.items()}
            n = W * H
            model = dict(variance_with_history=REPROJECT + FILTER_VAR + SPATIAL * (hit - inherit), temporal=REPROJECT + FILTER_FIXED,
                         variance_first_frame=REPROJECT + FILTER_VAR + SPATIAL * hit, variance_no_handle=FILTER_VAR - 4 + SPATIAL * hit,
                         denoise=FILTER_FIXED)
            row = dict(res="%dx%d" % (W, H), hit_fraction=round(hit, 3), inherit_fraction=round(inherit, 3))
            for k in calls:
                row[k + "_ms"] = round(med[k], 4)
                row[k + "_model_ms_at_8TBs"] = round(model[k] * n / HBM_PEAK * 1e3, 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
