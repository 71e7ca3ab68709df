"""Device time of ptx_denoise_adaptive at 1920x1080 and 3840x2160 on cornellObj.txt (C4), after an adaptive run that left the tiles with
different counts.  The yardstick is the closest sequence there was before the call existed: ptx_adaptive_resolve followed by
ptx_denoise_measured on a uniform (not tiled) moments handle of the same size.  Both are enqueueing calls, timed with hipEvents on the
tracer's stream around back-to-back calls, alternated, three runs each: the median and the spread (max - min) of the three are printed.
Bytes model per pixel beside each, at 8 TB/s:
  k_adaptive_prep: 12 + 16 + 16 B read of frame and guides + 40 B of state (mean, ma, the pixel's half of mb) + 4 B per 256 pixels of
    counts, 16 + 12 B written = 112 B; then tools/gpu_variance_time.py's passes (5 x 64 B + 8 B)
  the yardstick: the resolve 12 B read + 12 B written, then tools/gpu_moments_time.py's measured filter (116 B + the passes)
--yardstick-only: only the second, for a build that has no ptx_denoise_adaptive.
    python tools/gpu_adaptive_denoise_time.py [--reps N] [--yardstick-only]      (the lines go to profiles/adaptive_denoise_time.txt)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

HBM_PEAK = 8.0e12
PASSES = 5 * 64 + 8
ADAPTIVE = 112 + PASSES
YARDSTICK = 24 + 116 + PASSES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--yardstick-only", action="store_true")
    args = ap.parse_args()
    import torch
    for W, H in ((1920, 1080), (3840, 2160)):
        s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"), res=(W, H), depth=8)
        s.apply_runcuda_camera()
        with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Moments(0, W, H) as mu, pt.Adaptive(0, W, H) as a:
            rounds = a.render(T, m, batch=4, max_iterations=24, target=0.2)
            last = rounds[-1]
            for n in range(1, 5):                        # the uniform handle: four batches (the buffer does not move: the traffic is the same)
                mu.add(T, n)
            spp = int(last["samples_max"])
            calls = dict(yardstick=lambda: (a.resolve(T), T.denoise_measured(mu, spp, read=False)))
            if not args.yardstick_only:
                calls["adaptive"] = lambda: T.denoise_adaptive(a, m, read=False)
            for fn in calls.values():                    # warm-up: G-buffer, code objects
                fn()
            T.synchronize()
            st = torch.cuda.ExternalStream(T.stream_ptr())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed(fn):
                e0.record(st)
                for _ in range(args.reps):
                    fn()
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1) / args.reps

            ms = {k: [] for k in calls}
            for _ in range(3):                           # alternated
                for k, fn in calls.items():
                    ms[k].append(timed(fn))
            model = dict(yardstick=YARDSTICK, adaptive=ADAPTIVE)
            row = dict(res="%dx%d" % (W, H), rounds=len(rounds), samples_min=int(last["samples_min"]), samples_max=spp,
                       tiles_active=int(last["tiles_active"]), tiles=int(last["tiles"]), reps=args.reps)
            for k, v in ms.items():
                row[k + "_ms"] = round(sorted(v)[1], 4)
                row[k + "_spread_ms"] = round(max(v) - min(v), 4)
                row[k + "_runs_ms"] = [round(x, 4) for x in v]
                row[k + "_model_ms_at_8TBs"] = round(model[k] * W * H / HBM_PEAK * 1e3, 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
