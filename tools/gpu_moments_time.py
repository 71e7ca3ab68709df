"""Device time of the batch-means moments at 1920x1080 and 3840x2160 on cornellObj.txt: ptx_moments_add, ptx_moments_summarize, and
ptx_denoise_measured beside ptx_denoise_variance without a handle.  The enqueueing calls are timed with hipEvents on the tracer's
stream around back-to-back calls, alternated, median of three, as tools/gpu_variance_time.py does; ptx_moments_summarize waits for its
result, so it is timed on the host clock around the call (two launches, a 48-byte copy back and the synchronisation).
Bytes model per pixel beside each, at 8 TB/s:
  the add: 12 B read from the frame, 56 B read and 56 B written of state: 124 B
  the summary: 56 B read of state (the partials are 48 B per 256 pixels)
  the measured filter: prep 12 + 16 + 16 B read of frame and guides + 56 B of state, 16 B written = 116 B, then
    tools/gpu_variance_time.py's passes (5 x 64 B + 8 B); the spatial estimate only where a pixel has too few batches (nowhere here)
    python tools/gpu_moments_time.py [--reps N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

HBM_PEAK = 8.0e12
PASSES = 5
ADD = 124
SUMMARY = 56
FILTER_MEASURED = 116 + PASSES * 64 + 8
FILTER_SPATIAL = 60 + PASSES * 64 + 8          # + the spatial estimate on every hit pixel
SPATIAL = 52 * 700 / 256 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    for W, H in ((1920, 1080), (3840, 2160)):
        s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"), res=(W, H), depth=8)
        s.apply_runcuda_camera()
        with pt.Tracer(s) as T, pt.Moments(0, W, H) as m:
            n_spp = 0
            for _ in range(4):                           # four batches of one iteration: every pixel has min_batches
                T.render(n_spp + 1, 1)
                n_spp += 1
                m.add(T, n_spp)
            T.denoise_measured(m, n_spp, read=False)     # warm-up: G-buffer, code objects
            T.denoise_variance(n_spp, read=False)
            m.summary()
            T.synchronize()
            hit = float(T.gbuffer()["hit"].mean())
            st = torch.cuda.ExternalStream(T.stream_ptr())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            total = [n_spp]

            def timed(fn):
                e0.record(st)
                for _ in range(args.reps):
                    fn()
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1) / args.reps

            def add():                                   # (the frame does not change: the batches are zeros, the traffic is the same)
                total[0] += 1
                m.add(T, total[0])

            def summary():
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    m.summary()
                return (time.perf_counter() - t0) / args.reps * 1e3

            calls = dict(add=lambda: timed(add), measured=lambda: timed(lambda: T.denoise_measured(m, n_spp, read=False)),
                         variance_no_handle=lambda: timed(lambda: T.denoise_variance(n_spp, read=False)), summary_host_clock=summary)
            ms = {k: [] for k in calls}
            for _ in range(3):                           # alternated
                for k, fn in calls.items():
                    ms[k].append(fn())
            med = {k: sorted(v)[1] for k, v in ms.items()}
            n = W * H
            model = dict(add=ADD, measured=FILTER_MEASURED, variance_no_handle=FILTER_SPATIAL + SPATIAL * hit, summary_host_clock=SUMMARY)
            row = dict(res="%dx%d" % (W, H), hit_fraction=round(hit, 3))
            for k in calls:
                row[k + "_ms"] = round(med[k], 4)
                row[k + "_model_ms_at_8TBs"] = round(model[k] * n / HBM_PEAK * 1e3, 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
