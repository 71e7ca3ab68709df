"""Device time of ptx_denoise_temporal_measured beside ptx_denoise_variance with a handle, at 1920x1080 and 3840x2160 on
cornellObj.txt, on the same frames: view 1 through both (each on a handle of its own), a camera step, 4 batches of one iteration, then
both calls again and again on view 2 (the same segment, recomputed from the same history, so every call does the same work).  Timed
with hipEvents on the tracer's stream around back-to-back calls, alternated, median of three, as tools/gpu_moments_time.py does.
Bytes model per pixel beside each, at 8 TB/s:
  the reprojection: 56 B of G-buffer + 12 B of frame read, one history record (56 B) through the taps, 56 B of state + 12 B of mix +
    16 B of (h, n_h) written: 208 B; k_reproject_measured reads 16 B of ma and 8 B of mb on top: + 24 B
  the prep from the state: 48 B read, 16 B written; then tools/gpu_variance_time.py's passes (5 x 64 B + 8 B)
  ptx_denoise_variance also launches the spatial estimate, which leaves after one 4-byte load per pixel where every pixel of a tile
    inherits a V, and does its windowed sums where one does not; the new call does not launch it (no pixel is left without a V)
    python tools/gpu_temporal_measured_time.py [--reps N]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

HBM_PEAK = 8.0e12
PASSES = 5
REPROJECT = 208
FILTER = 64 + PASSES * 64 + 8
MODEL = dict(variance_handle=REPROJECT + 4 + FILTER, temporal_measured=REPROJECT + 24 + FILTER)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    for W, H in ((1920, 1080), (3840, 2160)):
        s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"), res=(W, H), depth=8)
        o = s.orbit_init()
        s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))
        with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Temporal(0, W, H) as tn, pt.Temporal(0, W, H) as tv:
            n_spp = 4

            def view():
                m.reset()
                for it in range(1, n_spp + 1):           # four batches of one iteration: min_batches
                    T.render(it, 1)
                    m.add(T, it)
                T.denoise_measured(m, n_spp, temporal=tn, read=False)
                T.denoise_variance(n_spp, tv, read=False)

            view()
            s.orbit_events(o, [("left", 8.0, 1.0)])
            T.set_camera(s)
            T.reset_image()
            view()                                       # (also the warm-up: G-buffer, code objects)
            T.synchronize()
            inherit = float((tn.read()["count"] > 0).mean())
            st = torch.cuda.ExternalStream(T.stream_ptr())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed(fn):
                e0.record(st)
                for _ in range(args.reps):
                    fn()
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1) / args.reps

            calls = dict(temporal_measured=lambda: T.denoise_measured(m, n_spp, temporal=tn, read=False),
                         variance_handle=lambda: T.denoise_variance(n_spp, tv, read=False))
            ms = {k: [] for k in calls}
            for _ in range(3):                           # alternated
                for k, fn in calls.items():
                    ms[k].append(timed(fn))
            med = {k: sorted(v)[1] for k, v in ms.items()}
            n = W * H
            row = dict(res="%dx%d" % (W, H), inheriting_fraction=round(inherit, 3))
            for k in calls:
                row[k + "_ms"] = round(med[k], 4)
                row[k + "_model_ms_at_8TBs"] = round(MODEL[k] * n / HBM_PEAK * 1e3, 4)
            row["measured_over_variance"] = round(med["temporal_measured"] / med["variance_handle"], 4)
            row["extra_24B_model_ms_at_8TBs"] = round(24 * n / HBM_PEAK * 1e3, 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
