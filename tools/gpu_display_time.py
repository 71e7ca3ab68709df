"""Device time of the display transform (ptx_display_tracer) next to the preview it stands beside (ptx_write_pbo_device) at 1920x1080 and
3840x2160 on cornellObj.txt, 4 spp: hipEvents on the tracer's stream around back-to-back calls of
    (a) ptx_write_pbo_device, the reference's rule (k_pbo),
    (b) the display call with a manual exposure (k_display_map alone),
    (c) the display call with the block meter (k_display_blocks + k_display_meter + k_display_map),
    (d) the same with keep_float,
alternated within one run: every round times `inner` calls of each in turn, the figure is the median over the rounds.  The bytes model
is what the stage has to move at least: the meter reads the frame (12 B per pixel), the map reads it again (12 B) and writes the codes
(4 B), plus the float frame (12 B) with keep_float.  Share = model bytes / 8 TB/s over the measured time.
    python tools/gpu_display_time.py [--rounds N] [--inner M] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

HBM_PEAK = 8.0e12
MODEL = dict(pbo=12 + 4, manual=12 + 4, blocks=12 + 12 + 4, keep_float=12 + 12 + 4 + 12)       # bytes per pixel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)      # rounds * inner = 200 calls of each by default
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    rows = []
    for W, H in ((1920, 1080), (3840, 2160)):
        s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"), res=(W, H), depth=8)
        s.apply_runcuda_camera()
        with pt.Tracer(s) as T, pt.Display(W, H) as D:
            T.render(1, 4)
            T.synchronize()
            st = torch.cuda.ExternalStream(T.stream_ptr())
            pbo = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
            calls = dict(pbo=lambda: pt.api._check(T.lib.ptx_write_pbo_device(T.h, 4, pbo.data_ptr()), "ptx_write_pbo_device"),
                         manual=lambda: D.tracer(T, 4, pbo=pbo.data_ptr(), meter="manual", exposure=2.0),
                         blocks=lambda: D.tracer(T, 4, pbo=pbo.data_ptr()),
                         keep_float=lambda: D.tracer(T, 4, pbo=pbo.data_ptr(), keep_float=1))
            for f in calls.values():                     # warm-up: code objects, the float frame
                for _ in range(3):
                    f()
            T.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = {k: [] for k in calls}
            for _ in range(args.rounds):
                for k, f in calls.items():
                    e0.record(st)
                    for _ in range(args.inner):
                        f()
                    e1.record(st)
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1) / args.inner)
            status = D.status()
            row = dict(res="%dx%d" % (W, H), calls_each=args.rounds * args.inner, metered=round(status["metered"], 4),
                       blocks=status["blocks_total"])
            for k in calls:
                med = float(np.median(ms[k]))
                b = MODEL[k] * W * H
                row[k + "_us"] = round(med * 1e3, 2)
                row[k + "_min_us"] = round(float(np.min(ms[k])) * 1e3, 2)
                row[k + "_model_us_at_8TBs"] = round(b / HBM_PEAK * 1e6, 2)
                row[k + "_bytes_model_share"] = round(b / HBM_PEAK * 1e3 / med, 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    return rows


if __name__ == "__main__":
    main()
