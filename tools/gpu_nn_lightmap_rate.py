"""Device time of the lightmap filter (ptx_nn_denoise_lightmap_device) beside the image entry point on the same 3-input network
(ptx_nn_denoise_images_device, hdr and the normal role), and what a progress monitor costs, at 1920x1080 and 3840x2160, by
tools/gpu_nn_image_rate.py's method: hipEvents on one stream around `inner` back-to-back calls, the calls alternated within a round,
the figure the median over the rounds (minimum and maximum next to it).  Synthetic weights on the standard channel table.
    images_hdr_ms     the image call, hdr, input_scale given: the yardstick for the HDR lightmap (the PU curve in place of the Log one)
    lightmap_hdr_ms   the lightmap call, input_scale given
    images_normal_ms  the image call, normal role: the directional lightmap's arithmetic
    lightmap_dir_ms   the lightmap call, directional
    monitor_ms        lightmap_hdr with a monitor that returns at once: every stage waited for on the host (18 reports per tile + 1)
    python tools/gpu_nn_lightmap_rate.py [--rounds N] [--inner M] [--sizes WxH,..] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mygpuraytracer_amd as pt  # noqa: E402
import unet_ref as U  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pt.load_library()
    st = torch.cuda.Stream()
    blob = U.weights_blob(U.synthetic_weights(3, 1))
    rows = []
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        rgb = np.random.default_rng(W).random((H, W, 3), dtype=np.float32)
        src = torch.from_numpy(rgb).to("cuda:0")
        dst = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
        c, o = (pt.nn_image_of(t.data_ptr(), format=pt.NN_FORMAT_FLOAT3) for t in (src, dst))
        with pt.NN(W, H, blob) as nn, pt.NN(W, H, blob) as watched:
            reports = []
            watched.set_progress(lambda n: reports.append(n) or True)
            s = st.cuda_stream
            calls = dict(images_hdr=lambda: nn.images_device(c, o, hdr=1, input_scale=0.5, stream=s),
                         lightmap_hdr=lambda: nn.lightmap_device(c, o, input_scale=0.5, stream=s),
                         images_normal=lambda: nn.images_device(c, o, role="normal", stream=s),
                         lightmap_dir=lambda: nn.lightmap_device(c, o, directional=True, stream=s),
                         monitor=lambda: watched.lightmap_device(c, o, input_scale=0.5, stream=s))
            for f in calls.values():
                for _ in range(3):
                    f()
            st.synchronize()
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
            row = dict(res=size, calls_each=args.rounds * args.inner, reports_per_call=len(reports) // (3 + args.rounds * args.inner))
            for k in calls:
                row[k + "_ms"] = round(float(np.median(ms[k])), 3)
                row[k + "_min_ms"] = round(float(np.min(ms[k])), 3)
                row[k + "_max_ms"] = round(float(np.max(ms[k])), 3)
            st.synchronize()
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
    return rows


if __name__ == "__main__":
    main()
