"""Device time of the network denoiser's image entry point (ptx_nn_denoise_images_device) beside the packed one (ptx_nn_denoise_device)
at 1920x1080 and 3840x2160, 6 inputs, LDR, by tools/gpu_nn_prefilter_rate.py's method: hipEvents on one stream around `inner`
back-to-back calls, the calls alternated within a round, the figure the median over the rounds (minimum and maximum next to it).
Synthetic weights on the standard channel table: time does not depend on the weights' values.
    packed_ms        ptx_nn_denoise_device on W*H*3 floats: the yardstick, in the same process and rounds
    float3_ms        the image call on packed Float3 descriptors of the same buffers
    float4_ms        the image call on float4 colour, albedo and output
    half4_ms         the image call on half4 colour, albedo and output
At the sizes of --tiled-sizes (3840x2160), with a second handle made under --max-memory-mb (512):
    tiled_ms         the image call on packed Float3, the output apart from the inputs
    tiled_inplace_ms the same with the output over the colour: the temporary and the copy kernel
    --packed-last    the packed call closes every round instead of opening it (what the place in the round is worth)
    python tools/gpu_nn_image_rate.py [--rounds N] [--inner M] [--sizes WxH,..] [--tiled-sizes WxH,..] [--max-memory-mb L] [--packed-last] [--out FILE]"""
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
    ap.add_argument("--tiled-sizes", default="3840x2160")
    ap.add_argument("--max-memory-mb", type=int, default=512)
    ap.add_argument("--packed-last", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pt.load_library()
    st = torch.cuda.Stream()
    blob = U.weights_blob(U.synthetic_weights(6, 1))
    tiled_sizes = args.tiled_sizes.split(",") if args.tiled_sizes else []
    rows = []
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(W)
        dev = lambda a: torch.from_numpy(a).to("cuda:0")
        rgb, alb = (rng.random((H, W, 3), dtype=np.float32) for _ in range(2))
        pad = lambda a, dtype: np.concatenate([a, np.ones((H, W, 1), np.float32)], axis=2).astype(dtype)
        f3 = [dev(rgb), dev(alb), torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")]
        f4 = [dev(pad(rgb, np.float32)), dev(pad(alb, np.float32)), torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")]
        h4 = [dev(pad(rgb, np.float16)), dev(pad(alb, np.float16)), torch.zeros((H, W, 4), dtype=torch.float16, device="cuda:0")]
        d3 = [pt.nn_image_of(t.data_ptr(), format=pt.NN_FORMAT_FLOAT3) for t in f3]
        d4 = [pt.nn_image_of(t.data_ptr(), format=pt.NN_FORMAT_FLOAT3, pixel_stride=16) for t in f4]
        dh = [pt.nn_image_of(t.data_ptr(), format=pt.NN_FORMAT_HALF3, pixel_stride=8) for t in h4]
        with pt.NN(W, H, blob) as nn:
            image = lambda d, n=nn, out=None: n.images_device(d[0], out or d[2], albedo=d[1], stream=st.cuda_stream)
            calls = dict(packed=lambda: nn.device(f3[0].data_ptr(), f3[2].data_ptr(), albedo_ptr=f3[1].data_ptr(), stream=st.cuda_stream),
                         float3=lambda: image(d3), float4=lambda: image(d4), half4=lambda: image(dh))
            tiled = None
            if size in tiled_sizes:
                tiled = pt.NN(W, H, blob, max_memory_mb=args.max_memory_mb)
                spare = dev(rgb)                                     # the in-place call's colour: its result replaces it, call after call
                dspare = pt.nn_image_of(spare.data_ptr(), format=pt.NN_FORMAT_FLOAT3)
                calls["tiled"] = lambda: image(d3, tiled)
                calls["tiled_inplace"] = lambda: image([dspare, d3[1], dspare], tiled)
            if args.packed_last:
                calls["packed"] = calls.pop("packed")
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
            row = dict(res=size, calls_each=args.rounds * args.inner, scratch_mib=round(nn.info()["scratch_bytes"] / 2 ** 20, 1))
            if tiled:
                t = tiled.tiling(tiles=False)
                row.update(max_memory_mb=args.max_memory_mb, tiles="%dx%d" % (t["tiles_x"], t["tiles_y"]), tiled_scratch_mib=round(t["scratch_bytes"] / 2 ** 20, 1))
            for k in calls:
                row[k + "_ms"] = round(float(np.median(ms[k])), 3)
                row[k + "_min_ms"] = round(float(np.min(ms[k])), 3)
                row[k + "_max_ms"] = round(float(np.max(ms[k])), 3)
            st.synchronize()
            if tiled:
                tiled.close()
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
    return rows


if __name__ == "__main__":
    main()
