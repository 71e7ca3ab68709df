"""Device time of the image metrics (ptx_metrics_compare_device) at 1920x1080 and 3840x2160: hipEvents on one stream around `inner`
back-to-back calls, the figure the median over the rounds with minimum and maximum next to it, the calls alternated within a round.
A call waits for its result (the means are finished on the host), so a figure is a whole call: its kernels, the wait and the 224-byte
read-back.
    all_ms        every metric: prep, grad, four pools, five SSIM launches, finish
    pointwise_ms  pointwise_only = 1: prep, grad, finish
    torch_ms      the yardstick: SSIM and MS-SSIM written here on PyTorch-ROCm -- a grouped conv2d per direction over the five stacked
                  quantities, avg_pool2d between the scales -- on planar float32 tensors already on the device, the two scalars read back
Bytes model (what must cross HBM if every value is read and written once; 4-byte floats, packed Float3 inputs), per call:
    prep  reads both images (24 B / pixel) and writes both planar level 0 (24); grad reads level 0 of both (24);
    SSIM at scale s reads both planes of that scale (24 B / pixel of the scale); a pool reads the scale above (24) and writes its own (24)
    all = prep + grad + sum over scales; pointwise = prep + grad.  The aprons (a 42 x 26 tile for 32 x 16 results, 2.13 x) are re-reads the
    model leaves to the caches.  The share is bytes / time against 8 TB/s.
    python tools/gpu_metrics_rate.py [--rounds N] [--inner M] [--sizes WxH,..] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mygpuraytracer_amd as pt  # noqa: E402

HBM_BYTES_PER_S = 8e12


def window(torch, device):
    k = torch.arange(11, dtype=torch.float32, device=device) - 5
    g = torch.exp(-(k * k) / 4.5)
    return g / g.sum()


def torch_ssim_chain(torch, x, y, g, weights):
    """(ssim, ms_ssim) of planar (1, 3, H, W) tensors, data range 1"""
    F = torch.nn.functional
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    kx, ky = g.view(1, 1, 1, 11).repeat(15, 1, 1, 1), g.view(1, 1, 11, 1).repeat(15, 1, 1, 1)
    mcs, ssim0 = [], None
    for s in range(5):
        if s:
            pad = (x.shape[2] % 2, x.shape[3] % 2)
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
        q = torch.cat((x, y, x * x, y * y, x * y), 1)
        f = F.conv2d(F.conv2d(q, kx, groups=15), ky, groups=15)
        m1, m2, fxx, fyy, fxy = f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9:12], f[:, 12:15]
        cs = (2 * (fxy - m1 * m2) + c2) / ((fxx - m1 * m1) + (fyy - m2 * m2) + c2)
        full = (2 * m1 * m2 + c1) / (m1 * m1 + m2 * m2 + c1) * cs
        if s == 0:
            ssim0 = full.mean()
        mcs.append((cs if s < 4 else full).mean((2, 3)))
    stack = torch.stack(mcs, -1)
    return ssim0, torch.prod(torch.relu(stack) ** weights, -1).mean()


def model_bytes(plan):
    level0 = plan["w"][0] * plan["h"][0]
    pointwise = 72 * level0
    total = pointwise
    for s in range(int(plan["scales"])):
        n = int(plan["w"][s]) * int(plan["h"][s])
        total += 24 * n
        if s:
            total += 24 * int(plan["w"][s - 1]) * int(plan["h"][s - 1]) + 24 * n
    return int(total), int(pointwise)


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
    rows = []
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(W)
        b = rng.random((H, W, 3), dtype=np.float32)
        a = np.clip(b + 0.15 * rng.standard_normal((H, W, 3), dtype=np.float32), 0, 1)
        da, db = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
        ia, ib = (pt.nn_image_of(t.data_ptr(), format=pt.NN_FORMAT_FLOAT3) for t in (da, db))
        xa, xb = (t.permute(2, 0, 1)[None].contiguous() for t in (da, db))
        g, weights = window(torch, "cuda:0"), torch.tensor([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], device="cuda:0")
        plan = pt.debug_metrics_plan(W, H)
        total_bytes, pointwise_bytes = model_bytes(plan)
        with pt.Metrics(W, H) as m:
            s = st.cuda_stream
            seen = {}

            def torch_call():
                with torch.cuda.stream(st):
                    v = torch_ssim_chain(torch, xa, xb, g, weights)
                    seen["torch"] = (float(v[0]), float(v[1]))

            calls = dict(all=lambda: seen.__setitem__("all", m.device(ia, ib, stream=s)),
                         pointwise=lambda: m.device(ia, ib, stream=s, pointwise_only=1),
                         torch=torch_call)
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
            row = dict(res=size, calls_each=args.rounds * args.inner, model_bytes_all=total_bytes, model_bytes_pointwise=pointwise_bytes,
                       ssim=seen["all"]["ssim"], msssim=seen["all"]["msssim"], torch_ssim=seen["torch"][0], torch_msssim=seen["torch"][1])
            for k in calls:
                row[k + "_ms"] = round(float(np.median(ms[k])), 3)
                row[k + "_min_ms"] = round(float(np.min(ms[k])), 3)
                row[k + "_max_ms"] = round(float(np.max(ms[k])), 3)
            row["all_share_of_8TBs"] = round(total_bytes / (row["all_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
            row["pointwise_share_of_8TBs"] = round(pointwise_bytes / (row["pointwise_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
    return rows


if __name__ == "__main__":
    main()
