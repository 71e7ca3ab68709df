"""Device time of the network denoiser (ptx_nn_denoise_device) at 1920x1080 and 3840x2160 for weights with 3, 6 and 9 input channels
(synthetic, the standard channel table: time does not depend on the weights' values), next to PyTorch's own fp16 channels-last conv2d
chain of the same shapes on the same device -- the one independent yardstick there is.  hipEvents on one stream around `inner`
back-to-back calls, the two alternated within a run, the figure the median over the rounds (the minimum next to it).
    ms            per denoise: input kernel, sixteen convolutions, output kernel (LDR, scale 1: no meter)
    tflops        2 * MACs of one run (ptx_nn_get_info) over that time, and its share of the 2.5 PFLOP/s dense fp16 peak
    bytes model   what the layers have to move at least: each layer reads its sources once and writes its output once (fp16, padded
                  channels; the pooled layers write the pooled tensor, the two-source layers read the small tensor and the skip), plus the
                  frames in and out; over 8 TB/s
The unfused forms of the two fusions (a materialised upsample + concat, an unpooled tensor and a pool pass) do not exist in the library,
so there is no on / off pair to time: the fused forms are the only ones.
    --max-memory-mb L[,L..]  one row per limit from a handle made under it (ptx_nn_create_tiled; 0 = no limit but the tile cap): the
                  tile grid and size, the tile's scratch, and area_ratio = the tiles' padded area over the frame's padded area, from the
                  plan -- the extra work tiling costs.  Without it: ptx_nn_create, one tile, as before.
    --other-lib SO  another build of the library (the parent commit's), its one-tile ptx_nn_denoise_device alternated with this one's in
                  the same rounds: other_ms next to ours_ms, and each one's spread (min .. max over the rounds); --other-first: the
                  other build goes first in every round
    python tools/gpu_nn_rate.py [--rounds N] [--inner M] [--no-torch] [--ics 3,6,9] [--max-memory-mb L,..] [--other-lib SO [--other-first]] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mygpuraytracer_amd as pt  # noqa: E402
import unet_ref as U  # noqa: E402

HBM_PEAK, FP16_PEAK = 8.0e12, 2.5e15
LEVELS = (0, 0, 1, 2, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 0)
POOLED = (1, 2, 3, 4)
pad16 = lambda c: (c + 15) // 16 * 16


def bytes_model(ic, w, h):
    wp, hp = pad16(w), pad16(h)
    total = w * h * 4 * (ic + 3)                                    # the fp32 frames in and the fp32 frame out
    total += wp * hp * (16 * 2 + 16 * 2 + 16)                       # the input tensor written, dec_conv0's fp32 output written and read
    for i, ((_, cin, cout), lv) in enumerate(zip(U.standard_channels(ic), LEVELS)):
        px = (wp >> lv) * (hp >> lv)
        if isinstance(cin, tuple):
            total += (px // 4) * pad16(cin[0]) * 2 + px * pad16(cin[1]) * 2
        else:
            total += px * pad16(cin) * 2
        if i < 15:
            total += (px // 4 if i in POOLED else px) * pad16(cout) * 2
    return total


class TorchChain:
    """the same sixteen convolutions in PyTorch: fp16, channels-last, pool / upsample / cat as torch ops"""

    def __init__(self, ic, weights, torch):
        self.torch = torch
        cl = torch.channels_last
        self.w = {k: torch.from_numpy(v).to("cuda:0", torch.float16) for k, v in weights.items()}
        self.w = {k: (v.contiguous(memory_format=cl) if v.ndim == 4 else v) for k, v in self.w.items()}

    def __call__(self, x):
        F = self.torch.nn.functional
        c = lambda t, n, relu=True: (F.relu(F.conv2d(t, self.w[n + ".weight"], self.w[n + ".bias"], padding=1)) if relu
                                     else F.conv2d(t, self.w[n + ".weight"], self.w[n + ".bias"], padding=1))
        t = c(x, "enc_conv0")
        p1 = F.max_pool2d(c(t, "enc_conv1"), 2)
        p2 = F.max_pool2d(c(p1, "enc_conv2"), 2)
        p3 = F.max_pool2d(c(p2, "enc_conv3"), 2)
        p4 = F.max_pool2d(c(p3, "enc_conv4"), 2)
        t = c(c(p4, "enc_conv5a"), "enc_conv5b")
        for lv, skip in (("4", p3), ("3", p2), ("2", p1), ("1", x)):
            t = self.torch.cat([F.interpolate(t, scale_factor=2, mode="nearest"), skip], 1)
            t = c(c(t, "dec_conv%sa" % lv), "dec_conv%sb" % lv)
        return c(t, "dec_conv0", relu=False)


class OtherLibrary:
    """one-tile handles of another build of the library, through the three entry points every build has"""

    def __init__(self, path):
        L = self.L = ctypes.CDLL(os.path.abspath(path))
        vp, i = ctypes.c_void_p, ctypes.c_int
        L.ptx_nn_create.restype, L.ptx_nn_create.argtypes = i, [i, i, i, vp, ctypes.c_size_t, ctypes.POINTER(vp)]
        L.ptx_nn_denoise_device.restype, L.ptx_nn_denoise_device.argtypes = i, [vp, vp, ctypes.c_float, vp, vp, vp, vp, vp]
        L.ptx_nn_destroy.restype, L.ptx_nn_destroy.argtypes = None, [vp]
        L.ptx_last_error.restype = ctypes.c_char_p

    def handle(self, w, h, blob):
        n = ctypes.c_void_p()
        if self.L.ptx_nn_create(0, w, h, ctypes.cast(ctypes.c_char_p(blob), ctypes.c_void_p), len(blob), ctypes.byref(n)):
            raise RuntimeError(self.L.ptx_last_error().decode())
        return n

    def denoise(self, n, ptrs, out_ptr, stream, params):
        if self.L.ptx_nn_denoise_device(n, ptrs[0], 1.0, ptrs[1], ptrs[2], ctypes.byref(params), out_ptr, stream):
            raise RuntimeError(self.L.ptx_last_error().decode())


def area_ratio(t):
    """the tiles' padded area over the frame's padded area"""
    return sum(pad16(k["w"]) * pad16(k["h"]) for k in t["tiles"]) / (pad16(t["width"]) * pad16(t["height"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--ics", default="3,6,9")
    ap.add_argument("--max-memory-mb", default=None)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--other-first", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    limits = [None] if args.max_memory_mb is None else [int(v) for v in args.max_memory_mb.split(",")]
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")                # PyTorch's convolutions: no exhaustive search per shape
    import torch
    pt.load_library()
    other = OtherLibrary(args.other_lib) if args.other_lib else None      # after torch and this tree's library: one HIP runtime in the process
    rows = []
    st = torch.cuda.Stream()
    for W, H in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        for ic, limit in ((int(v), l) for v in args.ics.split(",") for l in limits):
            weights = U.synthetic_weights(ic, 1)
            blob = U.weights_blob(weights)
            rng = np.random.default_rng(W + ic)
            frames = [torch.from_numpy(rng.random((H, W, 3), dtype=np.float32)).to("cuda:0") for _ in range(ic // 3)]
            out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
            with pt.NN(W, H, blob, max_memory_mb=limit) as nn:
                info = nn.info()
                ptrs = [f.data_ptr() for f in frames] + [None, None]
                ours = lambda: nn.device(ptrs[0], out.data_ptr(), albedo_ptr=ptrs[1], normal_ptr=ptrs[2], stream=st.cuda_stream, srgb=1, input_scale=1.0)
                calls = dict(ours=ours)
                if other:
                    theirs_nn, theirs_p = other.handle(W, H, blob), pt.default_nn_params(srgb=1, input_scale=1.0)
                    calls["other"] = lambda: other.denoise(theirs_nn, ptrs, out.data_ptr(), st.cuda_stream, theirs_p)
                    if args.other_first:                         # the order within a round, to tell a difference of the builds from one of the place
                        calls = dict(other=calls["other"], ours=ours)
                if not args.no_torch:
                    chain = TorchChain(ic, weights, torch)
                    hp, wp = pad16(H), pad16(W)
                    x = torch.rand((1, ic, hp, wp), device="cuda:0").to(torch.float16).contiguous(memory_format=torch.channels_last)

                    def theirs():
                        with torch.cuda.stream(st), torch.no_grad():
                            chain(x)
                    calls["torch"] = theirs
                for f in calls.values():                             # warm-up: code objects, the library's choice of algorithm
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
                flop, b = 2.0 * info["macs"], bytes_model(ic, W, H)
                row = dict(res="%dx%d" % (W, H), ic=ic, calls_each=args.rounds * args.inner, gmacs=round(info["macs"] / 1e9, 2),
                           scratch_mib=round(info["scratch_bytes"] / 2 ** 20, 1), bytes_model_mib=round(b / 2 ** 20, 1))
                if limit is not None:
                    t = nn.tiling()
                    row.update(max_memory_mb=limit, tiles="%dx%d" % (t["tiles_x"], t["tiles_y"]), tile="%dx%d" % (t["tile_width"], t["tile_height"]),
                               area_ratio=round(area_ratio(t), 3))
                for k in calls:
                    med = float(np.median(ms[k]))
                    row[k + "_ms"] = round(med, 3)
                    row[k + "_min_ms"] = round(float(np.min(ms[k])), 3)
                    row[k + "_max_ms"] = round(float(np.max(ms[k])), 3)
                    row[k + "_tflops"] = round(flop / med / 1e9, 1)
                    row[k + "_share_of_fp16_peak"] = round(flop / med / 1e-3 / FP16_PEAK, 4)
                row["ours_bytes_model_share_of_8TBs"] = round(b / HBM_PEAK * 1e3 / row["ours_ms"], 4)
                if "torch" in calls:
                    row["ours_over_torch"] = round(row["ours_ms"] / row["torch_ms"], 3)
                if other:
                    st.synchronize()
                    other.L.ptx_nn_destroy(theirs_nn)
                rows.append(row)
                print(json.dumps(row), flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(row) + "\n")
    return rows


if __name__ == "__main__":
    main()
