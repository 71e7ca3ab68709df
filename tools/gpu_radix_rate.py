#!/usr/bin/env python3
"""Rates of the radix sort of records by full 32-bit keys (sc_radix_sort_records_device) on one GPU, next to the one-pass counting sort
of the same records, to the same job composed from torch operators and to a device-to-device copy of the records.  Same method as
tools/gpu_records_rate.py; not part of bench.py: nothing the headline measures runs here.

    python tools/gpu_radix_rate.py [--out profiles/radix_sort_rate.txt] [--runs 9] [--calls 20]

Per size (1920x1080 and 3840x2160 records), 32-byte intersections + 44-byte path segments permuted alike:
  radix i32 [0,32)   random full-range int32 keys from an array of their own, four passes
  radix i32 [0,16)   the same keys, their low 16 bits, two passes
  radix i32 [0,8)    the 7 material ids read at materialId's offset inside the intersections, descending, one pass
  radix f32 [0,32)   random float32 keys, four passes
  one-pass 7 keys    sc_sort_records_by_key_device on the job of `radix i32 [0,8)`            (the counting sort this builds on)
  torch ...          the same jobs from torch: torch.sort(stable=True) of the (masked) keys + one index_select per array
  copy               torch's device-to-device copy of the same record bytes
Timing: torch (hip) events on a side stream around `calls` back-to-back calls after a warm-up of every variant, the variants taken in
turn inside every run, the median over `runs` runs.  Bytes model (what the algorithm has to move, not what the caches saw): per pass
the keys read twice (4 B each) and a pair written once (8 B); the gather reads the index (4 B) and moves every record once each way
(76 B in, 76 B out).  The torch variants and the one-pass sort are rated by the model of the job they do, so GB/s compares like
with like and ms compares everything."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "radix_sort_rate.txt"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    a = ap.parse_args()
    import torch
    import mygpuraytracer_amd as pt
    if not torch.cuda.is_available() or pt.load_library().ptx_device_count() < 1:
        sys.exit("gpu_radix_rate.py needs a HIP device: there is nothing to time without one")
    sc = pt.StreamCompaction()
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    lines = ["# tools/gpu_radix_rate.py on %s: median of %d runs of %d calls, hip events on a side stream" % (torch.cuda.get_device_name(0), a.runs, a.calls),
             "# GB/s by the bytes model: 16 B per element and pass (keys twice, a pair once) + 4 B index + 2 x 76 B records; x copy = share of the copy's GB/s",
             "%-10s %-26s %6s %10s %10s %8s" % ("n", "variant", "passes", "ms", "GB/s", "x copy")]
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        n, nkeys = w * h, 7
        rng = np.random.default_rng(n)
        isect = torch.from_numpy(rng.standard_normal((n, 8)).astype(np.float32)).to(dev)
        mat = torch.from_numpy(rng.integers(0, nkeys, n).astype(np.int32)).to(dev)
        isect[:, 4] = mat.view(torch.float32)                                      # materialId: byte 16 of 32
        path = torch.from_numpy(rng.standard_normal((n, 11)).astype(np.float32)).to(dev)
        ikeys = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)).to(dev)
        fkeys = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
        isect_out, path_out = torch.empty_like(isect), torch.empty_like(path)
        ws = torch.zeros((max(sc.radix_workspace_bytes(n), sc.records_workspace_bytes(n, nkeys)) + 7) // 8, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        st = side.cuda_stream
        res = {}

        def radix(key_type, descending, b0, b1, kptr, stride):
            sc.radix_sort_records_device(n, key_type, descending, b0, b1, kptr, stride, isect_out.data_ptr(), isect.data_ptr(), 32,
                                         path_out.data_ptr(), path.data_ptr(), 44, 0, 0, ws.data_ptr(), st)

        def radix_i32():
            radix(sc.KEY_INT32, 0, 0, 32, ikeys.data_ptr(), 4)

        def radix_i16():
            radix(sc.KEY_INT32, 0, 0, 16, ikeys.data_ptr(), 4)

        def radix_i8():
            radix(sc.KEY_INT32, 1, 0, 8, isect.data_ptr() + 16, 32)

        def radix_f32():
            radix(sc.KEY_FLOAT32, 0, 0, 32, fkeys.data_ptr(), 4)

        def onepass():
            sc.sort_records_by_key_device(n, nkeys, 1, isect.data_ptr() + 16, 32, isect_out.data_ptr(), isect.data_ptr(), 32,
                                          path_out.data_ptr(), path.data_ptr(), 44, 0, 0, ws.data_ptr(), st)

        def gathers(order):
            res["isect"], res["path"] = torch.index_select(isect, 0, order), torch.index_select(path, 0, order)

        def torch_i32():
            gathers(torch.sort(ikeys, stable=True)[1])

        def torch_i16():
            gathers(torch.sort(ikeys & 0xffff, stable=True)[1])

        def torch_i8():
            gathers(torch.sort(nkeys - 1 - isect[:, 4].view(torch.int32), stable=True)[1])

        def torch_f32():
            gathers(torch.sort(fkeys, stable=True)[1])

        def copy_both():
            isect_out.copy_(isect); path_out.copy_(path)

        def model(passes):
            return n * (16 * passes + 4 + 2 * 76)

        variants = [("radix i32 [0,32)", radix_i32, 4), ("radix i32 [0,16)", radix_i16, 2), ("radix i32 [0,8) 7 keys", radix_i8, 1), ("radix f32 [0,32)", radix_f32, 4),
                    ("one-pass sort 7 keys", onepass, 0), ("torch i32 [0,32)", torch_i32, 4), ("torch i32 [0,16)", torch_i16, 2), ("torch i32 [0,8) 7 keys", torch_i8, 1),
                    ("torch f32 [0,32)", torch_f32, 4), ("copy 32+44 B", copy_both, -1)]
        nbytes = {name: (n * 2 * 76 if passes < 0 else n * (8 + 2 * 76) if passes == 0 else model(passes)) for name, _, passes in variants}

        def same():
            return torch.equal(isect_out.view(torch.int32), res["isect"].view(torch.int32)) and torch.equal(path_out.view(torch.int32), res["path"].view(torch.int32))

        with torch.cuda.stream(side):
            # results first: faster and different is not faster
            for ours, theirs in ((radix_i32, torch_i32), (radix_i16, torch_i16), (radix_i8, torch_i8), (radix_f32, torch_f32), (onepass, torch_i8)):
                isect_out.zero_(); path_out.zero_()
                ours(); theirs(); side.synchronize()
                assert same(), ours.__name__
            for _, fn, _ in variants:
                for _ in range(3):
                    fn()
            side.synchronize()
            ms = {name: [] for name, _, _ in variants}
            for _ in range(a.runs):
                for name, fn, _ in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(side)
                    for _ in range(a.calls):
                        fn()
                    e1.record(side)
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / a.calls)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rate = {name: nbytes[name] / med[name] / 1e6 for name, _, _ in variants}
        for name, _, passes in variants:
            lines.append("%-10d %-26s %6s %10.4f %10.1f %8.2f" % (n, name, passes if passes > 0 else "-", med[name], rate[name], rate[name] / rate["copy 32+44 B"]))
        res.clear()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
