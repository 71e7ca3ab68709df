#!/usr/bin/env python3
"""Rates of the record primitives of the compaction library on one GPU, next to a device-to-device copy of the same records and to the
same job composed from torch operators.  Not part of bench.py: the tracer fuses its own sort, nothing the headline measures runs here.

    python tools/gpu_records_rate.py [--out profiles/records_rate.txt] [--runs 9] [--calls 20]

Per size (1920x1080 and 3840x2160 records):
  sort       sc_sort_records_by_key_device: 32-byte intersections + 44-byte path segments, 7 keys read at materialId's offset inside
             the intersections, descending                    (thrust::sort_by_key(.., sortByMaterial()), src/pathtrace.cu:518)
  partition  sc_partition_records_device: the 44-byte segments, ~46 % kept (config 4's first-bounce survival), flag read at
             remainingBounces' offset                         (thrust::stable_partition(.., isTerminate()), src/pathtrace.cu:541)
  compact    sc_compact_records_device on the same
  copy       torch's device-to-device copy of the same record bytes (read once, written once)
  torch      the same job on the same buffers: torch.sort(stable=True) of the keys (read out of the intersections, as a strided view)
             + one index_select per array; a boolean-mask gather per half, the mask from the flag inside the segments
Timing: torch (hip) events on a side stream around `calls` back-to-back calls after a warm-up of every variant, the variants taken in
turn inside every run, the median over `runs` runs.  Bytes model (what the algorithm has to move, not what the caches saw): keys or
flags read twice (4 B each time), every record read once and written once; compaction writes the survivors only.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "records_rate.txt"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    a = ap.parse_args()
    import torch
    import mygpuraytracer_amd as pt
    if not torch.cuda.is_available() or pt.load_library().ptx_device_count() < 1:
        sys.exit("gpu_records_rate.py needs a HIP device: there is nothing to time without one")
    sc = pt.StreamCompaction()
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    lines = ["# tools/gpu_records_rate.py on %s: median of %d runs of %d calls, hip events on a side stream" % (torch.cuda.get_device_name(0), a.runs, a.calls),
             "# GB/s by the bytes model (keys twice, records once in and once out; compaction writes survivors only); x copy = share of the copy's GB/s",
             "%-10s %-22s %10s %10s %8s" % ("n", "variant", "ms", "GB/s", "x copy")]
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        n, nkeys = w * h, 7
        rng = np.random.default_rng(n)
        isect = torch.from_numpy(rng.standard_normal((n, 8)).astype(np.float32)).to(dev)
        mat = torch.from_numpy(rng.integers(0, nkeys, n).astype(np.int32)).to(dev)
        isect[:, 4] = mat.view(torch.float32)                                      # materialId: byte 16 of 32
        path = torch.from_numpy(rng.standard_normal((n, 11)).astype(np.float32)).to(dev)
        live = torch.from_numpy(((rng.random(n) < 0.46) * rng.integers(1, 8, n)).astype(np.int32)).to(dev)
        path[:, 10] = live.view(torch.float32)                                     # remainingBounces: byte 40 of 44
        kept = int((live != 0).sum().item())
        isect_out, path_out = torch.empty_like(isect), torch.empty_like(path)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.zeros((sc.records_workspace_bytes(n, nkeys) + 7) // 8, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        st = side.cuda_stream
        res = {}

        def ours_sort():
            sc.sort_records_by_key_device(n, nkeys, 1, isect.data_ptr() + 16, 32, isect_out.data_ptr(), isect.data_ptr(), 32,
                                          path_out.data_ptr(), path.data_ptr(), 44, 0, 0, ws.data_ptr(), st)

        def ours_partition():
            sc.partition_records_device(n, 44, path_out.data_ptr(), path.data_ptr(), path.data_ptr() + 40, 44, count.data_ptr(), ws.data_ptr(), st)

        def ours_compact():
            sc.compact_records_device(n, 44, path_out.data_ptr(), path.data_ptr(), path.data_ptr() + 40, 44, count.data_ptr(), ws.data_ptr(), st)

        def copy_both():
            isect_out.copy_(isect); path_out.copy_(path)

        def copy_path():
            path_out.copy_(path)

        def torch_sort():
            order = torch.sort(nkeys - 1 - isect[:, 4].view(torch.int32), stable=True)[1]
            res["isect"], res["path"] = torch.index_select(isect, 0, order), torch.index_select(path, 0, order)

        def torch_partition():
            m = path[:, 10].view(torch.int32) != 0
            res["part"] = torch.cat([path[m], path[~m]])

        def torch_compact():
            res["comp"] = path[path[:, 10].view(torch.int32) != 0]

        sort_bytes, part_bytes = n * (8 + 2 * 76), n * (8 + 2 * 44)
        variants = [("sort 32+44 B, 7 keys", ours_sort, sort_bytes, "copy76"), ("copy 32+44 B", copy_both, n * 2 * 76, "copy76"),
                    ("torch sort+2 gathers", torch_sort, sort_bytes, "copy76"),
                    ("partition 44 B, 46 %", ours_partition, part_bytes, "copy44"), ("compact 44 B, 46 %", ours_compact, n * (8 + 44) + kept * 44, "copy44"),
                    ("copy 44 B", copy_path, n * 2 * 44, "copy44"), ("torch 2 mask gathers", torch_partition, part_bytes, "copy44"),
                    ("torch 1 mask gather", torch_compact, n * (8 + 44) + kept * 44, "copy44")]
        with torch.cuda.stream(side):
            # results first: faster and different is not faster
            ours_sort(); torch_sort(); side.synchronize()
            assert torch.equal(isect_out.view(torch.int32), res["isect"].view(torch.int32)) and torch.equal(path_out.view(torch.int32), res["path"].view(torch.int32))
            ours_partition(); torch_partition(); side.synchronize()
            assert int(count.item()) == kept and torch.equal(path_out.view(torch.int32), res["part"].view(torch.int32))
            for _, fn, _, _ in variants:
                for _ in range(3):
                    fn()
            side.synchronize()
            ms = {name: [] for name, _, _, _ in variants}
            for _ in range(a.runs):
                for name, fn, _, _ in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(side)
                    for _ in range(a.calls):
                        fn()
                    e1.record(side)
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / a.calls)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rate = {name: nbytes / med[name] / 1e6 for name, _, nbytes, _ in variants}
        copies = {"copy76": rate["copy 32+44 B"], "copy44": rate["copy 44 B"]}
        for name, _, _, ref in variants:
            lines.append("%-10d %-22s %10.4f %10.1f %8.2f" % (n, name, med[name], rate[name], rate[name] / copies[ref]))
        res.clear()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
