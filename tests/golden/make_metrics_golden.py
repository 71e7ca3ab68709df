"""Writes tests/golden/metrics/metrics_cases.npz: what the reference's training/ssim.py returns for the seeded images of
tests/metricscases.py (transform none), so that tests/test_metrics_cpu.py pins the restatements to it where the reference tree is absent.  Seeds, shapes and
scalars only -- the images are made again from the seeds.

    python tests/golden/make_metrics_golden.py /path/to/reference

Needs torch (CPU) and the reference tree; nothing of its text is stored.  The file has a directory of its own: the fixtures directly
under tests/golden/ are those tests/golden/make_golden.py lists with their provenance.  In its terms this one is [direct]: ssim.py's
own ssim and ms_ssim were called."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import metricscases as M  # noqa: E402


def reference_values(ssim_module, a, b, dtype):
    """(ssim, ms_ssim or NaN) of ssim.py on (H, W, 3) images at data_range 1, in `dtype` on the CPU"""
    x = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))[None]).to(dtype)
    y = torch.from_numpy(np.ascontiguousarray(b.transpose(2, 0, 1))[None]).to(dtype)
    s = float(ssim_module.ssim(x, y, data_range=1.))
    m = float(ssim_module.ms_ssim(x, y, data_range=1.)) if min(a.shape[:2]) > 160 else float("nan")
    return s, m


def golden_cases():
    return [(s, d, seed) for s in M.SSIM_SHAPES for d in M.DISTS for seed in M.SEEDS]


def main(reference_root):
    sys.path.insert(0, os.path.join(reference_root, "training"))
    import ssim as ssim_module
    rows = []
    for shape, dist, seed in golden_cases():
        a, b = M.images(shape, dist, seed)
        rows.append((shape[0], shape[1], M.DISTS.index(dist), seed) + reference_values(ssim_module, a, b, torch.float64) +
                    reference_values(ssim_module, a, b, torch.float32))
    rows = np.array(rows, np.float64)
    os.makedirs(os.path.join(HERE, "metrics"), exist_ok=True)
    np.savez(os.path.join(HERE, "metrics", "metrics_cases.npz"), width=rows[:, 0].astype(np.int32), height=rows[:, 1].astype(np.int32),
             dist=rows[:, 2].astype(np.int32), seed=rows[:, 3].astype(np.int32), ssim64=rows[:, 4], msssim64=rows[:, 5], ssim32=rows[:, 6],
             msssim32=rows[:, 7], window=ssim_module._fspecial_gauss_1d(11, 1.5).numpy().reshape(-1))
    print("wrote", len(rows), "cases")


if __name__ == "__main__":
    main(sys.argv[1])
