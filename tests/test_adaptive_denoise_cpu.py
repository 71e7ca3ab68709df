"""CPU: the definition of the variance-guided filter on an adaptively sampled frame (tests/adaptive_denoise_ref.py against the
restatements it is composed from), its C-ABI surface without a device, the headless driver's flag, and what the compiler made of its
kernel.  The device is held to the same restatement by tests/test_gpu_adaptive_denoise.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from adaptive_denoise_ref import denoise_adaptive, measured_v0_pixels
from adaptive_ref import tile_of
from moments_ref import LUM, measured_v0, quad
from resource_usage import kernels_named, resource_usage
from variance_ref import denoise_buffers_variance


def _frame(h, w, seed):
    """a synthetic frame with its guides: two planes that meet in the middle column, one miss pixel in a corner"""
    rng = np.random.default_rng(seed)
    hit = np.ones((h, w), bool)
    hit[0, 0] = False
    left = (np.arange(w) < w // 2)[None, :, None]
    normal = np.where(left, [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]) * np.ones((h, w, 1))
    position = np.stack(np.meshgrid(np.arange(w) * 0.1, np.arange(h) * 0.1), -1)
    position = np.concatenate([position, np.zeros((h, w, 1))], -1)
    albedo = 0.2 + 0.8 * rng.random((h, w, 3))
    ids = np.where(left, 1, 2) * np.ones((h, w, 2), np.int64)
    for a in (normal, position, albedo):
        a[~hit] = 0.0
    L = rng.standard_normal((h, w, 3, 3)) * 0.3
    C = L @ np.swapaxes(L, -1, -2)                                   # a covariance per pixel
    mean = 0.1 + rng.random((h, w, 3))
    return dict(hit=hit, normal=normal, position=position, albedo=albedo, ids=ids, C=C, mean=mean)


def test_one_count_for_all_tiles_is_the_measured_filter():
    """every tile with 48 samples and 6 batches: the restatement is variance_ref.denoise_buffers_variance on acc / 48 with
    moments_ref.measured_v0 -- exactly, for both colour spaces; below min_batches it is the all-spatial one, variance=None"""
    h, w, tp, n, B = 6, 10, 8, 48, 6
    f = _frame(h, w, 3)
    nt = -(-h * w // tp)
    acc = (f["mean"] * n).astype(np.float32)
    guides = (f["albedo"], f["normal"], f["position"], f["hit"])
    for demod in (1, 0):
        got = denoise_adaptive(acc, [n] * nt, f["C"], np.full((h, w), B), *guides, ids=f["ids"], tile_px=tp, demodulate=demod, passes=3)
        v0 = measured_v0(f["C"], n, B, f["hit"], f["albedo"], demod, 4)
        assert not np.isnan(v0).any() and not got[3].any()
        want = denoise_buffers_variance(acc.astype(np.float64) / n, *guides, ids=f["ids"], variance=v0, demodulate=demod, passes=3)
        for a, b in zip(got[:3], want):
            assert np.array_equal(a, b), demod
        assert v0[f["hit"]].min() > 0 and not got[2][~f["hit"]].any()
        got = denoise_adaptive(acc, [n] * nt, f["C"], np.full((h, w), B), *guides, ids=f["ids"], tile_px=tp, demodulate=demod, passes=3,
                               min_batches=B + 1)
        want = denoise_buffers_variance(acc.astype(np.float64) / n, *guides, ids=f["ids"], variance=None, demodulate=demod, passes=3)
        assert (got[3] == f["hit"]).all()
        for a, b in zip(got[:3], want):
            assert np.array_equal(a, b), demod


def test_two_tiles_of_8_and_64_samples_by_hand():
    """2 x 4 in tiles of 4: the upper row holds 8 samples in 2 batches, the lower 64 in 8, every pixel the same covariance and albedo.
    c is the buffer over the row's own count; the measured v0 scales as 1 / W; and with min_batches = 4 exactly the upper row's hit
    pixels fall back to the spatial estimate."""
    h, w, tp = 2, 4, 4
    hit = np.ones((h, w), bool)
    hit[1, 3] = False
    C = np.broadcast_to(np.array([[0.5, 0.1, 0.0], [0.1, 0.3, 0.05], [0.0, 0.05, 0.2]]), (h, w, 3, 3)).copy()
    albedo = np.full((h, w, 3), 0.5) * hit[..., None]
    normal = np.array([0.0, 0.0, 1.0]) * hit[..., None]
    position = np.zeros((h, w, 3))
    samples = np.array([8, 64])
    W, B = samples[tile_of(h, w, tp)], np.array([2, 8])[tile_of(h, w, tp)]
    assert W.tolist() == [[8] * 4, [64] * 4]
    acc = np.float32(W)[..., None] * np.float32([0.25, 0.5, 1.0])          # the same mean radiance everywhere
    q = float(LUM @ C[0, 0] @ LUM)
    for demod, scale in ((0, 1.0), (1, 4.0)):                              # g / 0.5: the form is 4 x as large
        v = measured_v0_pixels(C, W, B, hit, albedo, demod, min_batches=2)
        assert np.allclose(v[0], scale * q / 8, rtol=1e-14) and np.allclose(v[1, :3], scale * q / 64, rtol=1e-14) and v[1, 3] == 0.0
        assert np.allclose(v[0, 0] / v[1, 0], 8.0, rtol=1e-14)
        v = measured_v0_pixels(C, W, B, hit, albedo, demod, min_batches=4)
        assert np.array_equal(np.isnan(v), hit & (B < 4)) and np.isnan(v[0]).all() and not np.isnan(v[1]).any()
        out, vout, v0, fallback = denoise_adaptive(acc, samples, C, B, albedo, normal, position, hit, tile_px=tp, min_batches=4, demodulate=demod,
                                                   passes=2)
        assert np.array_equal(fallback, hit & (B < 4))
        assert (v0[0] < 1e-28).all()                      # a constant row: its spatial variance is 0 (to float64's rounding, squared)
        assert np.allclose(v0[1, :3], scale * q / 64, rtol=1e-14) and v0[1, 3] == 0.0 and vout[1, 3] == 0.0
        assert np.allclose(out[hit], [0.25, 0.5, 1.0], rtol=1e-12)          # acc / its own count, filtered among equals
        assert np.allclose(out[1, 3], [0.25, 0.5, 1.0], rtol=1e-7)          # a miss pixel keeps its colour
    assert np.isclose(quad(C, LUM)[0, 0], q)


def test_symbol_and_refusals_before_any_device_work(product):
    lib = product.load_library()
    header = open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()
    assert re.search(r"\bptx_denoise_adaptive\(", header) and hasattr(lib, "ptx_denoise_adaptive")
    assert lib.ptx_abi_version() == 5                    # no existing struct or entry point changed
    err = lambda: lib.ptx_last_error().decode()
    INVALID = 1
    assert lib.ptx_denoise_adaptive(None, None, None, None, None, 0) == INVALID and "null" in err()
    assert lib.ptx_denoise_adaptive(None, None, None, None, None, 4) == INVALID and "null" in err()
    assert lib.ptx_denoise_adaptive(None, None, None, None, None, 1) == INVALID and "min_batches" in err()
    for bad, what in ((dict(passes=0), "passes"), (dict(passes=11), "passes"), (dict(phi_normal=0.0), "phi_normal")):
        p = product.default_denoise_params(**bad)
        assert lib.ptx_denoise_adaptive(None, None, None, ctypes.byref(p), None, 0) == INVALID and what in err(), bad
    for bad, what in ((dict(phi_luminance=0.0), "phi_luminance"), (dict(epsilon=float("nan")), "epsilon"), (dict(spatial_radius=4), "spatial_radius")):
        p = product.default_variance_params(**bad)
        assert lib.ptx_denoise_adaptive(None, None, None, None, ctypes.byref(p), 0) == INVALID and what in err(), bad
    assert hasattr(product.Tracer, "denoise_adaptive")


def test_headless_help_names_adaptive_denoise(product):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mygpuraytracer_amd", "csrc"), "headless"])
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--adaptive-denoise" in r.stdout
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    bad = subprocess.run([exe, scene, "--adaptive-denoise"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--adaptive-denoise needs --adaptive" in bad.stderr
    bad = subprocess.run([exe, scene, "--adaptive", "0.1", "--denoise"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--adaptive does not combine" in bad.stderr


def test_adaptive_prep_does_not_spill():
    found = kernels_named(resource_usage("resource-usage-adaptive"), ("k_adaptive_prep",))
    v = found["k_adaptive_prep"]
    print("k_adaptive_prep", v)
    assert v.get("scratch") == 0 and v["lds"] == 0, v
