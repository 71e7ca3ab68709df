"""CPU: the definition of adaptive sampling by tiles (tests/adaptive_ref.py on synthetic iid samples), its C-ABI surface without a
device, and what the compiler made of its kernels.  The device is held to the same restatement by tests/test_gpu_adaptive.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from adaptive_ref import TiledMoments, decide, num_tiles, pixel_rel, resolve, status, tile_error, tile_of, tile_sizes
from moments_ref import LUM, Moments, quad
from resource_usage import kernels_named, resource_usage

SIZES = (0, 1, 2, 5, 12, 40)         # tests/test_moments_cpu.py's batch sizes, and 0: the tile is idle in that add


def test_tiled_add_is_moments_ref_on_each_tile_with_its_own_sequence():
    """a 5 x 13 frame in tiles of 8 pixels (the last one of 1): after every add the state equals, tile by tile, a moments_ref.Moments of
    that tile's pixels fed only the adds in which the tile advanced"""
    rng = np.random.default_rng(5)
    h, w, tp = 5, 13, 8
    n = num_tiles(h, w, tp)
    assert n == 9 and tile_sizes(h, w, tp).tolist() == [8] * 8 + [1]
    tile = tile_of(h, w, tp).ravel()
    t = TiledMoments(h, w, tp)
    own = [Moments(1, int(s)) for s in tile_sizes(h, w, tp)]
    acc, total = np.zeros((h * w, 3)), np.zeros(n, np.int64)
    for _ in range(9):
        ks = rng.choice(SIZES, n)
        acc = acc + ks[tile][:, None] * rng.random((h * w, 3))
        total = total + ks
        t.add(acc, total)
        for i in range(n):
            if ks[i]:
                own[i].add(acc[tile == i], int(total[i]))
        assert (t.W == [m.W for m in own]).all() and (t.B == [m.B for m in own]).all()
        mean, cov = t.mean.reshape(-1, 3), t.cov().reshape(-1, 3, 3)
        for i in range(n):
            assert np.array_equal(mean[tile == i], own[i].mean[0]) and np.array_equal(cov[tile == i], own[i].cov()[0])
    assert len(set(t.W.tolist())) > 1 and (t.W_pixels().ravel() == t.W[tile]).all()


def test_batch_means_stay_unbiased_under_per_tile_schedules():
    """tests/test_moments_cpu.py's check with every tile on a schedule of its own, idle adds included: 16 tiles of 256 pixels, 12 adds,
    64 sequences pooled.  The mean of C is the samples' covariance and the mean of g^T C g / W (W the pixel's own) the squared error of
    the pixel's mean luminance, both within 2 %."""
    rng = np.random.default_rng(20240608)
    tp, tiles, runs = 256, 16, 64
    P = tp * tiles
    mu = np.array([0.8, 0.5, 0.3])
    L = np.array([[0.5, 0.0, 0.0], [0.3, 0.4, 0.0], [0.2, 0.1, 0.3]])
    cov = L @ L.T
    Csum, pred, err2, used = np.zeros((3, 3)), 0.0, 0.0, set()
    for _ in range(runs):
        m = TiledMoments(1, P, tp)
        acc, total = np.zeros((P, 3)), np.zeros(tiles, np.int64)
        for _ in range(12):
            ks = rng.choice(SIZES, tiles)
            used.update(int(k) for k in ks)
            for t in np.flatnonzero(ks):
                acc[t * tp:(t + 1) * tp] += (mu + rng.standard_normal((tp, int(ks[t]), 3)) @ L.T).sum(1)
            total = total + ks
            m.add(acc, total)
        assert (m.B >= 2).all() and (m.W == total).all() and len(set(total.tolist())) > 1
        C = m.cov()
        Csum += C.mean((0, 1))
        pred += (quad(C, LUM) / m.W_pixels()).mean()
        err2 += (((m.mean - mu) @ LUM) ** 2).mean()
    Cbar = Csum / runs
    print("mean C / truth:\n%s\nmean g^T C g / W %.6g, squared error of the mean %.6g (ratio %.4f)" % (Cbar / cov, pred / runs, err2 / runs, pred / err2))
    assert used == set(SIZES)
    assert (np.abs(Cbar - cov) <= 0.02 * np.abs(cov)).all()
    assert abs(pred - err2) <= 0.02 * err2


def test_tile_error_and_the_decision_rule_by_hand():
    # 2 x 5 in tiles of 4: tiles of 4, 4 and 2 pixels; rel = 0.3 on tile 0, no estimate on tile 1, (0.1, no estimate) on tile 2
    rel = np.array([[0.3, 0.3, 0.3, 0.3, np.nan], [np.nan, np.nan, np.nan, 0.1, np.nan]])
    e, has = tile_error(rel, 4)
    assert has.tolist() == [True, False, True] and np.allclose(e, [0.3, 0.0, np.sqrt(0.01 / 2)])      # n_T counts the pixel without one
    # the rule: below min_batches active whatever the error; then active while e > target (equal stops); max_samples ends it either way
    f = lambda s, b, err: bool(decide([s], [b], [err], target=0.05, min_batches=4, max_samples=64)[0])
    assert f(8, 3, 0.0) and f(8, 3, 1.0)
    assert not f(8, 4, 0.05) and not f(8, 4, 0.0) and f(8, 4, np.nextafter(0.05, 1))
    assert not f(64, 1, 1.0) and not f(65, 9, 1.0) and f(63, 9, 1.0)
    st = status([8, 64, 3], [True, False, True], e, has, 2, 5, 4, rounds=7)
    assert st == dict(samples_total=8 * 4 + 64 * 4 + 3 * 2, pixels_active=6, tiles=3, tiles_active=2, samples_min=3, samples_max=64,
                      worst_error=float(e[0]), rounds=7)
    # per-pixel rel is the summary's, with the pixel's own W
    m = Moments(1, 2)
    a1 = np.array([[[4.0, 2.0, 0.0], [1.0, 1.0, 1.0]]])
    m.add(a1, 4)
    assert np.isnan(pixel_rel(m.mean, m.cov(), m.B, m.W)).all()
    m.add(3 * a1, 8)
    want = np.sqrt(quad(m.cov(), LUM) / np.array([[8, 2]])) / np.maximum(m.mean @ LUM, 0.05)
    assert np.allclose(pixel_rel(m.mean, m.cov(), m.B, np.array([[8, 2]])), want)
    # resolve: fp32 division by the tile's count, 0 where that is 0
    acc = np.arange(30, dtype=np.float32).reshape(2, 5, 3)
    r = resolve(acc, [3, 0, 7], 2, 5, 4)
    assert r.dtype == np.float32 and not r.reshape(-1, 3)[4:8].any()
    assert np.array_equal(r.reshape(-1, 3)[:4], acc.reshape(-1, 3)[:4] / np.float32(3)) and np.array_equal(r.reshape(-1, 3)[8:], acc.reshape(-1, 3)[8:] / np.float32(7))


def test_adaptive_structs_defaults_and_symbols(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    header = open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()
    for name in ("ptx_tile_pixels", "ptx_num_tiles", "ptx_set_active_tiles", "ptx_clear_active_tiles", "ptx_moments_add_host_tiled",
                 "ptx_moments_read_samples", "ptx_default_adaptive_params", "ptx_sizeof_adaptive_params", "ptx_sizeof_adaptive_status",
                 "ptx_adaptive_create", "ptx_adaptive_destroy", "ptx_adaptive_reset", "ptx_adaptive_num_tiles", "ptx_adaptive_add",
                 "ptx_adaptive_select", "ptx_adaptive_resolve", "ptx_adaptive_read", "ptx_adaptive_device_frame"):
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
    assert lib.ptx_sizeof_adaptive_params() == ctypes.sizeof(api.AdaptiveParams) == 16
    assert lib.ptx_sizeof_adaptive_status() == ctypes.sizeof(api.AdaptiveStatus) == 40
    p = product.default_adaptive_params()
    assert (p.target, p.floor, p.min_batches, p.max_samples) == (float(np.float32(0.02)), float(np.float32(0.05)), 4, 1 << 20)
    assert product.default_adaptive_params(target=0.5, min_batches=9).min_batches == 9
    with pytest.raises(AttributeError):
        product.default_adaptive_params(bogus=1)
    assert product.tile_pixels() == lib.ptx_tile_pixels() > 0
    assert lib.ptx_abi_version() == 5                    # no existing struct or entry point changed


def test_bad_adaptive_arguments_are_refused_before_any_device_work(product):
    lib = product.load_library()
    err = lambda: lib.ptx_last_error().decode()
    INVALID = 1
    out = ctypes.c_void_p()
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 16)):
        assert lib.ptx_adaptive_create(0, w, h, ctypes.byref(out)) == INVALID and "frame size" in err(), (w, h)
    assert lib.ptx_adaptive_create(0, 4, 4, None) == INVALID and "NULL" in err()
    assert lib.ptx_adaptive_create(-1, 4, 4, ctypes.byref(out)) == INVALID and "device" in err()
    assert not out.value
    if lib.ptx_device_count() < 1:                       # and with good arguments there is no CPU path
        assert lib.ptx_adaptive_create(0, 4, 4, ctypes.byref(out)) == 4 and "no HIP device" in err()
    assert lib.ptx_adaptive_reset(None) == INVALID and "null" in err()
    lib.ptx_adaptive_destroy(None)                       # a no-op
    assert lib.ptx_adaptive_read(None, None, None, None, None) == INVALID and "null" in err()
    assert lib.ptx_adaptive_add(None, None, None, 0) == INVALID and "k must" in err()
    assert lib.ptx_adaptive_add(None, None, None, 1) == INVALID and "null" in err()
    assert lib.ptx_adaptive_resolve(None, None) == INVALID and "null" in err()
    st = product.AdaptiveStatus()
    for bad, what in ((dict(target=0.0), "target"), (dict(target=float("nan")), "target"), (dict(floor=0.0), "floor"),
                      (dict(min_batches=1), "min_batches"), (dict(max_samples=0), "max_samples")):
        p = product.default_adaptive_params(**bad)
        assert lib.ptx_adaptive_select(None, None, None, ctypes.byref(p), ctypes.byref(st)) == INVALID and what in err(), bad
    assert lib.ptx_adaptive_select(None, None, None, None, ctypes.byref(st)) == INVALID and "null" in err()
    z = np.zeros(3, np.float32)
    assert lib.ptx_moments_add_host_tiled(None, z.ctypes.data_as(ctypes.c_void_p), None, 1) == INVALID and "null" in err()
    assert lib.ptx_set_active_tiles(None, None, 1) == INVALID and lib.ptx_clear_active_tiles(None) == INVALID and lib.ptx_num_tiles(None) == 0


def test_headless_help_names_adaptive(product):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mygpuraytracer_amd", "csrc"), "headless"])
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--adaptive E" in r.stdout and "--until-error" in r.stdout
    bad = subprocess.run([exe, os.path.join(ROOT, "scenes", "cornell.txt"), "--adaptive", "0"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "E > 0" in bad.stderr


def test_adaptive_kernels_do_not_spill():
    found = kernels_named(resource_usage("resource-usage-adaptive"), ("k_adaptive_advance", "k_adaptive_select", "k_adaptive_status", "k_adaptive_resolve"))
    found.update(kernels_named(resource_usage("resource-usage-moments"), ("k_moments_add_tiled",)))
    assert len(found) == 5, list(found)
    for k, v in found.items():
        assert v.get("scratch") == 0, (k, v)
        print(k, v)
    assert found["k_moments_add_tiled"]["lds"] == 0 and found["k_adaptive_resolve"]["lds"] == 0
