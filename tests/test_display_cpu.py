"""CPU: the display transform's definition (tests/display_ref.py) against the reference's own preview bytes, the meter's block grid as
the library computes it on the host, and the C-ABI surface of ptx_display_* (include/mi355x_pathtracer.h)."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import display_ref as dr
from conftest import GOLDEN, ROOT

SIZES = ((1, 1), (7, 7), (8, 8), (23, 23), (24, 8), (37, 23), (97, 61), (1920, 1080), (3840, 2160))


def test_the_reference_setting_is_the_reference_preview_on_every_golden_frame():
    """meter MANUAL, exposure 1, tone CLAMP, transfer LINEAR, quantize 0 reproduces sendImageToPBO's bytes (pbo_spp*, written by the
    reference itself) from the accumulation buffer of the same fixture: the property that ties the new path to the old one"""
    seen = 0
    for path in sorted(glob.glob(os.path.join(GOLDEN, "render_*.npz"))):
        g = np.load(path)
        for key in g.files:
            m = re.fullmatch(r"pbo_spp(\d+)", key)
            if not m:
                continue
            spp = int(m.group(1))
            img = g["image_spp%d" % spp]
            codes = dr.reference_setting_codes(img, spp, len(img), 1).reshape(-1, 4)
            assert np.array_equal(codes, g[key]), (path, key)
            # and through the general quantiser from an fp32 z
            z = dr.display(img, spp, 1.0, dr.TONE_CLAMP, dr.TRANSFER_LINEAR).astype(np.float32)
            assert np.array_equal(dr.quantise(z, len(img), 1, quantize=0).reshape(-1, 4), g[key]), (path, key)
            seen += 1
    assert seen == 8


def test_the_bayer_thresholds_are_exact_in_fp32_and_a_permutation():
    assert sorted(dr.BAYER8.ravel().tolist()) == list(range(64))
    t = (2 * dr.BAYER8 + 1) / 128.0
    assert np.array_equal(t.astype(np.float32).astype(np.float64), t) and t.min() > 0 and t.max() < 1
    # the recursive definition: B(x, y) interleaves the bits of x ^ y and y, most significant pair from bit 0
    for y in range(8):
        for x in range(8):
            a = x ^ y
            want = ((a & 1) << 5) | ((y & 1) << 4) | ((a & 2) << 2) | ((y & 2) << 1) | ((a & 4) >> 1) | ((y & 4) >> 2)
            assert dr.BAYER8[y, x] == want, (x, y)


@pytest.mark.parametrize("w,h", SIZES)
def test_block_grid_is_the_integer_formula(product, w, h):
    rows, cols = product.api.debug_display_blocks(w, h)
    hk, wk = (h + 8) // 16, (w + 8) // 16
    if hk == 0 or wk == 0:
        assert len(rows) == 0 and len(cols) == 0
        assert dr.block_grid(w, h) == ([], [])
        return
    assert rows.tolist() == [i * h // hk for i in range(hk + 1)] == dr.block_grid(w, h)[0]
    assert cols.tolist() == [j * w // wk for j in range(wk + 1)] == dr.block_grid(w, h)[1]
    for begin, end in ((rows, h), (cols, w)):
        d = np.diff(begin.astype(np.int64))
        assert begin[0] == 0 and begin[-1] == end and (d > 0).all() and d.max() <= 23, (w, h, d.max())


def test_no_blocks_below_eight_pixels_and_bad_sizes_are_refused(product):
    lib = product.load_library()
    hk, wk = ctypes.c_int(-1), ctypes.c_int(-1)
    for w, h in ((7, 100), (100, 7), (1, 1)):
        assert lib.ptx_debug_display_blocks(w, h, ctypes.byref(hk), ctypes.byref(wk), None, None) == 0 and (hk.value, wk.value) == (0, 0)
    assert lib.ptx_debug_display_blocks(0, 4, ctypes.byref(hk), ctypes.byref(wk), None, None) == 1
    assert lib.ptx_debug_display_blocks(4, 4, None, None, None, None) == 1


def test_the_meter_of_the_restatement_by_hand():
    # 16 x 16: one block; luminance 0.5 everywhere -> metered = 0.18 / 0.5
    img = np.full((16 * 16, 3), 0.5, np.float32)
    b = dr.block_means(img, 1, 16, 16)
    assert b.shape == (1, 1) and abs(b[0, 0] - 0.5) < 1e-12
    m = dr.meter(b)
    assert abs(m["metered"] - float(np.float32(0.18)) / 0.5) < 1e-12 and m["blocks_used"] == m["blocks_total"] == 1
    # a black frame and a frame without blocks meter 1
    assert dr.meter(dr.block_means(np.zeros((256, 3), np.float32), 1, 16, 16))["metered"] == 1.0
    assert dr.meter(dr.block_means(img[:49], 1, 7, 7)) == dict(metered=1.0, log2_mean=0.0, blocks_used=0, blocks_total=0)
    # sanitise: NaN, negative, inf, 1e30
    c = dr.sanitise(np.array([[np.nan, -1.0, np.inf], [1e30, 2.0, 0.0]], np.float32), 2)
    assert c.tolist() == [[0.0, 0.0, 65504.0], [65504.0, 1.0, 0.0]]
    # adaptation: half the way in log2
    assert abs(dr.adapt(1.0, 16.0, 0.5) - 4.0) < 1e-12 and abs(dr.adapt(3.0, 5.0, 1.0) - 5.0) < 1e-12
    # curves at a few points
    assert dr.tone(np.array([[0.0, 1e9, 0.5]]), dr.TONE_ACES).tolist()[0][:2] == [0.0, 1.0]
    x = np.array([[4.0, 4.0, 4.0]])
    assert np.allclose(dr.tone(x, dr.TONE_REINHARD, white=4.0), 1.0) and np.allclose(dr.tone(x / 4, dr.TONE_REINHARD, 4.0), (1 + 1 / 16) / 2)
    assert np.allclose(dr.transfer(np.array([0.0, 0.0031308, 1.0]), dr.TRANSFER_SRGB), [0.0, 12.92 * 0.0031308, 1.0])


def test_display_structs_defaults_and_symbols(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    header = open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()
    for name in ("ptx_default_display_params", "ptx_display_create", "ptx_display_destroy", "ptx_display_reset", "ptx_display_tracer",
                 "ptx_display_device", "ptx_display_host", "ptx_display_read", "ptx_display_read_blocks", "ptx_display_get_status",
                 "ptx_debug_display_blocks"):
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("PTX_METER_MANUAL", "PTX_METER_BLOCKS", "PTX_TONE_CLAMP", "PTX_TONE_REINHARD", "PTX_TONE_ACES", "PTX_TRANSFER_LINEAR",
                 "PTX_TRANSFER_SRGB", "PTX_DISPLAY_IMAGE", "PTX_DISPLAY_DENOISED"):
        m = re.search(r"#define %s (\d+)" % name, header)
        assert m and int(m.group(1)) == getattr(api, name[4:]), name
    assert lib.ptx_sizeof_display_params() == ctypes.sizeof(api.DisplayParams) == 40
    assert lib.ptx_sizeof_display_status() == ctypes.sizeof(api.DisplayStatus) == 32
    p = product.default_display_params()
    assert (p.meter, p.exposure, p.key, p.adapt, p.tone, p.white, p.transfer, p.quantize, p.dither, p.keep_float) == (
        api.METER_BLOCKS, 1.0, float(np.float32(0.18)), 1.0, api.TONE_ACES, 4.0, api.TRANSFER_SRGB, 1, 0, 0)
    q = product.default_display_params(tone="reinhard", transfer="linear", meter="manual", exposure=2.5)
    assert (q.tone, q.transfer, q.meter, q.exposure) == (api.TONE_REINHARD, api.TRANSFER_LINEAR, api.METER_MANUAL, 2.5)
    with pytest.raises(AttributeError):
        product.default_display_params(bogus=1)
    assert re.search(r"#define PTX_ABI_VERSION 5\b", header) and lib.ptx_abi_version() == 5      # additive: nothing existing changed


def test_bad_display_arguments_are_refused_before_any_device_work(product):
    lib = product.load_library()
    err = lambda: lib.ptx_last_error().decode()
    INVALID, NODEVICE = 1, 4
    out = ctypes.c_void_p()
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 16)):
        assert lib.ptx_display_create(0, w, h, ctypes.byref(out)) == INVALID and "frame size" in err(), (w, h)
    assert lib.ptx_display_create(0, 4, 4, None) == INVALID and "NULL" in err()
    assert lib.ptx_display_create(-1, 4, 4, ctypes.byref(out)) == INVALID and "device" in err()
    assert not out.value
    if lib.ptx_device_count() < 1:                       # with good arguments there is no CPU path
        assert lib.ptx_display_create(0, 4, 4, ctypes.byref(out)) == NODEVICE and "no HIP device" in err()
        assert not out.value
    assert lib.ptx_display_reset(None) == INVALID and "null" in err()
    lib.ptx_display_destroy(None)                        # a no-op
    assert lib.ptx_display_read(None, None, None) == INVALID and "null" in err()
    assert lib.ptx_display_read_blocks(None, None) == INVALID and "null" in err()
    assert lib.ptx_display_get_status(None, None) == INVALID and "null" in err()
    nan = float("nan")
    for bad, what in ((dict(meter=2), "meter"), (dict(tone=3), "tone"), (dict(tone=-1), "tone"), (dict(transfer=2), "transfer"),
                      (dict(quantize=2), "quantize"), (dict(adapt=0.0), "adapt"), (dict(adapt=1.5), "adapt"), (dict(adapt=nan), "adapt"),
                      (dict(key=0.0), "key"), (dict(key=-1.0), "key"), (dict(white=0.0), "white"), (dict(exposure=0.0), "exposure"),
                      (dict(exposure=nan), "exposure")):
        p = product.default_display_params(**bad)
        assert lib.ptx_display_device(None, None, 1.0, ctypes.byref(p), None, None) == INVALID and what in err(), bad
        assert lib.ptx_display_host(None, None, 1.0, ctypes.byref(p), None) == INVALID and what in err(), bad
        assert lib.ptx_display_tracer(None, None, 0, 1, ctypes.byref(p), None) == INVALID and what in err(), bad
    for samples in (0.0, -2.0, nan):
        assert lib.ptx_display_device(None, None, samples, None, None, None) == INVALID and "samples" in err(), samples
    assert lib.ptx_display_tracer(None, None, 0, 0, None, None) == INVALID and "spp" in err()
    assert lib.ptx_display_tracer(None, None, 7, 1, None, None) == INVALID and "source" in err()
    assert lib.ptx_display_device(None, None, 1.0, None, None, None) == INVALID and "null" in err()
    assert lib.ptx_display_tracer(None, None, 1, 0, None, None) == INVALID and "null" in err()      # denoised: spp is not read


def test_headless_help_names_the_display_flags(product):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mygpuraytracer_amd", "csrc"), "headless"])
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("--tonemap clamp|reinhard|aces", "--exposure auto|<scale>", "--srgb", "--dither", "--adapt A"):
        assert flag in r.stdout, flag
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    for args, what in ((["--tonemap", "filmic"], "--tonemap"), (["--exposure", "0"], "--exposure"), (["--adapt", "2"], "--adapt")):
        bad = subprocess.run([exe, scene] + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and what in bad.stderr, (args, bad.stderr)
