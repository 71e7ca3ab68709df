"""CPU: the lightmap filter without a device (csrc/pt_nn_lightmap.hip, "lightmap" in include/mi355x_pathtracer.h): the entry points and
the header; every refusal of ptx_nn_denoise_lightmap_host that comes before any device call, by name; the two constants of the Log
transfer function, bit for bit; the directional mode's restatement against the normal role's (tests/unet_aux_ref.py), bit for bit on a
sweep that holds NaN, +-inf, +-0 and values beyond +-1; the float32 and float64 restatements of the HDR mode against each other; the
unit's flags."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import nn_lightmap_ref as LM
import unet_aux_ref as X
from conftest import ROOT

CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
W, H = 7, 5


def check_refusals(pt):
    """ptx_nn_denoise_lightmap_host without a handle: the two scalars and the formats are refused first, each by name"""
    a32, a16 = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float16)
    lib = pt.load_library()

    def call(color=a32, output=a32, directional=0, input_scale=float("nan")):
        descs = [a if isinstance(a, pt.NNImage) else pt.nn_image_of(a) for a in (color, output)]
        rc = lib.ptx_nn_denoise_lightmap_host(None, ctypes.byref(descs[0]), ctypes.byref(descs[1]), int(directional), float(input_scale))
        return rc, lib.ptx_last_error().decode()

    bad = lambda a: pt.NNImage(ctypes.c_void_p(a.ctypes.data), 7, 0, 0, 0)
    for kw, text in ((dict(directional=2), "directional must be 0"), (dict(directional=-1), "directional must be 0"),
                     (dict(input_scale=0.0), "input_scale must be NaN (automatic) or finite and > 0"), (dict(input_scale=-1.0), "input_scale must be"),
                     (dict(input_scale=float("inf")), "input_scale must be"), (dict(directional=1, input_scale=0.0), "input_scale must be"),
                     (dict(output=bad(a32)), "the output image: unknown format 7"), (dict(color=bad(a32)), "the colour image: unknown format 7"),
                     (dict(), "null handle"), (dict(color=a16), "null handle"), (dict(directional=1, input_scale=0.37, output=a16), "null handle")):
        rc, msg = call(**kw)
        assert rc == 1 and text in msg and msg.startswith("ptx_nn_denoise_lightmap_host: "), (kw, rc, msg)
    rc = lib.ptx_nn_denoise_lightmap_device(None, None, None, 0, float("nan"), None)
    assert rc == 1 and lib.ptx_last_error().decode().startswith("ptx_nn_denoise_lightmap_device: null handle")
    assert lib.ptx_nn_set_progress(None, pt.api.NN_PROGRESS_FN(), None) == 1 and "null handle" in lib.ptx_last_error().decode()


def test_symbols_and_the_header(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    header = open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()
    assert "#define PTX_ABI_VERSION 5\n" in header and lib.ptx_abi_version() == api.ABI_VERSION == 5      # additive: the ABI stays
    for name in ("ptx_nn_denoise_lightmap_device", "ptx_nn_denoise_lightmap_host", "ptx_debug_nn_lightmap_constants", "ptx_nn_set_progress"):
        assert hasattr(lib, name) and name + "(" in header, name
    assert "#define PTX_ERR_CANCELLED 6 " in header and api.PTX_ERR_CANCELLED == 6
    assert "PTX_NN_ROLE_NORMAL's arithmetic to the bit" in header
    assert issubclass(product.Cancelled, product.PathTracerError)
    assert api.NN_ROLES == {"color": 0, "albedo": 1, "normal": 2}                                         # the lightmap is no role
    for name in ("lightmap_host", "lightmap_device", "set_progress"):
        assert callable(getattr(product.NN, name))


def test_the_refusals_that_come_before_any_device_call(product):
    check_refusals(product)


def test_none_of_it_touches_a_device(product):
    """the same refusals in a process where no device is visible"""
    import sys
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    code = ("import mygpuraytracer_amd as pt, test_nn_lightmap_cpu as T\n"
            "assert pt.load_library().ptx_device_count() == 0\n"
            "T.check_refusals(pt)\n"
            "print('no device: ok')\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "no device: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_the_two_constants_bit_for_bit(product):
    """xmax = (float)log(65505.0) = 0x1.62e050p+3, norm = (float)(1.0 / (double)xmax) = 0x1.71587ep-4: the library's, the restatement's"""
    xmax, norm = ctypes.c_float(), ctypes.c_float()
    product.load_library().ptx_debug_nn_lightmap_constants(ctypes.byref(xmax), ctypes.byref(norm))
    assert float(xmax.value).hex() == "0x1.62e0500000000p+3" and float(norm.value).hex() == "0x1.71587e0000000p-4"
    assert LM.LOG_XMAX == xmax.value and LM.LOG_NORM == norm.value
    assert float.fromhex("0x1.62e050p+3") == xmax.value and float.fromhex("0x1.71587ep-4") == norm.value


def _sweep():
    f = np.float32
    special = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 3e38, -3e38, 1e-45, -1e-45, 0.5, -0.5, 2.0 ** -24, 65504.0, 70000.0], f)
    near = np.concatenate([np.nextafter(special[5:9], f(np.inf)), np.nextafter(special[5:9], f(-np.inf))])
    rng = np.random.default_rng(3)
    v = np.concatenate([special, near, (rng.standard_normal(4000) * 1.2).astype(f), np.linspace(-2, 2, 2000).astype(f)])
    return np.resize(v, (v.size // 3, 1, 3)).astype(f)


def test_directional_is_the_normal_roles_restatement_bit_for_bit():
    v = _sweep()
    assert np.isnan(v).any() and np.isinf(v).any() and (np.abs(v[np.isfinite(v)]) > 1).any() and np.signbit(v[v == 0]).any()
    for scale in (1.0, 0.37, 2.5):
        a, b = LM.input_f32(v, True, scale), X.aux_input_f32(v, X.NORMAL, 0, scale)
        assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes(), scale
        # the network's output: anything, the same sweep shifted into and beyond [0, 1]
        net = (v * np.float32(0.75) + np.float32(0.5)).astype(np.float32)
        a, b = LM.output_f32(net, True, scale), X.aux_output_f32(net, X.NORMAL, 0, scale)
        assert a.tobytes() == b.tobytes(), scale
        with np.errstate(all="ignore"):
            assert np.array_equal(LM.input_f64(v, True, scale), X.aux_input(v, X.NORMAL, 0, scale))
            assert np.array_equal(LM.output_f64(net, True, scale), X.aux_output(net, X.NORMAL, 0, scale))


def test_hdr_restatements_agree_and_sanitise():
    """float32 against float64 within a few ulp and the rounding of v + 1 on [0, 65504]; NaN and negatives are exactly 0; 65504 maps to 1 and back"""
    f = np.float32
    y = np.concatenate([[0.0, 65504.0, 1.0, 2.0 ** -24, 2.0 ** -25], 10.0 ** np.linspace(-9, 4.8, 500)]).astype(f).reshape(-1, 1, 1).repeat(3, 2)
    for scale in (1.0, 0.25):
        x32, x64 = LM.input_f32(y, False, scale).astype(np.float64), LM.input_f64(y, False, scale)
        # float32: v + 1 is rounded (2^-24 of a value >= 1, so 2^-24 absolute in the logarithm), then logf and the product (2^-22 relative)
        assert (np.abs(x32 - x64) <= 2.0 ** -22 * np.abs(x64) + 2.0 ** -24).all()
        back = LM.output_f64(x64, False, scale)
        # there and back: norm * xmax is 1 to within 2^-23, times the exponent (up to 11.09), and v + 1 was rounded: 2^-19 of y + 1
        assert (np.abs(back - y) <= 2.0 ** -19 * (y + 1)).all()
    assert abs(LM.input_f64(np.full((1, 1, 3), 65504.0, f), False)[0, 0, 0] - 1.0) < 2.0 ** -23
    bad = np.asarray([np.nan, -1.0, -np.inf, -0.0, 0.0, 2.0 ** -25], f).reshape(2, 1, 3)
    assert (LM.input_f32(bad, False) == 0).all() and (LM.input_f64(bad, False)[..., :2] == 0).all()
    assert (LM.output_f32(np.asarray([np.nan, -3.0, 0.0], f).reshape(1, 1, 3), False, 0.5) == 0).all()
    assert np.isfinite(LM.input_f32(np.full((1, 1, 3), np.inf, f), False)).all()                    # clamped to FLT_MAX first


def test_the_unit_is_built_under_the_network_units_flags():
    line = [l for l in subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/pt_nn_lightmap.o"], text=True).splitlines() if " -c pt_nn_lightmap.hip " in l]
    assert len(line) == 1 and " -O3 " in line[0] and "-ffp-contract=off" in line[0] and line[0].index("-O3") > line[0].index("-Os")
    unit = open(os.path.join(CSRC, "pt_nn_lightmap.hip")).read()
    assert '#include "pt_nn_image_dev.h"' in unit and "pt_nn_run_tiles(n, st, stages)" in unit
    for word in ("__shared__", "atomic", "transfer_forward(", "transfer_inverse("):
        assert word not in unit.split("#include <hip/hip_runtime.h>")[1], word
    transfer = open(os.path.join(CSRC, "pt_nn_transfer.h")).read()
    assert "log_forward" not in transfer and "65505" not in transfer                                # the Log functions are the new unit's own
