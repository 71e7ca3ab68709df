"""CPU: the host side of the network denoiser's prefiltered guides (the ptx_nn_prefilter_* section of include/mi355x_pathtracer.h,
csrc/pt_nn_aux.hip) without a device: the symbols, structs and defaults, the refusals that need no device, the driver option and the
veneer switch, and the restatement's own pass-through identity (tests/unet_aux_ref.py), which the GPU tests stand on."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import unet_aux_ref as X
import unet_ref as U
from conftest import ROOT

CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
NAMES = ("ptx_default_nn_prefilter_params", "ptx_sizeof_nn_prefilter_params", "ptx_sizeof_nn_prefilter_info", "ptx_nn_prefilter_create",
         "ptx_nn_prefilter_create_from_files", "ptx_nn_prefilter_destroy", "ptx_nn_prefilter_get_info", "ptx_nn_prefilter_run_device",
         "ptx_nn_prefilter_run_host", "ptx_nn_prefilter_device_clean", "ptx_nn_prefilter_read", "ptx_nn_prefilter_invalidate",
         "ptx_denoise_nn_prefiltered", "ptx_kat_nn_transfer_aux", "ptx_debug_nn_prefilter_problem")


def test_symbols_structs_and_defaults(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    header = open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()
    assert "#define PTX_ABI_VERSION 5\n" in header and lib.ptx_abi_version() == api.ABI_VERSION == 5      # additive: the ABI stays
    for name in NAMES:
        assert hasattr(lib, name) and name + "(" in header, name
    assert "#define PTX_NN_AUX_ALBEDO 1\n" in header and "#define PTX_NN_AUX_NORMAL 2\n" in header
    assert (api.NN_AUX_ALBEDO, api.NN_AUX_NORMAL) == (X.ALBEDO, X.NORMAL) == (1, 2)
    assert lib.ptx_sizeof_nn_prefilter_params() == ctypes.sizeof(api.NNPrefilterParams) == 8
    assert lib.ptx_sizeof_nn_prefilter_info() == ctypes.sizeof(api.NNPrefilterInfo) == 16 + 2 * ctypes.sizeof(api.NNInfo) + 16
    # the existing structs are as they were: ptx_nn_params gained no field
    assert lib.ptx_sizeof_nn_params() == ctypes.sizeof(api.NNParams) == 12
    p = product.default_nn_prefilter_params()
    assert p.srgb == 0 and np.isnan(p.input_scale)
    assert product.default_nn_prefilter_params(srgb=1, input_scale=0.5).input_scale == 0.5
    lib.ptx_nn_prefilter_destroy(None)                                                             # NULL is a no-op
    # no device: the refusals that need none come first, then PTX_ERR_NODEVICE, never a CPU path
    blob = U.weights_blob(U.synthetic_weights(3, 1))
    ptr = ctypes.cast(ctypes.c_char_p(blob), ctypes.c_void_p)
    out = ctypes.c_void_p(1)
    assert lib.ptx_nn_prefilter_create(0, 64, 64, None, 0, None, 0, -1, ctypes.byref(out)) == 1 and out.value is None
    assert lib.ptx_nn_prefilter_create(0, 7681, 4320, ptr, len(blob), None, 0, -1, ctypes.byref(out)) == 1 and b"bad frame size" in lib.ptx_last_error()
    assert lib.ptx_nn_prefilter_create(0, 64, 64, ptr, len(blob), None, 0, 0, None) == 1
    assert lib.ptx_nn_prefilter_create_from_files(0, 64, 64, b"/nonexistent/alb.tza", None, -1, ctypes.byref(out)) == 2
    if lib.ptx_device_count() < 1:
        assert lib.ptx_nn_prefilter_create(0, 64, 64, ptr, len(blob), ptr, len(blob), -1, ctypes.byref(out)) == 4 and out.value is None
        assert lib.ptx_kat_nn_transfer_aux(0, 1, 1, 2, ptr, 0, 1.0, 0, ptr) == 4


def test_the_refusals_that_need_no_device(product):
    pt = product
    b3 = U.weights_blob(U.synthetic_weights(3, 1))
    narrow3 = U.weights_blob(U.synthetic_weights(3, 2, channels=U.table(3, *U.NARROW)))
    assert pt.debug_nn_prefilter_problem(b3, None) is None
    assert pt.debug_nn_prefilter_problem(None, narrow3) is None
    assert pt.debug_nn_prefilter_problem(b3, narrow3, srgb=1, input_scale=0.5) is None
    with pytest.raises(pt.PathTracerError, match="no weights"):
        pt.debug_nn_prefilter_problem(None, None)
    for ic in (6, 9):
        bad = U.weights_blob(U.synthetic_weights(ic, 1))
        with pytest.raises(pt.PathTracerError, match="the albedo weights take %d input channels" % ic):
            pt.debug_nn_prefilter_problem(bad, b3)
        with pytest.raises(pt.PathTracerError, match="the normal weights take %d input channels" % ic):
            pt.debug_nn_prefilter_problem(None, bad)
    with pytest.raises(pt.PathTracerError, match="weight blob"):
        pt.debug_nn_prefilter_problem(b3[:100])
    for bad, what in ((dict(srgb=2), "srgb"), (dict(srgb=-1), "srgb"), (dict(input_scale=0.0), "input_scale"), (dict(input_scale=-1.0), "input_scale"),
                      (dict(input_scale=float("inf")), "input_scale")):
        with pytest.raises(pt.PathTracerError, match=what):
            pt.debug_nn_prefilter_problem(b3, b3, **bad)
    with pytest.raises(pt.PathTracerError, match="hdr"):                                           # the RT filter refuses an hdr prefilter: no such field
        pt.debug_nn_prefilter_problem(b3, b3, hdr=1)


def test_driver_and_veneer_refuse_the_prefilter_without_the_network(product):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", CSRC, "headless"])
    for opt in ("--nn-albedo", "--nn-normal"):
        r = subprocess.run([exe, "scene.txt", "--denoise", opt, "w.tza"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 1 and opt + " needs --nn FILE" in r.stderr, (opt, r.stderr)
    veneer_h = open(os.path.join(CSRC, "pathtrace_api.h")).read()
    veneer = open(os.path.join(CSRC, "pathtrace_api.cpp")).read()
    driver = open(os.path.join(CSRC, "main_headless.cpp")).read()
    assert "std::string &nnAlbedoWeights();" in veneer_h and "std::string &nnNormalWeights();" in veneer_h
    assert "if (nnWeights().empty() && (!nnAlbedoWeights().empty() || !nnNormalWeights().empty())) {" in veneer and "they need nnWeights()" in veneer
    assert "ptx_denoise_nn_prefiltered(g_tracer, g_nn, g_nn_pf, &nnParams(), &nnPrefilterParams(), g_last_iter)" in veneer
    assert "ptx_nn_prefilter_destroy(g_nn_pf)" in veneer                                          # GPUdenoiseRelease frees it
    assert "nnMaxMemoryMB(), &g_nn_pf)" in veneer                                                  # the memory limit is the prefilter's too
    assert "ptx_denoise_nn_prefiltered(t, nn, pf, &nnParams(), nullptr, n)" in driver and "ptx_nn_prefilter_destroy(pf)" in driver
    # the unit under the network unit's flags, with -ffp-contract=off kept
    line = [l for l in subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/pt_nn_aux.o"], text=True).splitlines() if " -c pt_nn_aux.hip " in l]
    assert len(line) == 1 and " -O3 " in line[0] and "-ffp-contract=off" in line[0] and line[0].index("-O3") > line[0].index("-Os")


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("ic,pick", [(3, (0, 1, 2)), (9, (3, 4, 5)), (9, (6, 7, 8)), (9, (8, 0, 4))])
def test_the_pass_through_identity_holds_in_the_restatement(ic, pick, dtype_name):
    """a pass-through blob gives fp16(g * fp16(x)) of the three chosen channels, with zero unequal values: what the GPU tests read a
    network's input from.  Frames of one pixel, of no multiple of 16 each way, in the standard table and in NARROW."""
    rng = np.random.default_rng(7 * ic + pick[0])
    for (w, h), g, channels in (((1, 1), 1.0, None), ((33, 17), 0.5, None), ((38, 22), 1.0, None), ((33, 17), 0.5, U.table(ic, *U.NARROW))):
        x = rng.random((h, w, ic), dtype=np.float32)
        x[0, 0, pick[0]] = 0.0
        x[-1, -1, pick[1]] = 1.0
        weights = X.passthrough_weights(ic, pick, g, channels)
        assert U.read_tza(U.weights_blob(weights))["dec_conv1a.weight"][0].shape[1] == sum(dict((n, c) for n, c, _ in channels or U.standard_channels(ic))["dec_conv1a"])
        got = U.unet(x, weights, dtype_name)
        want = X.passthrough(x[..., list(pick)], g)
        assert got.shape == want.shape and int((got != want.astype(np.float64)).sum()) == 0, (w, h, g)


def test_the_float32_transforms_are_the_float64_ones_where_those_are_exact():
    """the step-for-step float32 restatement against the float64 one: the clamps, the special values and the sign of zero"""
    f = np.float32
    v = np.array([np.nan, np.inf, -np.inf, 3, -3, 1, -1, 0.0, -0.0, 0.25, -0.75, 1e-30], f).reshape(2, 2, 3)
    n_in = X.aux_input_f32(v, X.NORMAL)
    assert np.array_equal(n_in.astype(np.float64), X.aux_input(v, X.NORMAL)) and n_in.dtype == f
    assert n_in.reshape(-1)[:9].tolist() == [0.5, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.5, 0.5]
    a_in = X.aux_input_f32(v, X.ALBEDO, srgb=1)
    assert np.array_equal(a_in.astype(np.float64), X.aux_input(v, X.ALBEDO, srgb=1)) and not np.signbit(a_in).any()
    n_out = X.aux_output_f32(v, X.NORMAL)
    assert np.array_equal(n_out.astype(np.float64), X.aux_output(v, X.NORMAL))
    assert n_out.reshape(-1)[:9].tolist() == [-1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, -1.0, -1.0]
    a_out = X.aux_output_f32(v, X.ALBEDO, srgb=1, scale=0.5)
    assert np.array_equal(a_out.astype(np.float64), X.aux_output(v, X.ALBEDO, srgb=1, scale=0.5)) and a_out.max() == 2.0
