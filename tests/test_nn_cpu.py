"""CPU: the network denoiser's host side (csrc/pt_tza.h, the ptx_nn_* section of include/mi355x_pathtracer.h) without a device: the
TZA reader and the restatement's writer and reader (tests/unet_ref.py) pinned against the reference's own training/tza.py where the
reference tree exists, the plan's refusals with the tensor they name, the hostile blobs under the sanitizers as a stand-alone program
(tests/tza_check.cpp), the structs, defaults and symbols, and the veneer switch and the driver option in their sources."""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import unet_ref as U
from conftest import ROOT

CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
REF_TZA = "/root/reference/training/tza.py"


@pytest.fixture(scope="module")
def ref_tza():
    """the reference's training/tza.py, imported by path (it stands alone on numpy + struct); skipped where the tree does not exist"""
    if not os.path.exists(REF_TZA):
        pytest.skip("the reference tree is not here")
    spec = importlib.util.spec_from_file_location("reference_training_tza", REF_TZA)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tensors(dtype=np.float32):
    w = U.synthetic_weights(6, 5, dtype=dtype)
    return [(k, v, "oihw" if v.ndim == 4 else "x") for k, v in w.items()]


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_tza_writer_and_reader_are_pinned_against_the_references(product, ref_tza, tmp_path, dtype):
    """a file written by either writer is read identically by the other's reader and by ptx_debug_tza_list"""
    tensors = _tensors(dtype)
    ours = tmp_path / "ours.tza"
    ours.write_bytes(U.write_tza(tensors))
    theirs = tmp_path / "theirs.tza"
    with ref_tza.Writer(str(theirs)) as wr:
        for name, a, layout in tensors:
            wr.write(name, a, layout)
    assert ours.read_bytes() == theirs.read_bytes()                  # the same alignment, table and header: the same file
    for path in (ours, theirs):
        blob = path.read_bytes()
        mine, rd = U.read_tza(blob), ref_tza.Reader(str(path))
        assert len(rd) == len(mine) == len(tensors)
        listed = product.debug_tza_list(blob)
        assert listed == U.table_of(blob) and [t[0] for t in listed] == [t[0] for t in tensors]
        for (name, a, layout), (lname, dims, llayout, code, offset) in zip(tensors, listed):
            ta, tl = rd[name]
            ma, ml, mcode, moffset = mine[name]
            assert tl == ml == llayout == layout and lname == name and dims == a.shape and moffset == offset
            assert code == ("f" if dtype == np.float32 else "h")
            assert np.array_equal(np.asarray(ta), a) and np.array_equal(ma, a) and ta.dtype == ma.dtype == a.dtype


def test_the_restatements_reader_reads_its_writer_and_the_library_lists_it(product):
    for dtype in (np.float32, np.float16):
        tensors = _tensors(dtype)
        blob = U.write_tza(tensors)
        back = U.read_tza(blob)
        assert all(np.array_equal(back[n][0], a) and back[n][1] == l for n, a, l in tensors)
        assert product.debug_tza_list(blob) == U.table_of(blob)
        plan = product.debug_nn_plan(blob)
        assert plan["input_channels"] == 6
        assert plan["layers"] == [(n, sum(ci) if isinstance(ci, tuple) else ci, co) for n, ci, co in U.standard_channels(6)]


@pytest.mark.parametrize("dtype,code", [(np.float32, "f"), (np.float16, "h")])
@pytest.mark.parametrize("counts", [U.NARROW, U.WIDE], ids=["narrow", "wide"])
@pytest.mark.parametrize("ic", [3, 6, 9])
def test_the_plan_accepts_tables_off_the_standard_one(product, ic, counts, dtype, code):
    """channel counts are the blob's: any in 1 .. 256 that follow the graph, in tensors of type f or h; the plan reports them"""
    channels = U.table(ic, *counts)
    blob = U.weights_blob(U.synthetic_weights(ic, 4, channels=channels, dtype=dtype))
    listed = product.debug_tza_list(blob)
    assert listed == U.table_of(blob) and len(listed) == 32 and {t[3] for t in listed} == {code}
    assert [t[1] for t in listed[::2]] == [(co, sum(ci) if isinstance(ci, tuple) else ci, 3, 3) for _, ci, co in channels]
    plan = product.debug_nn_plan(blob)
    assert plan["input_channels"] == ic
    assert plan["layers"] == [(n, sum(ci) if isinstance(ci, tuple) else ci, co) for n, ci, co in channels]
    assert max(co for _, _, co in plan["layers"]) == max(counts)


def test_table_restates_the_standard_channels():
    for ic in (3, 6, 9):
        assert U.table(ic, U.EC1, U.EC2, U.EC3, U.EC4, U.EC5, U.DC4, U.DC3, U.DC2, U.DC1A, U.DC1B) == U.standard_channels(ic)


def _refused(product, weights, match):
    with pytest.raises(product.PathTracerError, match=match):
        product.debug_nn_plan(U.weights_blob(weights))
    lib = product.load_library()
    blob = U.weights_blob(weights)
    out = ctypes.c_void_p(1)
    rc = lib.ptx_nn_create(0, 64, 64, ctypes.cast(ctypes.c_char_p(blob), ctypes.c_void_p), len(blob), ctypes.byref(out))
    assert rc == 1 and out.value is None and match.replace("\\", "") in lib.ptx_last_error().decode()      # PTX_ERR_INVALID before any device work


def test_plan_refusals_name_their_tensor(product):
    good = U.synthetic_weights(3, 1)
    assert product.debug_nn_plan(U.weights_blob(good))["input_channels"] == 3
    w = dict(good); del w["dec_conv2b.bias"]
    _refused(product, w, "'dec_conv2b.bias' is missing")
    w = dict(good); del w["enc_conv3.weight"]
    _refused(product, w, "'enc_conv3.weight' is missing")
    w = dict(good); w["enc_conv1.weight"] = good["enc_conv1.weight"][:, :, :, 0]                  # rank 3
    with pytest.raises(product.PathTracerError, match="'enc_conv1.weight'"):
        product.debug_nn_plan(U.write_tza([(k, v, {4: "oihw", 1: "x", 3: "xxx"}[v.ndim]) for k, v in w.items()]))
    w = dict(good); w["enc_conv1.bias"] = np.zeros((32, 1, 1, 1), np.float32)                      # a bias of rank 4
    _refused(product, w, "'enc_conv1.bias' must have rank 1")
    w = dict(good); w["enc_conv1.weight"] = np.zeros(32 * 32 * 9, np.float32)                      # a weight of rank 1
    _refused(product, w, "'enc_conv1.weight' must have rank 4")
    w = dict(good); w["enc_conv2.weight"] = np.zeros((48, 33, 3, 3), np.float32)                   # Cin does not follow the graph
    _refused(product, w, "'enc_conv2.weight': Cin is 33, the graph feeds it 32")
    w = dict(good); w["dec_conv1a.weight"] = np.zeros((64, 64 + 6, 3, 3), np.float32)              # the skip is the 3-channel input
    _refused(product, w, "'dec_conv1a.weight': Cin is 70, the graph feeds it 67")
    w = dict(good); w["enc_conv1.weight"] = np.zeros((32, 32, 3, 5), np.float32)
    _refused(product, w, "'enc_conv1.weight' must be")
    w = dict(good); w["enc_conv1.bias"] = np.zeros(31, np.float32)
    _refused(product, w, "'enc_conv1.bias' must be")
    w = U.synthetic_weights(3, 1, channels=[(n, 4 if n == "enc_conv0" else ci, co) for n, ci, co in U.standard_channels(3)])
    _refused(product, w, "'enc_conv0.weight': the network takes 3, 6 or 9 input channels, not 4")
    w = U.synthetic_weights(3, 1, channels=[(n, ci, 4 if n == "dec_conv0" else co) for n, ci, co in U.standard_channels(3)])
    _refused(product, w, "'dec_conv0.weight': the network gives 3 output channels, not 4")
    ch = [(n, 257 if n == "enc_conv5b" else ci, 257 if n == "enc_conv5a" else co) for n, ci, co in U.standard_channels(3)]
    _refused(product, U.synthetic_weights(3, 1, channels=ch), "'enc_conv5a.weight': more than 256 channels")
    # a blob that is no blob, and one cut short, name what they can
    with pytest.raises(product.PathTracerError, match="magic"):
        product.debug_tza_list(b"\0" * 64)
    with pytest.raises(product.PathTracerError, match="ends inside|beyond its end"):
        product.debug_tza_list(U.weights_blob(good)[:-7])


def test_hostile_blobs_are_refused_cleanly_under_the_sanitizers(tmp_path):
    """tests/tza_check.cpp with its own main, -fsanitize=address,undefined, run as a program: truncation at every byte, a table offset
    beyond the end, a name length past the end, dims whose product overflows, an offset + size that wraps -- all refused, nothing reported"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "tza_check"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "tza_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "tza_check: 0 failures" in r.stdout and "truncations refused" in r.stdout, r.stdout[-2000:]


def test_nn_structs_defaults_and_symbols(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    header = open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()
    assert "#define PTX_ABI_VERSION 5\n" in header and lib.ptx_abi_version() == api.ABI_VERSION == 5      # additive: the ABI stays
    for name in ("ptx_default_nn_params", "ptx_sizeof_nn_params", "ptx_sizeof_nn_info", "ptx_nn_create", "ptx_nn_create_from_file",
                 "ptx_nn_destroy", "ptx_nn_get_info", "ptx_nn_denoise_device", "ptx_nn_denoise_host", "ptx_nn_read_scale", "ptx_denoise_nn",
                 "ptx_kat_nn_conv", "ptx_kat_nn_transfer", "ptx_debug_tza_list", "ptx_debug_nn_plan"):
        assert hasattr(lib, name) and name + "(" in header, name
    assert lib.ptx_sizeof_nn_params() == ctypes.sizeof(api.NNParams) == 12
    assert lib.ptx_sizeof_nn_info() == ctypes.sizeof(api.NNInfo)
    p = product.default_nn_params()
    assert p.hdr == 0 and p.srgb == 0 and np.isnan(p.input_scale)
    assert product.default_nn_params(hdr=1, input_scale=2.5).input_scale == 2.5
    lib.ptx_nn_destroy(None)                                                                       # NULL is a no-op
    # no device: the refusals that need none come first, then PTX_ERR_NODEVICE, never a CPU path
    blob = U.weights_blob(U.synthetic_weights(3, 1))
    ptr = ctypes.cast(ctypes.c_char_p(blob), ctypes.c_void_p)
    out = ctypes.c_void_p()
    assert lib.ptx_nn_create(0, 7681, 4320, ptr, len(blob), ctypes.byref(out)) == 1 and b"bad frame size" in lib.ptx_last_error()
    assert lib.ptx_nn_create(0, 64, 64, ptr, len(blob), None) == 1
    assert lib.ptx_nn_create_from_file(0, 64, 64, b"/nonexistent/weights.tza", ctypes.byref(out)) == 2
    if lib.ptx_device_count() < 1:
        assert lib.ptx_nn_create(0, 64, 64, ptr, len(blob), ctypes.byref(out)) == 4 and out.value is None
        assert lib.ptx_kat_nn_transfer(0, 1, 1, ptr, None, None, 0, 0, 1.0, 0, ptr) == 4


def test_veneer_switch_and_driver_option_exist():
    veneer_h = open(os.path.join(CSRC, "pathtrace_api.h")).read()
    veneer = open(os.path.join(CSRC, "pathtrace_api.cpp")).read()
    driver = open(os.path.join(CSRC, "main_headless.cpp")).read()
    assert "std::string &nnWeights();" in veneer_h and "ptx_nn_params &nnParams();" in veneer_h
    assert "ptx_denoise_nn(g_tracer, g_nn, &nnParams(), g_last_iter)" in veneer and "ptx_nn_create_from_file(g_device" in veneer
    assert "ptx_nn_destroy(g_nn)" in veneer                                                       # GPUdenoiseRelease frees it
    assert 'a == "--nn"' in driver and 'a == "--nn-hdr"' in driver and "ptx_denoise_nn(t, nn, &nnParams(), n)" in driver
    assert "--nn needs --denoise" in driver
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "pt_nn.o" in makefile and "resource-usage-nn" in makefile and "NNOPT" in makefile
    # the unit under its own optimisation flags, with -ffp-contract=off kept
    line = [l for l in subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/pt_nn.o"], text=True).splitlines() if " -c pt_nn.hip " in l]
    assert len(line) == 1 and " -O3 " in line[0] and "-ffp-contract=off" in line[0] and line[0].index("-O3") > line[0].index("-Os")
    # pt_tza.h is host only
    tza = open(os.path.join(CSRC, "pt_tza.h")).read()
    assert "#include <hip" not in tza and "hipMalloc" not in tza


def test_headless_help_names_the_nn_option(product):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", CSRC, "headless"])
    r = subprocess.run([exe, "scene.txt", "--nn", "w.tza"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "--nn needs --denoise" in r.stderr
    r = subprocess.run([exe, "scene.txt", "--denoise", "--nn-hdr"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "--nn-hdr needs --nn FILE" in r.stderr
