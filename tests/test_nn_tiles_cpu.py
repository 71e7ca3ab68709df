"""CPU: the network denoiser's tile plan (csrc/pt_nn_tiles.h, "Tiles" in include/mi355x_pathtracer.h) without a device: the library's
plan against the restated rule (tests/nn_tiles_ref.py) over a grid of frame sizes, limits and channel tables; what every plan must hold
whatever the rule, checked on its own; the network of tests/unet_ref.py run tile by tile against the whole frame, equal to the last bit;
the plan under the sanitizers as a stand-alone program (tests/nn_tiles_check.cpp); the new symbols, structs, veneer switch and driver
option in their sources.

Two of the plan's properties are checked in the form the rule allows.  (1) "One tile, or both tile dimensions at least 288" holds along
each side that is split: 289 x 17 is two tiles of 288 x 32, its height being the padded frame's.  (2) ptx_debug_nn_plan takes no frame
size and reports no scratch, so the one-tile plan's scratch_bytes is held to scratch_model, the restatement of the allocation's memory
model, which gives DESIGN.md's 494 MiB and 1962 MiB; tests/test_gpu_nn_tiles.py holds it to the one-tile handle's own figure."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import nn_tiles_ref as R
import unet_ref as U
from conftest import ROOT

CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
SIZES = (1, 16, 17, 287, 288, 289, 304, 400, 1920, 3840, 7680, 7681, 16384)
LIMITS = (0, 1, 8, 64, 512, 3000)
TABLES = {"standard3": (3, None), "standard9": (9, None), "wide": (6, U.WIDE)}
X, Y, W_, H_, OX, OY, OW, OH = range(8)


def _blob(ic, counts, seed=1):
    channels = U.table(ic, *counts) if counts else None
    return U.weights_blob(U.synthetic_weights(ic, seed, channels=channels, dtype=np.float16))


def _invariants(t, tiles):
    """what a plan must hold whatever rule made it; tiles: (n, 8) int32 in execution order"""
    W, H, tw, th, tx, ty = t["width"], t["height"], t["tile_width"], t["tile_height"], t["tiles_x"], t["tiles_y"]
    n = tx * ty
    what = (W, H, t["max_memory_mb"])
    assert tiles.shape == (n, 8), what
    a = tiles.astype(np.int64)
    # every window inside the frame, at a multiple of 16, within the tile buffer; the buffer within the cap
    assert (a[:, X] >= 0).all() and (a[:, Y] >= 0).all() and (a[:, W_] >= 1).all() and (a[:, H_] >= 1).all(), what
    assert (a[:, X] + a[:, W_] <= W).all() and (a[:, Y] + a[:, H_] <= H).all(), what
    assert (a[:, X] % 16 == 0).all() and (a[:, Y] % 16 == 0).all(), what
    assert (a[:, W_] <= tw).all() and (a[:, H_] <= th).all() and tw <= 7680 and th <= 4320 and tw % 16 == 0 and th % 16 == 0, what
    # a kept pixel is at least 96 pixels from every window edge that is not a frame edge
    assert (a[:, OW] >= 1).all() and (a[:, OH] >= 1).all(), what
    assert ((a[:, OX] - a[:, X] >= 96) | (a[:, X] == 0)).all() and ((a[:, OY] - a[:, Y] >= 96) | (a[:, Y] == 0)).all(), what
    right, bottom = a[:, X] + a[:, W_] - a[:, OX] - a[:, OW], a[:, Y] + a[:, H_] - a[:, OY] - a[:, OH]
    assert (a[:, OX] >= a[:, X]).all() and (a[:, OY] >= a[:, Y]).all() and (right >= 0).all() and (bottom >= 0).all(), what
    assert ((right >= 96) | (a[:, X] + a[:, W_] == W)).all() and ((bottom >= 96) | (a[:, Y] + a[:, H_] == H)).all(), what
    # one tile, or at least 288 along every side that is split
    assert (tx == 1 or tw >= 288) and (ty == 1 or th >= 288), what
    # the kept rectangles cover the frame exactly once: painted where the frame is small, and as a grid whose columns and rows each
    # cover their axis once at every size
    if W * H <= 1 << 21:
        count = np.zeros((H, W), np.int32)
        for r in a:
            count[r[OY]:r[OY] + r[OH], r[OX]:r[OX] + r[OW]] += 1
        assert (count == 1).all(), what
    g = a.reshape(ty, tx, 8)
    assert (g[:, :, OX] == g[0, :, OX]).all() and (g[:, :, OW] == g[0, :, OW]).all(), what
    assert (g[:, :, OY] == g[:, :1, OY]).all() and (g[:, :, OH] == g[:, :1, OH]).all(), what
    for begin, size, whole in ((g[0, :, OX], g[0, :, OW], W), (g[:, 0, OY], g[:, 0, OH], H)):
        assert begin[0] == 0 and (begin[1:] == (begin + size)[:-1]).all() and begin[-1] + size[-1] == whole, what


@pytest.mark.parametrize("table", sorted(TABLES))
def test_the_plan_is_the_restated_rule_and_holds_its_invariants(product, table):
    ic, counts = TABLES[table]
    blob = _blob(ic, counts)
    layers = product.debug_nn_plan(blob)["layers"]
    couts = [co for _, _, co in layers]
    one_tile = {}

    def scratch(tw, th):                                   # the library's figure for one tile of that size (limit 0, within the cap)
        if (tw, th) not in one_tile:
            t = product.debug_nn_tiling(blob, tw, th, 0, tiles=False)
            assert t["tiles_x"] == t["tiles_y"] == 1 and (t["tile_width"], t["tile_height"]) == (R.pad16(tw), R.pad16(th))
            one_tile[(tw, th)] = t["scratch_bytes"]
        return one_tile[(tw, th)]

    most = 0
    for W in SIZES:
        for H in SIZES:
            for mb in LIMITS:
                t = product.debug_nn_tiling(blob, W, H, mb, tiles="array")
                tw, th, tx, ty = R.plan(W, H, mb, scratch)
                assert (t["tile_width"], t["tile_height"], t["tiles_x"], t["tiles_y"]) == (tw, th, tx, ty), (W, H, mb)
                assert (t["width"], t["height"], t["max_memory_mb"]) == (W, H, mb)
                want = R.tiles_array(W, H, tw, th, tx, ty)
                assert np.array_equal(t["tiles"], want), (W, H, mb)
                assert t["scratch_bytes"] == scratch(tw, th) == R.scratch_model(couts, tw, th), (W, H, mb)
                shapes, counts_ = np.unique(np.stack([want[:, 2], want[:, 3]], 1), axis=0, return_counts=True)
                assert t["macs"] == sum(int(k) * R.macs_model(layers, int(w), int(h)) for (w, h), k in zip(shapes, counts_)), (W, H, mb)
                _invariants(t, t["tiles"])
                if mb == 0 and W <= 7680 and H <= 4320:
                    assert tx == ty == 1 and (tw, th) == (R.pad16(W), R.pad16(H))
                if mb > 0 and (tw > 288 or th > 288):
                    assert t["scratch_bytes"] <= mb * 2 ** 20, (W, H, mb)      # the limit holds wherever the tile is not at its minimum
                most = max(most, tx * ty)
    assert most == 169 * 169                                # 16384 x 16384 in 288 x 288 tiles: the largest plan there is


def test_the_memory_model_gives_the_documented_figures(product):
    """494 MiB at 1920 x 1080 and 1962 MiB at 3840 x 2160 with the standard table and 9 inputs, as one tile; the limits
    the time table is measured at split them as it says"""
    blob = _blob(9, None)
    mib = lambda w, h, mb: round(product.debug_nn_tiling(blob, w, h, mb, tiles=False)["scratch_bytes"] / 2 ** 20)
    assert mib(1920, 1080, 0) == 494 and mib(3840, 2160, 0) == 1962 and mib(3840, 2160, 3000) == 1962
    t = product.debug_nn_tiling(blob, 3840, 2160, 512)
    assert (t["tiles_x"], t["tiles_y"]) == (3, 2) and t["scratch_bytes"] <= 512 * 2 ** 20
    # the cap alone splits a frame no one-tile handle takes
    t = product.debug_nn_tiling(blob, 7696, 16, 0)
    assert (t["tiles_x"], t["tiles_y"], t["tile_width"], t["tile_height"]) == (2, 1, 3952, 16)


CASES = [(289, 17, 9, (2, 1)), (400, 40, 3, (3, 1)), (305, 300, 6, (2, 2))]


@pytest.mark.parametrize("w,h,ic,grid", CASES)
def test_the_network_tile_by_tile_is_the_network_on_the_whole_frame(product, w, h, ic, grid):
    """unet_ref.unet in float64 with NARROW weights on the plan's windows, the kept rectangles pasted together, against the same on the
    whole frame: no value differs.  The comparison can fail: the same tiles with an overlap of 64 differ (400 x 40: thousands of values)."""
    weights = U.synthetic_weights(ic, 3, channels=U.table(ic, *U.NARROW))
    t = product.debug_nn_tiling(U.weights_blob(weights), w, h, 1)
    assert (t["tiles_x"], t["tiles_y"]) == grid and t["tile_width"] == 288
    x = np.random.default_rng(w + h).random((h, w, ic))
    whole = U.unet(x, weights)
    tiled = R.tiled_unet(x, weights, t["tiles"])
    assert whole.std() > 0.01
    assert np.array_equal(tiled, whole), "%d values differ, by at most %g" % ((tiled != whole).sum(), np.abs(tiled - whole).max())
    if (w, h) == (400, 40):
        short = R.tiles(w, h, 288, 48, 2, 1, overlap=64)
        cut = R.tiled_unet(x, weights, short)
        assert not np.isnan(cut).any() and (cut != whole).sum() > 1000


def test_the_plan_is_clean_under_the_sanitizers(tmp_path):
    """tests/nn_tiles_check.cpp with its own main, -fsanitize=address,undefined, run as a program"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "nn_tiles_check"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "nn_tiles_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "nn_tiles_check: 0 failures" in r.stdout and "at most 28561 tiles" in r.stdout, r.stdout[-2000:]


def test_tile_structs_symbols_and_refusals(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    header = open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()
    assert "#define PTX_ABI_VERSION 5\n" in header and lib.ptx_abi_version() == api.ABI_VERSION == 5      # additive: the ABI stays
    for name in ("ptx_sizeof_nn_tile", "ptx_sizeof_nn_tiling", "ptx_nn_create_tiled", "ptx_nn_create_from_file_tiled", "ptx_nn_get_tiling",
                 "ptx_debug_nn_tiling"):
        assert hasattr(lib, name) and name + "(" in header, name
    for line in ("#define PTX_NN_TILE_ALIGN 16\n", "#define PTX_NN_TILE_OVERLAP 96\n", "#define PTX_NN_MIN_TILE 288 ", "#define PTX_NN_MAX_FRAME 16384 ",
                 "#define PTX_NN_MAX_WIDTH 7680 ", "#define PTX_NN_MAX_HEIGHT 4320\n", "} ptx_nn_tile;", "} ptx_nn_tiling;"):
        assert line in header, line
    assert lib.ptx_sizeof_nn_tile() == ctypes.sizeof(api.NNTile) == 32
    assert lib.ptx_sizeof_nn_tiling() == ctypes.sizeof(api.NNTiling) == 48
    assert lib.ptx_sizeof_nn_params() == 12 and lib.ptx_sizeof_nn_info() == ctypes.sizeof(api.NNInfo)      # the structs there were are as they were
    assert (R.ALIGN, R.OVERLAP, R.MIN_TILE, R.MAX_FRAME) == (16, 96, 288, 16384)
    blob = _blob(3, None)
    ptr = ctypes.cast(ctypes.c_char_p(blob), ctypes.c_void_p)
    out = ctypes.c_void_p(1)
    # the refusals that need no device, from the create call and from the host-only plan alike
    assert lib.ptx_nn_create_tiled(0, 64, 64, ptr, len(blob), -1, ctypes.byref(out)) == 1 and out.value is None
    assert b"max_memory_mb" in lib.ptx_last_error()
    assert lib.ptx_nn_create_tiled(0, 16385, 1, ptr, len(blob), 0, ctypes.byref(out)) == 1 and b"bad frame size" in lib.ptx_last_error()
    assert lib.ptx_nn_create_tiled(0, 1, 16385, ptr, len(blob), 0, ctypes.byref(out)) == 1 and b"bad frame size" in lib.ptx_last_error()
    assert lib.ptx_nn_create_tiled(0, 0, 4, ptr, len(blob), 0, ctypes.byref(out)) == 1 and b"bad frame size" in lib.ptx_last_error()
    assert lib.ptx_nn_create_tiled(0, 64, 64, ptr, len(blob), 0, None) == 1
    assert lib.ptx_nn_create_tiled(0, 64, 64, ptr, 100, 0, ctypes.byref(out)) == 1 and b"weight blob" in lib.ptx_last_error()
    assert lib.ptx_nn_create_from_file_tiled(0, 64, 64, b"/nonexistent/weights.tza", 0, ctypes.byref(out)) == 2
    assert lib.ptx_nn_create(0, 7681, 1, ptr, len(blob), ctypes.byref(out)) == 1 and b"bad frame size" in lib.ptx_last_error()      # as before
    for bad, match in (((64, 64, -1), "max_memory_mb"), ((16385, 1, 0), "bad frame size"), ((1, 16385, 0), "bad frame size"), ((0, 4, 0), "bad frame size")):
        with pytest.raises(product.PathTracerError, match=match):
            product.debug_nn_tiling(blob, *bad)
    with pytest.raises(product.PathTracerError, match="weight blob"):
        product.debug_nn_tiling(blob[:100], 64, 64, 0)
    tiling = api.NNTiling()
    assert lib.ptx_debug_nn_tiling(ptr, len(blob), 400, 40, 1, None, None, 0) == 1
    assert lib.ptx_nn_get_tiling(None, ctypes.byref(tiling), None, 0) == 1
    # cap: the first min(cap, n) tiles are written, the rest of the caller's array is left alone
    three = (api.NNTile * 3)()
    three[2].x = -7
    assert lib.ptx_debug_nn_tiling(ptr, len(blob), 400, 40, 1, ctypes.byref(tiling), three, 2) == 0
    assert tiling.tiles_x == 3 and (three[0].w, three[1].x, three[1].out_x, three[2].x) == (288, 96, 192, -7)
    if lib.ptx_device_count() < 1:
        assert lib.ptx_nn_create_tiled(0, 400, 40, ptr, len(blob), 1, ctypes.byref(out)) == 4 and out.value is None


def test_veneer_switch_driver_option_and_host_only_header():
    veneer_h = open(os.path.join(CSRC, "pathtrace_api.h")).read()
    veneer = open(os.path.join(CSRC, "pathtrace_api.cpp")).read()
    driver = open(os.path.join(CSRC, "main_headless.cpp")).read()
    assert "int &nnMaxMemoryMB();" in veneer_h and "std::string &nnWeights();" in veneer_h
    assert "ptx_nn_create_from_file_tiled(g_device, w, h, nnWeights().c_str(), nnMaxMemoryMB(), &g_nn)" in veneer
    assert "static int mb = -1;" in veneer                                                        # the default: ptx_nn_create_from_file, as before
    assert 'a == "--nn-max-memory"' in driver and "ptx_nn_create_from_file_tiled(nn_device, width, height, nn_path.c_str(), nn_max_memory, &nn)" in driver
    assert "--nn-max-memory needs --nn FILE" in driver
    tiles_h = open(os.path.join(CSRC, "pt_nn_tiles.h")).read()
    assert "#include <hip" not in tiles_h and "hipMalloc" not in tiles_h and "pt_handle.h" not in tiles_h
    unit = open(os.path.join(CSRC, "pt_nn.hip")).read()
    assert "pt_nn_scratch(plan, n->wp, n->hp)" in unit and "pt_nn_tiling(plan, n->w, n->h, tl_max_memory_mb)" in unit      # one memory model
    assert unit.count("__global__") == 3                                                          # k_nn_input, k_nn_output, k_nn_conv<>: no kernel added
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "pt_nn_tiles.h" in makefile
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "one tile is the whole frame" not in design and "one tile is the whole frame" not in open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()


def test_headless_refuses_the_memory_option_without_weights(product):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", CSRC, "headless"])
    r = subprocess.run([exe, "scene.txt", "--denoise", "--nn-max-memory", "512"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "--nn-max-memory needs --nn FILE" in r.stderr
    r = subprocess.run([exe, "scene.txt", "--denoise", "--nn", "w.tza", "--nn-max-memory", "-1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "--nn-max-memory needs MB >= 0" in r.stderr
