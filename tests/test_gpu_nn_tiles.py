"""GPU: the network denoiser under a memory limit (ptx_nn_create_tiled, csrc/pt_nn.hip, csrc/pt_nn_tiles.h): a tiled run gives the
bits of a one-tile run.  Every case makes two handles from one blob for one size, NN(w, h, blob) and NN(w, h, blob, max_memory_mb=...),
runs both on the same frames and compares bit for bit -- and asserts the tile grid it expects, so that a plan that quietly returns one
tile cannot pass.  The one-tile path is held to the float64 restatement by tests/test_gpu_nn.py and tests/test_gpu_nn_channels.py; the
one frame here that no one-tile handle takes (7696 x 16) is held to it directly, by test_gpu_nn.py's rule.  Synthetic weights only.

The frames are a few hundred pixels on a side: the smallest tile is 288, so 289 is the first width that splits."""
import os

import numpy as np
import pytest

import unet_ref as U
from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

_BLOBS = {}


def _weights(ic, table, seed=1):
    key = (ic, table, seed)
    if key not in _BLOBS:
        channels = U.table(ic, *U.NARROW) if table == "narrow" else None
        w = U.synthetic_weights(ic, seed, channels=channels)
        _BLOBS[key] = (w, U.weights_blob(w))
    return _BLOBS[key]


def _frames(w, h, ic, seed):
    """colour in [0, 2) with a few NaN and negative values, albedo in [0, 1), normals in [-1, 1)"""
    rng = np.random.default_rng(seed)
    rgb = (rng.random((h, w, 3), dtype=np.float32) * 2).astype(np.float32)
    flat = rgb.reshape(-1)
    where = rng.choice(flat.size, 12, replace=False)
    flat[where[:6]] = np.nan
    flat[where[6:]] = -0.75
    alb = rng.random((h, w, 3), dtype=np.float32) if ic >= 6 else None
    nrm = (rng.random((h, w, 3), dtype=np.float32) * 2 - 1).astype(np.float32) if ic >= 9 else None
    return rgb, alb, nrm


def _grid(nn):
    t = nn.tiling()
    return t["tiles_x"], t["tiles_y"]


# frame, input channels, table, limit (MiB), the grid expected
CASES = [
    (289, 17, 3, "narrow", 1, (2, 1)),      # one pixel past the smallest tile; the last window is 193 wide in a 288-wide buffer
    (17, 289, 9, "narrow", 1, (1, 2)),      # the same in y, with guides
    (400, 40, 6, "standard", 1, (3, 1)),    # a middle tile that drops its overlap on both sides
    (305, 300, 9, "narrow", 1, (2, 2)),     # corners; both tile dimensions ragged
]


@pytest.mark.parametrize("w,h,ic,table,mb,grid", CASES, ids=["%dx%d" % c[:2] for c in CASES])
def test_tiled_is_one_tile_bit_for_bit(gpu_product, w, h, ic, table, mb, grid):
    pt = gpu_product
    _, blob = _weights(ic, table)
    rgb, alb, nrm = _frames(w, h, ic, w + h)
    with pt.NN(w, h, blob) as one, pt.NN(w, h, blob, max_memory_mb=mb) as tiled:
        want = one.host(rgb, alb, nrm)
        got = tiled.host(rgb, alb, nrm)
        t = tiled.tiling()
        print("%dx%d ic %d: %d x %d tiles, %d of %d values differ" % (w, h, ic, t["tiles_x"], t["tiles_y"],
                                                                    (got.view(np.uint32) != want.view(np.uint32)).sum(), got.size))
        assert want.std() > 0.01 and beq(got, want)
        assert _grid(one) == (1, 1) and _grid(tiled) == grid
        assert t == pt.debug_nn_tiling(blob, w, h, mb) and (t["tile_width"] >= 288 or grid[0] == 1) and (t["tile_height"] >= 288 or grid[1] == 1)
        # the tiled handle reports its tile buffer, the tile's scratch and the summed work; the one-tile handle's figures are the plan's at limit 0
        ti, oi = tiled.info(), one.info()
        assert (ti["padded_width"], ti["padded_height"], ti["scratch_bytes"], ti["macs"]) == (t["tile_width"], t["tile_height"], t["scratch_bytes"], t["macs"])
        assert ti["scratch_bytes"] < oi["scratch_bytes"]
        p0 = pt.debug_nn_tiling(blob, w, h, 0)
        assert (oi["scratch_bytes"], oi["macs"], oi["padded_width"], oi["padded_height"]) == (p0["scratch_bytes"], p0["macs"], p0["tile_width"], p0["tile_height"])
        assert ti["macs"] > oi["macs"]
    # no limit within the cap: the handle ptx_nn_create makes
    with pt.NN(w, h, blob, max_memory_mb=0) as same:
        assert same.info() == oi and _grid(same) == (1, 1) and beq(same.host(rgb, alb, nrm), want)


def test_a_tile_between_the_minimum_and_the_frame(gpu_product):
    """1024 x 64 under the first limit that gives 288 < tile_width < 1024: the rule's pad16(ceil(..)) + 192 branch"""
    pt = gpu_product
    w, h, ic = 1024, 64, 3
    _, blob = _weights(ic, "standard")
    plans = {mb: pt.debug_nn_tiling(blob, w, h, mb, tiles=False) for mb in range(1, 33)}
    mb = min(m for m, t in plans.items() if 288 < t["tile_width"] < 1024)
    rgb, _, _ = _frames(w, h, ic, 5)
    with pt.NN(w, h, blob) as one, pt.NN(w, h, blob, max_memory_mb=mb) as tiled:
        t = tiled.tiling()
        assert 288 < t["tile_width"] < 1024 and t["tiles_x"] >= 2 and t["tiles_y"] == 1 and t["scratch_bytes"] <= mb * 2 ** 20
        assert t["tile_width"] == (-(-(w - 192) // t["tiles_x"]) + 15) // 16 * 16 + 192
        print("1024x64 limit %d MiB: %d tiles of %d" % (mb, t["tiles_x"], t["tile_width"]))
        assert beq(tiled.host(rgb), one.host(rgb))


def test_the_meter_runs_once_on_the_whole_frame(gpu_product):
    """hdr with the automatic scale on a frame whose left half is 1000 times brighter: a scale taken tile by tile would differ between
    the tiles; the scale read back is the one-tile handle's, bit for bit, and so is the frame"""
    pt = gpu_product
    w, h, ic = 400, 40, 3
    _, blob = _weights(ic, "standard")
    rgb, _, _ = _frames(w, h, ic, 9)
    rgb[:, : w // 2] *= np.float32(1000)
    with pt.NN(w, h, blob) as one, pt.NN(w, h, blob, max_memory_mb=1) as tiled:
        assert _grid(tiled) == (3, 1)
        want = one.host(rgb, samples=2, hdr=1)
        got = tiled.host(rgb, samples=2, hdr=1)
        assert one.scale().tobytes() == tiled.scale().tobytes() and one.scale() != 1 and one.scale() > 0
        assert beq(got, want) and np.isfinite(want).all() and want.std() > 0


def test_a_tiled_handle_leaves_nothing_behind(gpu_product):
    """the same tiled handle on two different frames, then on the first again: the first and third results are equal (the scratch is
    one buffer for every tile, and a short last tile uses a prefix of it)"""
    pt = gpu_product
    w, h, ic = 305, 300, 9
    _, blob = _weights(ic, "narrow")
    a, b = _frames(w, h, ic, 21), _frames(w, h, ic, 22)
    with pt.NN(w, h, blob, max_memory_mb=1) as tiled:
        assert _grid(tiled) == (2, 2)
        first, second, third = tiled.host(*a), tiled.host(*b), tiled.host(*a)
        assert beq(first, third) and not beq(first, second)


def test_tracer_denoise_nn_takes_a_tiled_handle(gpu_product):
    """a 304 x 48 Cornell render at 2 spp: the tracer's accumulation buffer and its float4 G-buffer records through the windows"""
    pt = gpu_product
    W, H, spp, ic = 304, 48, 2, 9
    _, blob = _weights(ic, "narrow")
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"), res=(W, H), depth=4)
    s.apply_runcuda_camera()
    with pt.NN(W, H, blob) as one, pt.NN(W, H, blob, max_memory_mb=1) as tiled, pt.Tracer(s) as T:
        assert _grid(tiled) == (2, 1)
        T.render(1, spp)
        want = T.denoise_nn(one, spp).copy()
        got = T.denoise_nn(tiled, spp)
        assert beq(got, want) and want.any()


def test_a_frame_above_the_tile_cap_against_the_float64_restatement(gpu_product):
    """7696 x 16 with max_memory_mb = 0: two tiles by the cap alone, and no one-tile handle to compare with.  Linear mode, NARROW, 3
    inputs: A = the float64 restatement, B = the float32 one; test_gpu_nn.py's rule, max|gpu - A| <= 4 max|A - B| and the same for the RMS,
    with 4 max|A - B| <= rms(A) / 4 so that the bound cannot hide a window or offset error."""
    pt = gpu_product
    w, h, ic = 7696, 16, 3
    weights, blob = _weights(ic, "narrow")
    rgb = np.random.default_rng(7).random((h, w, 3), dtype=np.float32)
    with pytest.raises(pt.PathTracerError, match="bad frame size"):
        pt.NN(w, h, blob)
    with pt.NN(w, h, blob, max_memory_mb=0) as tiled:
        t = tiled.tiling()
        assert t["tiles_x"] >= 2 and t["tiles_y"] == 1 and t["tile_width"] <= 7680
        got = tiled.host(rgb, srgb=1).astype(np.float64)
    A = U.denoise(rgb, weights, srgb=1)
    B = U.denoise(rgb, weights, srgb=1, dtype_name="float32")
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    print("7696x16: max|A-B| %.3g rms|A-B| %.3g rms(A) %.3g; max|gpu-A| %.3g rms|gpu-A| %.3g" % (
        np.abs(A - B).max(), rms(A - B), rms(A), np.abs(got - A).max(), rms(got - A)))
    assert 4 * np.abs(A - B).max() <= rms(A) / 4
    assert np.abs(got - A).max() <= 4 * np.abs(A - B).max()
    assert rms(got - A) <= 4 * rms(A - B)


def test_refusals(gpu_product):
    import torch
    pt = gpu_product
    w, h = 289, 17
    _, blob = _weights(3, "narrow")
    with pytest.raises(pt.PathTracerError, match="max_memory_mb"):
        pt.NN(w, h, blob, max_memory_mb=-1)
    with pytest.raises(pt.PathTracerError, match="bad frame size"):
        pt.NN(16385, 1, blob, max_memory_mb=0)
    with pytest.raises(pt.PathTracerError, match="bad frame size"):
        pt.NN(7681, 1, blob)                                                      # ptx_nn_create is as it was
    buf = torch.rand((2 * h * w * 3 + 4,), dtype=torch.float32, device="cuda:0")
    p, frame = buf.data_ptr(), 4 * h * w * 3
    with pt.NN(w, h, blob) as one, pt.NN(w, h, blob, max_memory_mb=1) as tiled:
        assert _grid(tiled) == (2, 1)
        for rgb, out in ((p, p), (p, p + 4), (p, p + frame - 4), (p + frame - 4, p)):      # the same bytes; ranges that share their first or last float
            with pytest.raises(pt.PathTracerError, match="may not overlap"):
                tiled.device(rgb, out)
        with pytest.raises(pt.PathTracerError, match="no denoise"):
            tiled.scale()                                                         # nothing of that was enqueued
        tiled.device(p, p + frame)                                                # side by side: accepted
        assert tiled.scale() == 1
        one.device(p, p)                                                          # one tile stays as permissive as it was
        assert one.scale() == 1
        torch.cuda.synchronize()
