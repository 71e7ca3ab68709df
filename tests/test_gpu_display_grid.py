"""GPU: the display transform's kernels (csrc/pt_display.hip) where the small frames of tests/test_gpu_display.py cannot take them
(cases: tests/displaycases.py, checked on the CPU by tests/test_display_grid_cpu.py):

    k_display_meter  at block counts around every guard of its four loads per trip, into its second trip (1023 .. 5121 blocks)
    k_display_blocks on a block of 529 pixels, the only one whose third trip runs, and its 506-pixel neighbours
    k_display_map    over tone x transfer x exposure (2^-20 .. 3e34), samples and white, on a frame of every value class a channel can
                     hold; at every W*H mod 4, below one quad and at exactly one, in both forms
    adaptation       across keys and rates over six frames
"""
import struct

import numpy as np
import pytest

import display_ref as dr
import displaycases as dc
from conftest import beq
from test_gpu_display import BLOCK_TOL, TOL, _dev, _metric

pytestmark = pytest.mark.gpu

# |log2_mean - the float64 mean of log2 of the device's own block luminances|.  The ROCm installation documents no accuracy bound for
# the device's log2f, so: the largest deviation over the thirteen column frames measured on one MI355X (LOG2_MEAN_SEEN, at 4096 blocks;
# the test prints each), times four.
LOG2_MEAN_SEEN = 1.277e-8
LOG2_MEAN_TOL = 4 * LOG2_MEAN_SEEN
_COLUMNS = {}


def _column(n, scale=1.0):
    if (n, scale) not in _COLUMNS:
        _COLUMNS[(n, scale)] = dc.column_frame(n, seed=n, scale=scale)
    return _COLUMNS[(n, scale)]


def _log2_mean_of(blocks):
    v = blocks.ravel()
    v = v[v > np.float32(dr.L_MIN)].astype(np.float64)
    return float(np.log2(v).mean()), int(v.size)


@pytest.mark.parametrize("n", dc.METER_BLOCK_COUNTS)
def test_meter_around_every_guard_of_its_four_loads(gpu_product, n):
    """One column of n constant blocks whose exponents differ between any two blocks 1024 j apart: the counts exactly, the block
    luminances, log2_mean against the float64 mean over the device's own blocks, the metered exposure, and the same bits twice."""
    pt = gpu_product
    c = _column(n)
    with pt.Display(c["w"], c["h"]) as D:
        d = _dev(c["rgb"])
        D.device(d.data_ptr(), 1)
        got, st = D.blocks(), D.status()
        D.device(d.data_ptr(), 1)
        st2 = D.status()
        assert beq(got, D.blocks()) and st2.pop("frames") == 2 and st.pop("frames") == 1 and st == st2
        assert all(struct.pack("f", st[k]) == struct.pack("f", st2[k]) for k in ("metered", "applied", "log2_mean"))
    assert got.shape == (n, 1) and (st["blocks_total"], st["blocks_used"]) == (n, c["blocks_used"])
    want = c["blocks"]
    zero = want == 0
    assert zero.any() and (got[:, 0][zero] == 0).all()
    rel = float((np.abs(got[:, 0].astype(np.float64) - want)[~zero] / want[~zero]).max())
    m, used = _log2_mean_of(got)
    dev = abs(st["log2_mean"] - m)
    print("%d blocks: block luminances within %.3g relative; log2_mean %.9g, float64 over the device's blocks %.12g: off by %.3g (bound %.3g)"
          % (n, rel, st["log2_mean"], m, dev, LOG2_MEAN_TOL))
    assert rel <= BLOCK_TOL and used == c["blocks_used"]
    # the smallest single-block mistake, one exponent off by 1 in one block, is at least ten bounds even at the largest frame
    assert 1.0 / max(dc.METER_BLOCK_COUNTS) >= 10 * LOG2_MEAN_TOL and 1.0 / n >= 10 * LOG2_MEAN_TOL
    assert dev <= LOG2_MEAN_TOL
    assert abs(m - c["log2_mean"]) <= 1e-6                                           # (the device's blocks are the constants' to 1.2e-7)
    metered = float(np.float32(0.18)) / 2.0 ** c["log2_mean"]
    assert abs(st["metered"] - metered) <= BLOCK_TOL * metered and st["applied"] == st["metered"]


@pytest.mark.parametrize("w,h", ((23, 23), (22, 23), (23, 22)))
def test_blocks_beyond_512_pixels(gpu_product, w, h):
    """23 x 23 is one block of 529 pixels: thread t adds pixels t, t + 256 and t + 512"""
    pt = gpu_product
    rgb = dc.hdr_buffer(w, h)
    want = dr.block_means(rgb, 3, w, h)
    ref = dr.meter(want)
    assert want.shape == (1, 1) and want[0, 0] > 1e-3 and ref["blocks_used"] == 1
    with pt.Display(w, h) as D:
        assert D.status() == dict(metered=1.0, applied=1.0, log2_mean=0.0, blocks_used=0, blocks_total=1, frames=0)
        D.host(rgb, 3)
        got, st = D.blocks(), D.status()
        D.host(rgb, 3)
        st2 = D.status()
        assert beq(got, D.blocks()) and st2.pop("frames") == 2 and st.pop("frames") == 1 and st == st2
    rel = abs(float(got[0, 0]) - want[0, 0]) / want[0, 0]
    print("%d x %d (%d pixels): block average within %.3g relative" % (w, h, w * h, rel))
    assert got.shape == (1, 1) and rel <= BLOCK_TOL
    assert (st["blocks_used"], st["blocks_total"]) == (1, 1)
    assert abs(st["metered"] - ref["metered"]) <= BLOCK_TOL * ref["metered"] and st["applied"] == st["metered"]
    assert abs(st["log2_mean"] - ref["log2_mean"]) <= 1e-3


_SWEEP = {}


def _sweep(samples):
    """the sweep frame times `samples`, on the host and on the device, once per value of samples"""
    if samples not in _SWEEP:
        rgb = (dc.sweep_frame() * np.float32(samples)).astype(np.float32)
        _SWEEP[samples] = (rgb, _dev(rgb))
    return _SWEEP[samples]


# float32(1.055) * 1 - float32(0.055), the fp32 value of the sRGB branch at y = 1 (log2 1 = 0 and exp2 0 = 1 are exact): 1 - 2^-24
SRGB_OF_ONE = np.float32(np.float32(1.055) * np.float32(1.0) - np.float32(0.055))


@pytest.mark.parametrize("case", dc.MAP_GRID, ids=dc.case_id)
def test_map_over_the_parameter_grid(gpu_product, case):
    """z against the float64 restatement, the codes against the numpy quantiser of the device's own z, alpha 0; a pixel the curve takes
    to 1 or beyond holds exactly the transfer of 1, and a channel sanitised to 0 holds 0"""
    from mygpuraytracer_amd import api
    pt = gpu_product
    w, h = dc.SWEEP_SIZE
    rgb, d = _sweep(case["samples"])
    tone, transfer = api._DISPLAY_NAMES["tone"][case["tone"]], api._DISPLAY_NAMES["transfer"][case["transfer"]]
    E, white = float(np.float32(case["exposure"])), float(np.float32(case["white"]))
    ref = dr.display(rgb, case["samples"], E, tone, transfer, white=white)
    y = dc.premapped(case)
    c = dr.sanitise(rgb, case["samples"])
    sat = dc.saturated(case, y)
    assert sat.any() or E < 1e-4
    assert (c == 0).any() and ((y > 0) & (y < 1)).any()
    one = SRGB_OF_ONE if case["transfer"] == "srgb" else np.float32(1.0)
    with pt.Display(w, h) as D:
        for cs, (quantize, dither) in dc.map_launches():
            if cs is not case:
                continue
            D.device(d.data_ptr(), case["samples"], meter="manual", exposure=case["exposure"], tone=case["tone"], transfer=case["transfer"],
                     white=case["white"], quantize=quantize, dither=dither, keep_float=1)
            z, codes = D.read(float_frame=True)
            m = _metric(z, ref)
            print("%s q%d d%d: z within %.3g; %d saturated, %d black channels" % (dc.case_id(case), quantize, dither, m, sat.sum(), (c == 0).sum()))
            assert D.status()["frames"] == 0
            assert np.array_equal(codes, dr.quantise(z, w, h, quantize, dither)) and not codes[..., 3].any()
            assert (z[c == 0] == 0).all()
            wrong = z[sat] != one
            assert not wrong.any(), "%d of %d saturated channels are not %r: %r" % (wrong.sum(), wrong.size, one, np.unique(z[sat][wrong])[:8])
            assert m <= TOL


def _poison(D, n, keep):
    """a frame of 65504s through the handle first: codes 255 and z 1 everywhere, so a pixel the next call does not write shows"""
    import torch
    full = torch.full((3 * n + 8,), 65504.0, dtype=torch.float32, device="cuda:0")
    D.device(full.data_ptr(), 1, meter="manual", exposure=1.0, tone="clamp", transfer="linear", keep_float=keep)
    assert (D.read() == np.array([255, 255, 255, 0], np.uint8)).all()
    return full


@pytest.mark.parametrize("w,h", dc.TAIL_SIZES)
def test_tails_in_both_forms(gpu_product, w, h):
    """every W*H mod 4, frames below one quad and of exactly one: the 16-byte-aligned form and the frame 4 bytes off the grid, with and
    without keep_float, into the handle's buffer and into a caller's between guard bytes: one z, one set of codes, the guards whole"""
    import torch
    from mygpuraytracer_amd import api
    pt = gpu_product
    n = w * h
    rgb = dc.hdr_buffer(w, h) if n >= 12 else (np.arange(1, 3 * n + 1, dtype=np.float32).reshape(h, w, 3) / np.float32(4))
    kw = dict(meter="manual", exposure=0.7, tone="aces", transfer="srgb", dither=1)
    ref = dr.display(rgb, 3, float(np.float32(0.7)), api.TONE_ACES, api.TRANSFER_SRGB)
    d = _dev(rgb)
    shifted = torch.zeros(3 * n + 8, dtype=torch.float32, device="cuda:0")
    shifted[1:1 + 3 * n] = d.reshape(-1)
    assert d.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 0
    GUARD = 32
    seen = []
    with pt.Display(w, h) as D:
        for src in (d.data_ptr(), shifted.data_ptr() + 4):
            for keep in (1, 0):
                for own in (True, False):
                    _poison(D, n, keep)
                    pbo = torch.full((4 * n + 2 * GUARD,), 7, dtype=torch.uint8, device="cuda:0")
                    assert pbo.data_ptr() % 16 == 0
                    D.device(src, 3, pbo=None if own else pbo.data_ptr() + GUARD, keep_float=keep, **kw)
                    z = D.read_float() if keep else None
                    torch.cuda.synchronize()
                    host = pbo.cpu().numpy()
                    codes = D.read() if own else host[GUARD:GUARD + 4 * n].reshape(h, w, 4)
                    assert (host[:GUARD] == 7).all() and (host[GUARD + 4 * n:] == 7).all()
                    assert own == (host == 7).all()
                    seen.append((z, codes))
    z0 = seen[0][0]
    assert _metric(z0, ref) <= TOL
    want = dr.quantise(z0, w, h, 1, 1)
    for z, codes in seen:
        assert np.array_equal(codes, want) and (z is None or beq(z, z0))


@pytest.mark.parametrize("key", (0.01, 0.18, 10.0))
@pytest.mark.parametrize("adapt", (0.05, 0.5, 1.0))
def test_adaptation_across_keys_and_rates(gpu_product, adapt, key):
    """six metered frames of one 1025-block column at scales 1, 8, 1/8, 64, 1, 1/64: metered = key / 2^m of each, applied follows the
    recurrence of the restatement at every step, and the first frame and the one after reset() jump"""
    pt = gpu_product
    n = 1025
    scales = (1.0, 8.0, 0.125, 64.0, 1.0, 1.0 / 64)
    with pt.Display(8, 16 * n - 8) as D:
        prev = None
        for i, s in enumerate(scales):
            c = _column(n, s)
            d = _dev(c["rgb"])
            D.device(d.data_ptr(), 1, adapt=adapt, key=key)
            st = D.status()
            metered = float(np.float32(key)) / 2.0 ** c["log2_mean"]
            assert st["frames"] == i + 1 and (st["blocks_used"], st["blocks_total"]) == (c["blocks_used"], n)
            assert abs(st["metered"] - metered) <= BLOCK_TOL * metered, (s, st, metered)
            if prev is None or adapt == 1.0:
                assert st["applied"] == st["metered"]
            else:
                want = dr.adapt(prev["applied"], st["metered"], adapt)
                assert abs(st["applied"] - want) <= 1e-6 * want, (i, s, st, want)
                if s != scales[i - 1]:
                    assert st["applied"] != st["metered"]
            prev = st
        assert len({_column(n, s)["blocks_used"] for s in scales}) > 1                # the scales move blocks across L_MIN and 65504
        D.reset()
        assert D.status()["frames"] == 0 and D.status()["applied"] == 1.0
        c = _column(n, 8.0)
        D.device(_dev(c["rgb"]).data_ptr(), 1, adapt=adapt, key=key)
        st = D.status()
        assert st["frames"] == 1 and st["applied"] == st["metered"]
        assert abs(st["metered"] - float(np.float32(key)) / 2.0 ** c["log2_mean"]) <= BLOCK_TOL * st["metered"]
