"""GPU: the active-tile mask of the tracer (include/mi355x_pathtracer.h: ptx_set_active_tiles, ptx_clear_active_tiles).  A mask that
switches nothing off that traces anything changes no bit; an inactive tile's pixels keep theirs; the active pixels receive what they
receive without a mask in distribution (no bias over a run); the mask survives a camera change; the refusals."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, beq
from test_gpu_lit_planes import aux_nonzero

pytestmark = pytest.mark.gpu

WIDE = (768, 24)         # three tiles to a row: tiles do not wrap whole rows
ODD = (97, 61)           # 23 whole tiles and one of 29 pixels
DEPTH = 4
# test_active_pixels_are_unbiased: the largest ratio of the mean squared errors of two unmasked 64-iteration runs of WIDE over the same
# pixels, among 8 runs on disjoint iteration ranges (28 pairs), measured on an MI355X by mse_of_unmasked_runs below, times
# 1.25 for a ninth draw.  Not taken from the masked run.
WORST_UNMASKED_RATIO = 1.429194    # mean squared errors from 5.13e-4 to 7.34e-4
BOUND = 1.25 * WORST_UNMASKED_RATIO


def _scene(pt, name, res, depth=DEPTH):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s


def base_words(pt, s):
    """the per-tile words of visible geoms the tracer computes for this camera (ptx_debug_tile_geoms, on the CPU), from the geoms' world
    boxes formed as ptx_create forms them: the transformed unit cube or mesh vertices in double, widened by 1e-3 + 1e-4 |coordinate|"""
    d = s.dump()
    boxes = []
    for gi in range(len(d["geom_ints"])):
        xf = d["geom_mats"][gi][:16].reshape(4, 4).T.astype(np.float64)
        f = d["faces"][gi]
        if len(f):
            v = np.concatenate([f[:, 0:3], f[:, 5:8], f[:, 10:13]]).astype(np.float64)
        else:
            v = np.array([[sx, sy, sz] for sz in (-.5, .5) for sy in (-.5, .5) for sx in (-.5, .5)], np.float64)
        w = (v[:, 0:1] * xf[:3, 0] + v[:, 1:2] * xf[:3, 1]) + v[:, 2:3] * xf[:3, 2] + xf[:3, 3]
        lo, hi = w.min(0), w.max(0)
        m = 1e-3 + 1e-4 * np.maximum(np.abs(lo), np.abs(hi))
        boxes.append(np.concatenate([np.nextafter((lo - m).astype(np.float32), np.float32(-np.inf)),
                                     np.nextafter((hi + m).astype(np.float32), np.float32(np.inf))]))
    return pt.api.debug_tile_geoms(s.camera, np.array(boxes, np.float32))


def tile_of_pixel(pt, T):
    return np.arange(T.width * T.height) // pt.tile_pixels()


def _sees(pt, s, T):
    """precondition, checked on the CPU: the frame has tiles that see no geom and tiles that see some"""
    words = base_words(pt, s)
    assert len(words) == T.num_tiles and (words == 0).any() and (words != 0).any(), (len(words), T.num_tiles)
    return words != 0


def _drive(T, first, count, how):
    if how == "render":
        T.render(first, count)
    else:
        T.set_render_ahead(how == "ahead")
        for it in range(first, first + count):
            T.pathtrace(it)


CASES = [("cornell.txt", "render"), ("cornell.txt", "ahead"), ("cornell.txt", "per_call"), ("cornellObj.txt", "render"),
         ("cornellObj.txt", "ahead"), ("cornellSpaceship20k.txt", "render"), ("cornellSpaceship20k.txt", "ahead")]


@pytest.mark.parametrize("scene,how", CASES, ids=["%s-%s" % (s[:-4], h) for s, h in CASES])
def test_a_mask_that_switches_nothing_off_changes_no_bit(gpu_product, scene, how):
    """8 iterations under a mask of all ones, and under one that switches off exactly the tiles that see no geom anyway, against a tracer
    that never had a mask: image and statistics bit for bit, through ptx_render and ptx_iterate with render-ahead on and off, with a small
    mesh and with the split mesh search."""
    pt = gpu_product
    s = _scene(pt, scene, WIDE)
    with pt.Tracer(s) as N, pt.Tracer(s) as A, pt.Tracer(s) as Z:
        sees = _sees(pt, s, N)
        if scene == "cornellSpaceship20k.txt":
            meshes = [g for g, f in enumerate(s.dump()["faces"]) if len(f)]
            assert meshes and N.mesh_plan(meshes[0])["split"] == 1
        A.set_active_tiles(np.ones(A.num_tiles, np.uint8))
        Z.set_active_tiles(sees)
        for T in (N, A, Z):
            _drive(T, 1, 8, how)
        img, st = N.read_image(), N.stats()
        assert img.any()
        for T in (A, Z):
            assert beq(T.read_image(), img), how
            assert T.stats()["rays_per_bounce"] == st["rays_per_bounce"] and T.stats()["iterations"] == st["iterations"]


@pytest.mark.parametrize("how", ["render", "ahead"])
def test_inactive_tiles_keep_their_bits_and_clearing_restores_the_tracer(gpu_product, how):
    """4 iterations unmasked, then 8 under a mask that switches off every second tile that sees geometry: the inactive tiles' pixels hold
    the bits they held, every active tile that had light has changed (not to what it holds without a mask: a path's random numbers are
    seeded by its place in the sorted stream, which the missing paths shift), the camera bounce still counts every pixel, nothing is
    left in the planes and totals.  After clearing the mask and resetting the image the tracer is a fresh one."""
    pt = gpu_product
    s = _scene(pt, "cornell.txt", WIDE)
    with pt.Tracer(s) as T, pt.Tracer(s) as N:
        sees = _sees(pt, s, T)
        tile = tile_of_pixel(pt, T)
        off = np.zeros(T.num_tiles, bool)
        off[np.flatnonzero(sees)[::2]] = True
        assert off.sum() >= 2 and (sees & ~off).sum() >= 2
        for X in (T, N):
            _drive(X, 1, 4, how)
        before = T.read_image()
        assert beq(before, N.read_image())
        T.set_active_tiles(~off)
        for X in (T, N):
            _drive(X, 5, 8, how)
        after, full = T.read_image(), N.read_image()
        assert beq(after[off[tile]], before[off[tile]])
        lit = np.array([before[tile == t].any() for t in range(T.num_tiles)])
        assert (lit & ~off).sum() >= 2
        for t in np.flatnonzero(lit & ~off):
            assert not beq(after[tile == t], before[tile == t]), t
        st, sn = T.stats(), N.stats()
        assert st["rays_per_bounce"][0] == sn["rays_per_bounce"][0] > 0 and st["iterations"] == sn["iterations"] == 12
        assert st["rays_per_bounce"][1] < sn["rays_per_bounce"][1]
        assert aux_nonzero(T)[:2] == [0, 0]
        T.clear_active_tiles()
        T.reset_image()
        _drive(T, 1, 8, how)
        with pt.Tracer(s) as F:
            _drive(F, 1, 8, how)
            assert beq(T.read_image(), F.read_image()) and T.stats()["rays_per_bounce"] == F.stats()["rays_per_bounce"]


def test_the_mask_outlives_a_camera_change(gpu_product):
    pt = gpu_product
    s = _scene(pt, "cornell.txt", WIDE)
    with pt.Tracer(s) as T:
        sees = _sees(pt, s, T)
        tile = tile_of_pixel(pt, T)
        off = np.zeros(T.num_tiles, bool)
        off[np.flatnonzero(sees)[::2]] = True
        T.set_active_tiles(~off)
        o = s.orbit_init()
        s.orbit_events(o, [("left", 12, -4)])
        T.set_camera(s)
        T.reset_image()
        T.render(1, 8)
        img = T.read_image()
        with pt.Tracer(s) as F:                                      # the new view, never masked
            F.render(1, 8)
            full = F.read_image()
        assert full[off[tile]].any() and not img[off[tile]].any()    # they would have received light; they received nothing
        lit = np.array([full[tile == t].any() for t in range(T.num_tiles)])
        assert all(img[tile == t].any() for t in np.flatnonzero(lit & ~off)) and not img[~lit[tile]].any()


def _view_with_a_lit_last_tile(pt):
    """cornell.txt at 97 x 61, zoomed in until the 29 pixels of the last tile (the end of the last row) receive light: at least 8 of them
    within 16 iterations, so that 16 more change the tile for certain"""
    for zoom in (0, -40, -80, -160, -320):
        s = _scene(pt, "cornell.txt", ODD)
        if zoom:
            s.orbit_events(s.orbit_init(), [("right", zoom)])
        with pt.Tracer(s) as T:
            T.render(1, 16)
            if T.read_image()[tile_of_pixel(pt, T) == T.num_tiles - 1].any(1).sum() >= 8:
                return s
    raise AssertionError("no view lights the last tile")


@pytest.mark.parametrize("only_last", [False, True])
def test_partial_last_tile(gpu_product, only_last):
    """97 x 61: the last tile has 29 pixels; switched off alone, and active alone"""
    pt = gpu_product
    s = _view_with_a_lit_last_tile(pt)
    with pt.Tracer(s) as T:
        tile = tile_of_pixel(pt, T)
        last = T.num_tiles - 1
        assert T.num_tiles == -(-ODD[0] * ODD[1] // pt.tile_pixels()) and 0 < (tile == last).sum() < pt.tile_pixels()
        T.render(1, 16)
        before = T.read_image()
        active = np.zeros(T.num_tiles, bool)
        active[last] = True
        if not only_last:
            active = ~active
        T.set_active_tiles(active)
        T.render(17, 16)
        after = T.read_image()
        assert beq(after[~active[tile]], before[~active[tile]]) and before[~active[tile]].any()
        lit = np.array([before[tile == t].any(1).sum() >= 8 for t in range(T.num_tiles)])
        assert lit[last] and lit[active].any() and all(not beq(after[tile == t], before[tile == t]) for t in np.flatnonzero(lit & active))
        assert aux_nonzero(T)[:2] == [0, 0]


def test_refusals_leave_the_tracer_usable(gpu_product):
    pt = gpu_product
    INVALID, UNSUPPORTED = 1, 5
    s = _scene(pt, "cornell.txt", (96, 64))
    for opt, ntiles_off, code, what in ((dict(no_cull=1), 0, UNSUPPORTED, "table"), (dict(antialiasing=0), 0, UNSUPPORTED, "cache"),
                                        (dict(tile_rows=8, tile_rank=0, tile_world=2), 0, INVALID, "row tile"), (dict(), 1, INVALID, "ntiles"),
                                        (dict(), -1, INVALID, "ntiles")):
        with pt.Tracer(s, **opt) as T, pt.Tracer(s, **opt) as N:
            n = T.num_tiles + ntiles_off
            m = np.zeros(n + 1, np.uint8)
            rc = T.lib.ptx_set_active_tiles(T.h, m.ctypes.data_as(ctypes.c_void_p), n)
            assert rc == code and what in T.lib.ptx_last_error().decode(), (opt, rc, T.lib.ptx_last_error())
            T.clear_active_tiles()                                   # no mask: a no-op
            for X in (T, N):
                X.render(1, 3)
            assert beq(T.read_image(), N.read_image()) and T.read_image().any(), opt
    with pt.Tracer(s) as T:
        assert T.lib.ptx_set_active_tiles(T.h, None, T.num_tiles) == INVALID
        assert T.lib.ptx_set_active_tiles(None, None, 1) == INVALID and T.lib.ptx_clear_active_tiles(None) == INVALID
        assert T.lib.ptx_num_tiles(None) == 0


def unbiased_setup(pt, s, T):
    """(mask with every second geometry-seeing tile off, the pixels of the active tiles that see geometry)"""
    sees = _sees(pt, s, T)
    off = np.zeros(T.num_tiles, bool)
    off[np.flatnonzero(sees)[::2]] = True
    return ~off, (sees & ~off)[tile_of_pixel(pt, T)]


def reference_frame(T):
    """4096 iterations on numbers no run below uses"""
    T.reset_image()
    T.render(100001, 4096)
    return T.read_image().astype(np.float64) / 4096


def mse_of_run(T, first, pixels, ref):
    T.reset_image()
    T.render(first, 64)
    return float(((T.read_image().astype(np.float64) / 64 - ref)[pixels] ** 2).mean())


def mse_of_unmasked_runs(pt):
    """the measurement behind WORST_UNMASKED_RATIO: 8 unmasked runs of 64 iterations on disjoint ranges"""
    s = _scene(pt, "cornell.txt", WIDE)
    with pt.Tracer(s) as T:
        _, pixels = unbiased_setup(pt, s, T)
        ref = reference_frame(T)
        return [mse_of_run(T, 1001 + 64 * j, pixels, ref) for j in range(8)]


def test_active_pixels_are_unbiased(gpu_product):
    """64 iterations with half of the geometry-seeing tiles masked against 64 unmasked ones on other iteration numbers, both against a
    4096-iteration frame, over the masked run's active pixels: the ratio of the mean squared errors stays below the largest ratio two
    unmasked runs showed, times 1.25.  A mask that cost the active pixels a share of their light, or gave them a neighbour's, would move
    the squared error by the square of that share of the signal -- orders above the sampling noise's own spread."""
    pt = gpu_product
    s = _scene(pt, "cornell.txt", WIDE)
    with pt.Tracer(s) as T:
        mask, pixels = unbiased_setup(pt, s, T)
        ref = reference_frame(T)
        unmasked = mse_of_run(T, 65, pixels, ref)
        T.set_active_tiles(mask)
        masked = mse_of_run(T, 1, pixels, ref)
    print("MSE over %d active pixels: masked %.6g, unmasked %.6g, ratio %.4f (bound %.4f)" % (pixels.sum(), masked, unmasked, masked / unmasked, BOUND))
    assert masked / unmasked <= BOUND
