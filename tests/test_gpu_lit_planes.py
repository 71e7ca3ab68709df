"""The per-iteration "lit" bit-planes and the per-bounce totals are cleared by the kernels that read them (k_gather, k_stats), not by
a fill in front of every launch set.  These tests check the invariant that replaces the fill -- both are zero whenever no set is in
flight (ptx_debug_aux_nonzero) -- and that the paths which break it (traced-ahead work dropped unfinished, an image reset, a camera
change) leave no stale bit behind: a stale bit would add an old iteration's radiance to a frame."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, beq


def aux_nonzero(T):
    """[nonzero plane words, nonzero totals words, lanes marked for a full clear before their next set]"""
    L = T.lib
    L.ptx_debug_aux_nonzero.restype = C.c_int
    L.ptx_debug_aux_nonzero.argtypes = [C.c_void_p, C.c_void_p]
    out = np.zeros(3, np.int64)
    assert L.ptx_debug_aux_nonzero(T.h, out.ctypes.data_as(C.c_void_p)) == 0
    return out.tolist()


def make_scene(pt, name="cornellObj.txt", res=(96, 72), depth=5):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,batch,aa", [(1, 4, 1), (3, 4, 1), (3, 5, 0), (1, 6, 0)])
def test_planes_and_totals_zero_between_sets(gpu_product, lanes, batch, aa):
    """After bulk renders of one and several launch sets (aa 0: the first-bounce cache fills, then replays its light hits into the
    planes), nothing is left in the planes or totals of any lane that has run a set, and the frame is the one-at-a-time frame."""
    pt = gpu_product
    s = make_scene(pt)
    with pt.Tracer(s, lanes=lanes, batch=batch, antialiasing=aa) as T, pt.Tracer(s, lanes=1, batch=1, antialiasing=aa) as R:
        it = 1
        for count in (1, batch, 3 * batch + 1, 2):
            T.render(it, count)
            R.render(it, count)
            it += count
            nz = aux_nonzero(T)
            assert nz[0] == 0 and nz[1] == 0, (count, nz)
            assert nz[2] < lanes, nz          # (lanes that have not run a set yet keep the mark they were created with)
        assert beq(T.read_image(), R.read_image())
        assert T.stats()["rays_per_bounce"] == R.stats()["rays_per_bounce"]


@pytest.mark.gpu
@pytest.mark.parametrize("aa", [1, 0])
def test_render_ahead_leaves_gathered_segments_zero(gpu_product, aa):
    """Render-ahead gathers a traced-ahead batch one segment per call: every segment it has gathered is zero again, call by call,
    across batch boundaries; switching it off drops the rest, and the next set on those lanes starts from a full clear."""
    pt = gpu_product
    s = make_scene(pt)
    with pt.Tracer(s, batch=4, antialiasing=aa) as T, pt.Tracer(s, batch=4, antialiasing=aa) as R:
        T.set_render_ahead(True)
        for it in range(1, 15):
            T.pathtrace(it)
            R.pathtrace(it)
            nz = aux_nonzero(T)
            assert nz[0] == 0 and nz[1] == 0, (it, nz)
        T.set_render_ahead(False)                       # lanes 1 and 2 still held traced-ahead segments: dropped
        assert aux_nonzero(T)[2] >= 1
        T.render(15, 12)
        R.render(15, 12)
        nz = aux_nonzero(T)
        assert nz[0] == 0 and nz[1] == 0, nz
        assert beq(T.read_image(), R.read_image())


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["reset", "camera", "jump"])
def test_abandoned_ahead_work_leaves_no_stale_bits(gpu_product, how):
    """Render-ahead traces the next batches on lanes 1 and 2; the caller then resets the image, moves the camera or jumps in the
    iteration number, and renders.  The frame equals a fresh tracer's that did only the last part."""
    pt = gpu_product
    s = make_scene(pt)
    with pt.Tracer(s, batch=4) as T:
        T.set_render_ahead(True)
        for it in range(1, 7):                          # lane 1's batch half gathered, lane 2's traced and untouched
            T.pathtrace(it)
        if how == "camera":
            o = s.orbit_init()
            s.orbit_events(o, [("left", 25, -10), ("right", 15)])
            T.set_camera(s)
        T.reset_image()
        if how == "jump":
            for it in range(1, 4):                      # served by a new ahead batch started at 1
                T.pathtrace(it)
            T.set_render_ahead(False)
            T.render(4, 13)
        else:
            T.render(1, 16)
        img = T.read_image()
        st = T.stats()
    with pt.Tracer(s, batch=4) as F:
        F.render(1, 16)
        ref = F.read_image()
        sf = F.stats()
    assert beq(img, ref)
    assert st["rays_per_bounce"] == sf["rays_per_bounce"] and st["iterations"] == sf["iterations"]
