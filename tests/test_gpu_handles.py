"""GPU: the life of the four post-processing handles (ptx_temporal, ptx_moments, ptx_adaptive, ptx_display) on a device: the upper end
of the ordinal check, a handle destroyed with its event recorded and nothing read, the next handle made right after it, and the
buffers a handle allocates on first use going with it.  8 x 8 and 70 x 5 pixels: the second is wider than one 64-pixel row segment
and its 350 pixels are not a multiple of the tile size.  What the handles compute is held by the suites of their own
(test_gpu_temporal.py, test_gpu_moments.py, test_gpu_adaptive.py, test_gpu_display.py); the refusals without a device by
test_handles_cpu.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (70, 5)]            # (W, H)
KINDS = ("temporal", "moments", "adaptive", "display")


def _frame(w, h, seed=5):
    return (0.05 + 0.95 * np.random.default_rng(seed).random((h, w, 3))).astype(np.float32)


def _scene(pt, w, h):
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"), res=(w, h), depth=4)
    s.apply_runcuda_camera()
    return s


@pytest.mark.parametrize("kind", KINDS)
def test_ordinal_at_the_device_count_is_refused_and_the_next_create_succeeds(gpu_product, kind):
    lib = gpu_product.load_library()
    create, destroy = getattr(lib, "ptx_%s_create" % kind), getattr(lib, "ptx_%s_destroy" % kind)
    ndev = lib.ptx_device_count()
    for w, h in SIZES:
        out = ctypes.c_void_p(0xDEAD0)
        assert create(ndev, w, h, ctypes.byref(out)) == 1
        assert lib.ptx_last_error().decode() == "ptx_%s_create: device ordinal out of range" % kind and out.value is None
        assert create(0, w, h, ctypes.byref(out)) == 0 and out.value
        destroy(out)


@pytest.mark.parametrize("size", SIZES)
def test_moments_handle_destroyed_unread_and_made_again(gpu_product, size):
    pt = gpu_product
    w, h = size
    f = _frame(w, h)
    m = pt.Moments(0, w, h)
    m.add_host(4 * f, 4)                                 # records the handle's event; d_stage allocated on this first use
    m.close()
    with pt.Moments(0, w, h) as m:
        m.add_host(4 * f, 4)
        m.add_host(12 * f, 8)
        r = m.read()
    assert r["samples"] == 8 and (r["batches"] == 2).all()
    assert np.allclose(r["mean"], 1.5 * f, rtol=1e-6, atol=0)      # two batch means, f and 2 f, of equal weight


@pytest.mark.parametrize("size", SIZES)
def test_moments_tiled_add_allocates_on_first_use_and_goes_with_the_handle(gpu_product, size):
    pt = gpu_product
    w, h = size
    nt = -(-w * h // pt.tile_pixels())
    assert nt == (1 if size == (8, 8) else 2)
    f = _frame(w, h)
    m = pt.Moments(0, w, h)
    m.add_host_tiled(3 * f, np.full(nt, 3))              # d_stage and the (k, W') table: both allocated here
    m.close()
    with pt.Moments(0, w, h) as m:
        m.add_host_tiled(3 * f, np.full(nt, 3))
        assert (m.read_samples() == 3).all()
        r = m.read()
    assert (r["batches"] == 1).all() and np.allclose(r["mean"], f, rtol=1e-6, atol=0)


@pytest.mark.parametrize("size", SIZES)
def test_display_handle_destroyed_unread_and_made_again(gpu_product, size):
    pt = gpu_product
    w, h = size
    f = _frame(w, h)
    d = pt.Display(w, h)
    first = d.host(f)                                    # (host returns the codes: the handle's own read stays unused)
    d.close()
    with pt.Display(w, h) as d:
        again = d.host(f)
        assert beq(d.read(), again)
    assert beq(first, again) and again[..., :3].any() and not again[..., 3].any()      # (alpha 0)


@pytest.mark.parametrize("size", SIZES)
def test_display_float_frame_allocates_on_first_use_and_goes_with_the_handle(gpu_product, size):
    pt = gpu_product
    w, h = size
    f = _frame(w, h)
    d = pt.Display(w, h)
    d.host(f, keep_float=1)                              # d_float (and d_stage): first use
    d.close()
    with pt.Display(w, h) as d:
        codes = d.host(f, keep_float=1, meter="manual", tone="clamp", transfer="linear")
        z, own = d.read(float_frame=True)
    assert beq(own, codes) and beq(z, np.minimum(f, np.float32(1)))      # exposure 1, clamp, linear: z is the frame itself


@pytest.mark.parametrize("size", SIZES)
def test_temporal_handle_destroyed_unread_and_made_again(gpu_product, size):
    pt = gpu_product
    w, h = size
    spp = 2
    with pt.Tracer(_scene(pt, w, h)) as T:
        T.render(1, spp)
        c = (T.read_image().reshape(h, w, 3) / np.float32(spp)).astype(np.float32)
        tm = pt.Temporal(0, w, h)
        first = T.denoise_temporal(tm, spp)
        tm.close()
        want = T.denoise(spp)
        with pt.Temporal(0, w, h) as tm:
            again = T.denoise_temporal(tm, spp)
            r = tm.read()
    assert beq(first, want) and beq(again, want)         # no history either time: ptx_denoise's bits
    assert not r["count"].any() and not r["history"].any() and beq(r["mix"], c)      # ... and the mix is the frame


@pytest.mark.parametrize("size", SIZES)
def test_adaptive_handle_destroyed_unread_and_made_again(gpu_product, size):
    pt = gpu_product
    w, h = size
    k = 2
    with pt.Tracer(_scene(pt, w, h)) as T:
        T.render(1, k)
        a, m = pt.Adaptive(0, w, h), pt.Moments(0, w, h)
        a.add(m, T, k)                                   # both handles' events recorded on the tracer's stream
        a.close()
        m.close()
        with pt.Adaptive(0, w, h) as a, pt.Moments(0, w, h) as m:
            a.add(m, T, k)
            a.resolve(T)
            r = a.read()
            assert (m.read_samples() == k).all()
        img = T.read_image().reshape(h, w, 3)
    assert (r["samples"] == k).all() and r["tile_active"].all()
    assert beq(r["mean"], img / np.float32(k))
