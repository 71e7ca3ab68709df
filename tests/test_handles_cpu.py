"""CPU: what the four post-processing handles (ptx_temporal, ptx_moments, ptx_adaptive, ptx_display) refuse at create, before any
device work -- the return code and the exact ptx_last_error text, one table for the four -- and the NULL-handle answers of their
destroy / reset / read; and the Python classes' ownership of a handle (close, __exit__, __del__) against a fake library that counts the
destroy calls.  The device side of create and destroy is tests/test_gpu_handles.py's."""
import ctypes
import gc

import pytest

INVALID, NODEVICE = 1, 4
CAP_W, CAP_H = 32768, 16384          # 536870912 pixels: one above INT_MAX / 4, below INT_MAX / 3

# kind -> (the no-device message's noun, the divisor of the unit's pixel cap)
HANDLES = {"temporal": ("the temporal denoiser", 3), "moments": ("the moments handle", 4), "adaptive": ("the adaptive handle", 4),
           "display": ("the display handle", 4)}


def _create(lib, kind, device, w, h, out):
    return getattr(lib, "ptx_%s_create" % kind)(device, w, h, out)


@pytest.mark.parametrize("kind", sorted(HANDLES))
def test_create_refusals_keep_their_order_codes_and_texts(product, kind):
    lib = product.load_library()
    err = lambda: lib.ptx_last_error().decode()
    fn = "ptx_%s_create" % kind
    noun, cap_div = HANDLES[kind]
    assert (1 << 31) - 1 == 2147483647 and CAP_W * CAP_H == 2147483647 // 4 + 1 and CAP_W * CAP_H <= 2147483647 // 3

    def refused(device, w, h):
        """(code, message) of a create whose `out` held a stale pointer going in; it is NULL coming out"""
        out = ctypes.c_void_p(0xDEAD0)
        rc = _create(lib, kind, device, w, h, ctypes.byref(out))
        assert out.value is None, (device, w, h)
        return rc, err()

    # out NULL comes first: the size and the ordinal beside it are bad too
    assert _create(lib, kind, -1, 0, 0, None) == INVALID and err() == fn + ": out is NULL"
    assert _create(lib, kind, 0, 4, 4, None) == INVALID and err() == fn + ": out is NULL"
    # the size before the ordinal
    assert refused(0, 0, 4) == (INVALID, fn + ": bad frame size")
    assert refused(0, 4, 0) == (INVALID, fn + ": bad frame size")
    assert refused(-1, 0, 4) == (INVALID, fn + ": bad frame size")
    assert refused(-1, -4, -4) == (INVALID, fn + ": bad frame size")
    assert refused(-1, 4, 4) == (INVALID, fn + ": device ordinal out of range")
    # the cap boundary, with an ordinal that is refused before any device is asked for: each unit keeps its own cap
    want = fn + (": bad frame size" if cap_div == 4 else ": device ordinal out of range")
    assert refused(-1, CAP_W, CAP_H) == (INVALID, want)
    assert refused(-1, CAP_H, CAP_W) == (INVALID, want)
    assert refused(-1, 1 << 16, 1 << 16) == (INVALID, fn + ": bad frame size")          # above every cap
    if lib.ptx_device_count() < 1:
        assert refused(0, 4, 4) == (NODEVICE, "no HIP device available; %s has no CPU path" % noun)
        assert refused(7, 4, 4) == (NODEVICE, "no HIP device available; %s has no CPU path" % noun)      # the count before the upper end


def test_null_handles_are_refused_with_their_codes_and_texts(product):
    lib = product.load_library()
    err = lambda: lib.ptx_last_error().decode()
    for kind in HANDLES:
        getattr(lib, "ptx_%s_destroy" % kind)(None)      # a no-op
    assert lib.ptx_temporal_reset(None) == INVALID and err() == "null temporal handle"
    assert lib.ptx_temporal_read(None, None, None, None) == INVALID and err() == "null temporal handle"
    assert lib.ptx_moments_reset(None) == INVALID and err() == "ptx_moments_reset: null moments handle"
    assert lib.ptx_moments_read(None, None, None, None, None) == INVALID and err() == "ptx_moments_read: null moments handle"
    buf = (ctypes.c_int32 * 4)()
    assert lib.ptx_moments_read_samples(None, buf) == INVALID and err() == "ptx_moments_read_samples: null moments handle or array"
    assert lib.ptx_adaptive_reset(None) == INVALID and err() == "ptx_adaptive_reset: null adaptive handle"
    assert lib.ptx_adaptive_read(None, None, None, None, None) == INVALID and err() == "ptx_adaptive_read: null adaptive handle"
    assert lib.ptx_adaptive_num_tiles(None) == 0 and not lib.ptx_adaptive_device_frame(None)
    assert lib.ptx_display_reset(None) == INVALID and err() == "ptx_display_reset: null display handle"
    assert lib.ptx_display_read(None, None, None) == INVALID and err() == "ptx_display_read: null display handle"
    fbuf = (ctypes.c_float * 4)()
    assert lib.ptx_display_read_blocks(None, fbuf) == INVALID and err() == "ptx_display_read_blocks: null display handle or array"


class FakeLib:
    """any ptx_*_destroy / ptx_scene_free / ptx_destroy: counts the calls per (function, handle)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not (name.endswith("destroy") or name.endswith("free")):
            raise AttributeError(name)
        return lambda h: self.calls.append((name, h))


OWNERS = {"Temporal": "ptx_temporal_destroy", "Moments": "ptx_moments_destroy", "Adaptive": "ptx_adaptive_destroy",
          "Display": "ptx_display_destroy", "Tracer": "ptx_destroy", "Scene": "ptx_scene_free", "MultiTracer": "ptx_multi_destroy"}


def _owner(api, name, lib, handle):
    """an instance as its __init__ leaves it after a successful create, without a create"""
    obj = getattr(api, name).__new__(getattr(api, name))
    obj.lib, obj.h = lib, handle
    return obj


@pytest.mark.parametrize("name", sorted(OWNERS))
def test_python_owners_destroy_a_handle_once(name):
    from mygpuraytracer_amd import api
    lib, destroy = FakeLib(), OWNERS[name]
    obj = _owner(api, name, lib, 101)
    obj.close()
    assert lib.calls == [(destroy, 101)] and obj.h is None
    obj.close()                                          # idempotent
    obj.__del__()
    assert lib.calls == [(destroy, 101)]
    del obj
    gc.collect()
    assert lib.calls == [(destroy, 101)]
    # dropped without a close: __del__ alone
    obj = _owner(api, name, lib, 102)
    del obj
    gc.collect()
    assert lib.calls == [(destroy, 101), (destroy, 102)]
    # a half-made instance (create failed before `h` was set) is dropped without a call
    half = getattr(api, name).__new__(getattr(api, name))
    half.lib = lib
    half.h = None
    half.close()
    del half
    gc.collect()
    assert len(lib.calls) == 2
    if hasattr(getattr(api, name), "__exit__"):
        with _owner(api, name, lib, 103) as o:
            assert o.h == 103
        assert lib.calls[2:] == [(destroy, 103)] and o.h is None
        o.close()
        del o
        gc.collect()
        assert lib.calls[2:] == [(destroy, 103)]
