"""CPU: the temporal reuse's definition (tests/temporal_ref.py checked by hand on synthetic frames), its C-ABI surface without a device,
and what the compiler made of its kernel.  The device is held to the same restatement by tests/test_gpu_temporal.py."""
import ctypes

import numpy as np
import pytest

from resource_usage import kernels_named, resource_usage
from temporal_ref import mix, plane_gbuffer, project, reproject, state, synthetic_camera



def _plane_frames(shift_px=(3, 2), W=64, H=48, seed=0):
    """the plane z = 0 seen from a camera at z = 8 and from the same camera moved parallel to it so that current pixel (x, y) sees
    what previous pixel (x + dx, y + dy) saw: previous state (random D, n = 3) and the current G-buffer"""
    prev_cam = synthetic_camera(W, H, position=(0.0, 0.0, 8.0), pl=1.0 / 128)
    step = 8.0 / 128                                          # one pixel on the plane
    cur_cam = synthetic_camera(W, H, position=(-shift_px[0] * step, -shift_px[1] * step, 8.0), pl=1.0 / 128)
    rng = np.random.default_rng(seed)
    prev = state(plane_gbuffer(prev_cam), rng.random((H, W, 3)) * 2, np.full((H, W), 3.0))
    return prev_cam, cur_cam, prev, plane_gbuffer(cur_cam)


def test_projection_inverts_the_pixel_centre_ray():
    cam = synthetic_camera(40, 30)
    cam["right"] = np.array([2.0, 0.3, 0.0])                 # not orthonormal, as runCuda leaves them
    cam["up"] = np.array([0.1, 0.7, 0.2])
    g = plane_gbuffer(cam, z=-3.0)
    s, u, v = project(cam, g["position"])
    y, x = np.mgrid[0:30, 0:40]
    assert np.abs(u - x).max() < 1e-9 and np.abs(v - y).max() < 1e-9 and (s > 0).all()


def test_translation_by_whole_pixels_shifts_d():
    prev_cam, cur_cam, prev, cur = _plane_frames((3, 2))
    h, nh, _ = reproject(prev_cam, cur, prev, [False, False], max_history=16)
    H, W = nh.shape
    got = h[:H - 2, :W - 3] / 0.5                            # back to D: the albedo is 0.5
    assert np.abs(got - prev["D"][2:, 3:]).max() < 1e-6
    assert np.allclose(nh[:H - 2, :W - 3], 3.0)
    assert not nh[:, W - 2:].any() and not nh[H - 1:].any()  # their taps lie outside the previous frame


def test_rejections():
    prev_cam, cur_cam, prev, cur = _plane_frames((3, 2))
    _, base_n, _ = reproject(prev_cam, cur, prev, [False, False])
    assert (base_n[10:20, 10:20] == 3.0).all()

    def changed(what, value=None):
        pg = {k: np.array(v, copy=True) for k, v in prev["gbuf"].items()}
        if what == "normal":
            pg["normal"][..., 2] = -1.0                       # flipped
        elif what == "position":
            pg["position"][..., 2] += value                   # offset along the normal
        else:
            pg[what][:] = value
        return dict(prev, gbuf=pg)

    for what, value in (("geom", 7), ("material", 0), ("normal", None), ("position", 0.2), ("hit", False)):
        _, nh, _ = reproject(prev_cam, cur, changed(what, value), [False, False])
        assert not nh.any(), what
    # an offset within plane_tolerance * distance (0.01 * ~8) is accepted
    _, nh, _ = reproject(prev_cam, cur, changed("position", 0.05), [False, False])
    assert np.array_equal(nh, base_n)
    # a specular material inherits nothing unless specular_history
    _, nh, _ = reproject(prev_cam, cur, prev, [False, True])
    assert not nh.any()
    _, nh, _ = reproject(prev_cam, cur, prev, [False, True], specular_history=1)
    assert np.array_equal(nh, base_n)


def test_behind_the_camera_and_off_frame_give_no_history():
    prev_cam, cur_cam, prev, cur = _plane_frames((0, 0))
    behind = dict(prev_cam, position=np.array([0.0, 0.0, -5.0]))          # z = 0 lies behind a camera at z = -5 looking down -z
    s, _, _ = project(behind, cur["position"])
    assert (s < 0).all()
    _, nh, _ = reproject(behind, cur, prev, [False, False], plane_tolerance=1e9)
    assert not nh.any()
    far = dict(prev_cam, position=np.array([100.0, 0.0, 8.0]))            # everything projects outside the frame
    _, nh, _ = reproject(far, cur, prev, [False, False], plane_tolerance=1e9)
    assert not nh.any()


def test_max_history_clamps_and_zero_means_no_history():
    prev_cam, cur_cam, prev, cur = _plane_frames((1, 1))
    prev = dict(prev, n=np.full_like(prev["n"], 40.0))
    _, nh, _ = reproject(prev_cam, cur, prev, [False, False], max_history=16)
    assert nh.max() == 16.0
    h, nh, _ = reproject(prev_cam, cur, prev, [False, False], max_history=0)
    assert not nh.any() and not h.any()


def test_no_history_mix_is_c_exactly():
    rng = np.random.default_rng(3)
    H, W = 12, 17
    rgb = (rng.random((H, W, 3)) * 7).astype(np.float32)
    hit = rng.random((H, W)) > 0.3
    nh = np.where(rng.random((H, W)) > 0.5, 5.0, 0.0)
    h = rng.random((H, W, 3))
    m, n, c32 = mix(rgb, 3, hit, h, nh)
    plain = (~hit) | (nh == 0)
    assert np.array_equal(m[plain], (rgb / np.float32(3)).astype(np.float64)[plain])
    assert (n[plain] == 3).all() and np.allclose(n[~plain], 8.0)
    assert np.allclose(m[~plain], ((3 * c32.astype(np.float64) + nh[..., None] * h) / (3 + nh[..., None]))[~plain])


def test_temporal_params_struct_and_defaults(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    assert lib.ptx_sizeof_temporal_params() == ctypes.sizeof(api.TemporalParams) == 16
    p = product.default_temporal_params()
    # the documented defaults (include/mi355x_pathtracer.h)
    assert (p.max_history, p.specular_history) == (16, 0)
    assert (p.normal_cos, p.plane_tolerance) == tuple(float(np.float32(v)) for v in (0.9, 0.01))
    q = product.default_temporal_params(max_history=4, normal_cos=0.5)
    assert (q.max_history, q.normal_cos, q.plane_tolerance) == (4, 0.5, p.plane_tolerance)
    with pytest.raises(AttributeError):
        product.default_temporal_params(bogus=1)


def test_bad_temporal_arguments_raise_before_any_device_work(product):
    lib = product.load_library()
    dp = product.default_denoise_params()
    err = lambda: lib.ptx_last_error().decode()
    for bad, what in ((dict(max_history=-1), "max_history"), (dict(normal_cos=1.5), "normal_cos"),
                      (dict(normal_cos=float("nan")), "normal_cos"), (dict(plane_tolerance=-0.1), "plane_tolerance"),
                      (dict(plane_tolerance=float("inf")), "plane_tolerance")):
        tp = product.default_temporal_params(**bad)
        assert lib.ptx_denoise_temporal(None, None, ctypes.byref(dp), ctypes.byref(tp), 1) == 1     # PTX_ERR_INVALID
        assert what in err(), (bad, err())
    bad_dp = product.default_denoise_params(passes=0)
    assert lib.ptx_denoise_temporal(None, None, ctypes.byref(bad_dp), None, 1) == 1 and "passes" in err()
    assert lib.ptx_denoise_temporal(None, None, None, None, 0) == 1 and "spp" in err()
    assert lib.ptx_denoise_temporal(None, None, None, None, 1) == 1 and "null" in err()
    for w, h in ((0, 4), (4, -1), (1 << 16, 1 << 16)):
        with pytest.raises(product.PathTracerError, match="frame size"):
            product.Temporal(0, w, h)
    with pytest.raises(product.PathTracerError, match="device"):
        product.Temporal(-1, 4, 4)
    assert lib.ptx_temporal_reset(None) == 1
    assert lib.ptx_temporal_read(None, None, None, None) == 1
    lib.ptx_temporal_destroy(None)                                          # a no-op


def test_temporal_create_has_no_cpu_fallback(product):
    if product.load_library().ptx_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(product.PathTracerError, match=r"code 4\).*no HIP device"):
        product.Temporal(0, 8, 8)


def test_temporal_kernel_does_not_spill():
    kernels = kernels_named(resource_usage("resource-usage-temporal"), ("k_temporal_reproject", "k_reproject_variance"))
    assert len(kernels) == 2, list(kernels)
    for k, v in kernels.items():
        assert v.get("scratch") == 0, (k, v)
