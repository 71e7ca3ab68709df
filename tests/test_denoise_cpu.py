"""CPU: the denoiser's definition (tests/atrous_ref.py checked by hand), its C-ABI surface without a device, and what the compiler made of
its kernels.  The device is held to the same restatement by tests/test_gpu_denoise.py."""
import ctypes

import numpy as np
import pytest

from atrous_ref import atrous, bspline_atrous, random_frame
from resource_usage import kernels_named, resource_usage

BIG = 1e30


def test_constant_image_is_a_fixed_point():
    f = random_frame(23, 31, 1)
    c0 = float(np.float32(0.37))
    rgb = np.full_like(f["rgb"], c0)
    out = atrous(rgb, f["albedo"], f["normal"], f["position"], f["hit"], 5, False, 4.0, 0.1, 0.5)
    assert np.abs(out - c0).max() < 1e-12
    # demodulated, the filtered quantity is colour / albedo: constant (and so a fixed point) when the albedo is
    out = atrous(rgb, np.full_like(f["albedo"], 0.5), f["normal"], f["position"], f["hit"], 5, True, 4.0, 0.1, 0.5)
    assert np.abs(out - c0).max() < 1e-12


def test_infinite_phis_give_the_b3_spline_convolution():
    rng = np.random.default_rng(2)
    for h, w in ((19, 40), (1, 7), (33, 2)):
        rgb = rng.random((h, w, 3))
        f = random_frame(h, w, 3)
        allhit = np.ones((h, w), bool)
        for passes in (1, 3, 5):
            out = atrous(rgb, f["albedo"], f["normal"], f["position"], allhit, passes, False, BIG, BIG, BIG)
            assert np.abs(out - bspline_atrous(rgb, passes)).max() < 1e-12, (h, w, passes)


def test_miss_pixels_are_untouched():
    f = random_frame(40, 50, 4)
    for demod in (False, True):
        out = atrous(f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"], 5, demod, 4.0, 0.1, 0.5)
        miss = ~f["hit"]
        assert miss.sum() > 100
        assert np.array_equal(out[miss], f["rgb"][miss].astype(np.float64))
        assert not np.array_equal(out[f["hit"]], f["rgb"][f["hit"]].astype(np.float64))


def test_two_pixel_normal_edge_does_not_blur_with_small_phi_normal():
    h, w = 24, 40
    n = np.zeros((h, w, 3)); n[..., 2] = 1.0
    n[:, 20:22] = [1.0, 0.0, 0.0]                     # a 2-pixel-wide stripe facing elsewhere
    rgb = np.zeros((h, w, 3)); rgb[:, 20:22] = 1.0
    pos, alb, hit = np.zeros((h, w, 3)), np.ones((h, w, 3)), np.ones((h, w), bool)
    sharp = atrous(rgb, alb, n, pos, hit, 5, False, BIG, 1e-4, BIG)
    assert np.abs(sharp - rgb).max() < 1e-12
    blurred = atrous(rgb, alb, n, pos, hit, 5, False, BIG, BIG, BIG)      # the same stripe without the normal weight does spread
    assert blurred[:, 20:22].max() < 0.6 and blurred[:, 10].min() > 1e-3


def test_denoise_params_struct_and_defaults(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    assert lib.ptx_sizeof_denoise_params() == ctypes.sizeof(api.DenoiseParams) == 20
    p = product.default_denoise_params()
    # the documented defaults (include/mi355x_pathtracer.h)
    assert (p.passes, p.demodulate) == (5, 1)
    assert (p.phi_color, p.phi_normal, p.phi_position) == tuple(float(np.float32(v)) for v in (16.0, 0.1, 0.5))
    q = product.default_denoise_params(passes=3, phi_color=2)
    assert (q.passes, q.phi_color, q.phi_normal) == (3, 2.0, p.phi_normal)


def test_bad_denoise_arguments_raise_before_any_device_work(product):
    f = random_frame(4, 5, 5)
    args = (f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"])
    for bad in (dict(passes=0), dict(passes=11), dict(phi_color=0.0), dict(phi_normal=-1.0), dict(phi_position=float("nan"))):
        with pytest.raises(product.PathTracerError, match="ptx_denoise_params"):
            product.denoise_buffers(*args, **bad)
    with pytest.raises(product.PathTracerError, match="alb3"):
        product.denoise_buffers(f["rgb"], None, f["normal"], f["position"], f["hit"])


def test_denoise_buffers_has_no_cpu_fallback(product):
    if product.load_library().ptx_device_count() > 0:
        pytest.skip("a HIP device is present")
    f = random_frame(6, 7, 6)
    with pytest.raises(product.PathTracerError, match="no HIP device"):
        product.denoise_buffers(f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"])


PASSES = tuple("k_atrous_passILb%dELb%dEE" % (var, last) for var in (0, 1) for last in (0, 1))


def test_denoiser_kernels_do_not_spill():
    filt = kernels_named(resource_usage("resource-usage-denoise"), ("k_atrous_prep",) + PASSES)
    assert len(filt) == 5, list(filt)                 # prep + the four instances of the pass
    gbuf = kernels_named(resource_usage("resource-usage"), ("k_gbuffer",))
    for k, v in {**filt, **gbuf}.items():
        assert v["scratch"] == 0, (k, v)
    for k in PASSES[:2]:
        assert filt[k]["lds"] == 0, (k, filt[k])      # the plain instances: no prefilter tile
