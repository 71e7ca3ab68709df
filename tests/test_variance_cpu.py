"""CPU: the variance guidance's definition (tests/variance_ref.py checked on synthetic data and against tests/atrous_ref.py), its C-ABI
surface without a device, and what the compiler made of its kernels.  The device is held to the same restatement by
tests/test_gpu_variance.py."""
import ctypes

import numpy as np
import pytest

from atrous_ref import atrous, random_frame
from resource_usage import kernels_named, resource_usage
from variance_ref import atrous_variance, denoise_buffers_variance, lum, spatial_variance, update



@pytest.mark.parametrize("batches", [[2] * 8, [2, 2, 2, 64], [1, 7, 3, 20, 2]])
def test_estimator_is_unbiased_whatever_the_batch_sizes(batches):
    """iid samples of variance 4 around 3: after the batches, mean V is the per-sample variance and mean V / n the squared error of the
    mix, whatever each call's spp (the first batch's V comes from elsewhere -- the spatial estimate -- so it is seeded with the truth)"""
    rng = np.random.default_rng(sum(batches))
    P, sigma2 = 200000, 4.0
    n, m, V = 0.0, None, None
    for s in batches:
        l = 3.0 + rng.standard_normal((P, s)).mean(1) * np.sqrt(sigma2)
        if m is None:
            n, m, V = float(s), l, np.full(P, sigma2)
        else:
            V = update(V, m, n, l, float(s))
            m = (n * m + s * l) / (n + s)
            n += s
    err2 = ((m - 3.0) ** 2).mean()
    print("batches %s: mean V %.4f (truth %.1f), mean V/n %.5f, squared error of the mix %.5f" % (batches, V.mean(), sigma2, (V / n).mean(), err2))
    assert abs(V.mean() - sigma2) <= 0.02 * sigma2
    assert abs((V / n).mean() - err2) <= 0.02 * err2


def _flat(h, w):
    """flat geometry: one normal, one position, every pixel a hit"""
    n = np.zeros((h, w, 3)); n[..., 2] = 1.0
    return n, np.zeros((h, w, 3)), np.ones((h, w), bool)


def test_zero_variance_and_distinct_luminances_give_the_input_back():
    h, w = 20, 23
    n, x, hit = _flat(h, w)
    # every pixel its own grey level, 0.1 apart: any two different taps differ by >= 0.1
    grey = (np.arange(h * w, dtype=np.float64).reshape(h, w) * 0.1)
    col = np.repeat(grey[..., None], 3, -1)
    out, v = atrous_variance(col, np.zeros((h, w)), n, x, hit, passes=4, epsilon=1e-4)     # exp(-0.1 / 1e-4) = exp(-1000) = 0
    # (a tap clamped onto the pixel itself counts again with weight b b: sum w c / sum w is then c up to a rounding)
    assert np.allclose(out, col, rtol=1e-14, atol=0) and np.array_equal(out[8:-8, 8:-8], col[8:-8, 8:-8]) and not v.any()


def test_constant_frame_scales_the_variance_by_sum_b_squared():
    h, w, v0 = 40, 44, 0.37
    n, x, hit = _flat(h, w)
    col = np.full((h, w, 3), 0.8)
    for passes in (1, 2, 3):
        out, v = atrous_variance(col, np.full((h, w), v0), n, x, hit, passes=passes)
        m = 2 * (2 ** passes - 1)                                     # the footprint's half width: the interior is beyond it
        assert np.allclose(out, col, rtol=0, atol=1e-15)
        assert np.allclose(v[m:-m, m:-m], v0 * (35.0 / 128) ** (2 * passes), rtol=1e-12)     # sum b^2 = 35/128 per axis


def test_huge_variance_is_the_plain_filter_without_a_colour_weight():
    f = random_frame(37, 41, seed=5)
    for demod in (0, 1):
        want = atrous(f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"], 3, demod, 1e30, 0.1, 0.5)
        got, _, _ = denoise_buffers_variance(f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"], variance=np.full((37, 41), 1e30),
                                             passes=3, demodulate=demod)
        assert np.allclose(got, want, rtol=1e-9, atol=1e-12)


def test_spatial_variance_by_hand():
    h, w = 9, 11
    n, x, hit = _flat(h, w)
    rng = np.random.default_rng(1)
    col = rng.random((h, w, 3))
    # flat geometry: every weight is 1, so var_s is the plain variance of the clamped window's luminances
    got = spatial_variance(col, n, x, hit, None, radius=2)
    l = lum(col)
    for (y, xx) in ((0, 0), (4, 5), (8, 10), (3, 0)):
        win = [l[min(max(y + dy, 0), h - 1), min(max(xx + dx, 0), w - 1)] for dy in range(-2, 3) for dx in range(-2, 3)]
        assert np.isclose(got[y, xx], np.var(win), rtol=1e-12)
    # a tap of another geom or material, or a miss, weighs nothing
    ids = np.zeros((h, w, 2), np.int32)
    ids[:, 6:, 1] = 1
    hit2 = hit.copy(); hit2[4, 4] = False
    got = spatial_variance(col, n, x, hit2, ids, radius=1)
    win = [l[yy, xq] for yy in (3, 4, 5) for xq in (4, 5) if (yy, xq) != (4, 4)]
    assert np.isclose(got[4, 5], np.var(win), rtol=1e-12) and got[4, 4] == 0.0


def test_variance_params_struct_and_defaults(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    assert lib.ptx_sizeof_variance_params() == ctypes.sizeof(api.VarianceParams) == 16
    p = product.default_variance_params()
    # the documented defaults (include/mi355x_pathtracer.h)
    assert (p.phi_luminance, p.epsilon) == tuple(float(np.float32(v)) for v in (4.0, 1e-4))
    assert (p.spatial_radius, p.prefilter) == (3, 1)
    q = product.default_variance_params(phi_luminance=2, prefilter=0)
    assert (q.phi_luminance, q.prefilter, q.spatial_radius) == (2.0, 0, 3)
    with pytest.raises(AttributeError):
        product.default_variance_params(bogus=1)


def test_bad_variance_arguments_raise_before_any_device_work(product):
    lib = product.load_library()
    err = lambda: lib.ptx_last_error().decode()
    fake = ctypes.c_void_p(8)                                # never dereferenced: every call below is refused on its arguments
    for bad, what in ((dict(phi_luminance=0.0), "phi_luminance"), (dict(phi_luminance=float("nan")), "phi_luminance"),
                      (dict(epsilon=0.0), "epsilon"), (dict(epsilon=float("inf")), "epsilon"),
                      (dict(spatial_radius=0), "spatial_radius"), (dict(spatial_radius=4), "spatial_radius")):
        vp = product.default_variance_params(**bad)
        assert lib.ptx_denoise_variance(None, None, None, None, ctypes.byref(vp), 1) == 1, bad     # PTX_ERR_INVALID
        assert what in err(), (bad, err())
        z = np.zeros(3, np.float32)
        ptr = z.ctypes.data_as(ctypes.c_void_p)
        assert lib.ptx_denoise_buffers_variance(0, 1, 1, ptr, ptr, ptr, ptr, ptr, None, None, None, ctypes.byref(vp), ptr, None) == 1
        assert what in err(), (bad, err())
    bad_dp = product.default_denoise_params(passes=0)
    assert lib.ptx_denoise_variance(None, None, ctypes.byref(bad_dp), None, None, 1) == 1 and "passes" in err()
    bad_tp = product.default_temporal_params(max_history=-1)
    assert lib.ptx_denoise_variance(None, None, None, ctypes.byref(bad_tp), None, 1) == 1 and "max_history" in err()
    assert lib.ptx_denoise_variance(None, None, None, None, None, 0) == 1 and "spp" in err()
    no_demod = product.default_denoise_params(demodulate=0)
    assert lib.ptx_denoise_variance(None, fake, ctypes.byref(no_demod), None, None, 1) == 1 and "demodulate" in err()
    assert lib.ptx_denoise_variance(None, None, None, None, None, 1) == 1 and "null" in err()
    assert lib.ptx_read_variance(None, None, None) == 1
    f = random_frame(4, 5, seed=0)
    with pytest.raises(product.PathTracerError, match="alb3"):
        product.denoise_buffers_variance(f["rgb"], None, f["normal"], f["position"], f["hit"])
    with pytest.raises(product.PathTracerError, match="frame size"):
        product.denoise_buffers_variance(np.zeros((0, 4, 3)), None, np.zeros((0, 4, 3)), np.zeros((0, 4, 3)), np.zeros((0, 4)), demodulate=0)
    with pytest.raises(TypeError, match="bogus"):
        product.denoise_buffers_variance(f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"], bogus=1)


def test_variance_filter_has_no_cpu_fallback(product):
    if product.load_library().ptx_device_count() > 0:
        pytest.skip("a HIP device is present")
    f = random_frame(4, 5, seed=0)
    with pytest.raises(product.PathTracerError, match=r"code 4\).*no HIP device"):
        product.denoise_buffers_variance(f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"])


def test_variance_kernels_do_not_spill():
    found = kernels_named(resource_usage("resource-usage-denoise"),
                          ("k_atrous_prep", "k_variance_prep_state", "k_variance_spatial", "k_atrous_passILb1ELb0EE", "k_atrous_passILb1ELb1EE"))
    found.update(kernels_named(resource_usage("resource-usage-temporal"), ("k_reproject_variance",)))
    assert len(found) == 6, list(found)          # two preps, the spatial estimate, two passes, the reprojection with V
    for k, v in found.items():
        assert v.get("scratch") == 0, (k, v)
    spatial = found["k_variance_spatial"]
    # 28 KB of LDS per workgroup, five workgroups (20 waves) per CU of 160 KiB
    assert spatial["lds"] <= 160 * 1024 // 5 and spatial["waves"] >= 5, spatial
