"""CPU: the pooled variance rule of ptx_denoise_temporal_measured (tests/temporal_measured_ref.py) as an estimator, on seeded synthetic
samples; its fall-back below min_batches; the inputs of the device's estimator test; the C-ABI surface without a device; and what the
compiler made of the new kernel.  The device is held to the same restatement by tests/test_gpu_temporal_measured.py."""
import ctypes

import numpy as np
import pytest

from moments_ref import LUM, Moments, quad
from resource_usage import kernels_named, resource_usage
from temporal_measured_ref import estimator_figures, estimator_samples, pooled, temporal_measured_variance
from temporal_ref import plane_gbuffer, state, synthetic_camera
from variance_ref import temporal_variance, update

N_PIXELS = 100000


def _draw(rng, kind, shape):
    """iid samples and their true variance"""
    if kind == "gaussian":
        return 1.0 + 0.5 * rng.standard_normal(shape), 0.25
    return (rng.random(shape) < 0.05).astype(np.float64), 0.05 * 0.95          # Bernoulli(0.05): heavy tail


def _batch_means_q(cur):
    """q per pixel through moments_ref itself: cur (spp, B-batched) -> Moments fed the running sums, r = g = b = the sample"""
    B, k, P = cur.shape
    m = Moments(P, 1)
    acc = np.zeros((P, 1, 3))
    for b in range(B):
        acc = acc + cur[b].sum(0)[:, None, None]
        m.add(acc, (b + 1) * k)
    assert m.B == B
    return np.maximum(quad(m.cov(), LUM), 0.0)[:, 0]                          # the Rec. 709 weights sum to 1: l(s, s, s) = s


@pytest.mark.parametrize("kind", ["gaussian", "bernoulli"])
@pytest.mark.parametrize("spp,B,n_h", [(16, 4, 16), (8, 4, 16), (32, 8, 16)])
def test_pooled_rule_is_unbiased_and_closer_than_todays(kind, spp, B, n_h):
    """per pixel: n_h history samples (their mean mu_h and their variance V_h with n_h - 1 degrees of freedom), spp current samples in B
    batches.  Both rules' mean of V / sigma^2 within [0.97, 1.03]; the pooled rule's relative RMS error below today's, no margin."""
    rng = np.random.default_rng(1000 * spp + 10 * B + (kind == "bernoulli"))
    hist, s2 = _draw(rng, kind, (n_h, N_PIXELS))
    cur, _ = _draw(rng, kind, (B, spp // B, N_PIXELS))
    mu_h, V_h = hist.mean(0), hist.var(0, ddof=1)
    l_c = cur.mean((0, 1))
    q = _batch_means_q(cur)
    today = update(V_h, mu_h, float(n_h), l_c, float(spp))
    new = pooled(V_h, mu_h, float(n_h), l_c, float(spp), q, float(B))
    (mt, et), (mp, ep) = estimator_figures(today, s2), estimator_figures(new, s2)
    print("%s spp %d in %d batches, n_h %d: today's rule mean %.3f rel RMS %.3f, pooled mean %.3f rel RMS %.3f" % (
        kind, spp, B, n_h, mt, et, mp, ep))
    assert 0.97 <= mt <= 1.03 and 0.97 <= mp <= 1.03, (mt, mp)
    assert ep < et, (ep, et)


def _synthetic_views():
    """two views of a plane, the camera moved by a third of a pixel, a history state with V and a moments state of 4 batches"""
    rng = np.random.default_rng(7)
    cam0 = synthetic_camera(W=40, H=24)
    cam1 = synthetic_camera(W=40, H=24, position=(0.034, -0.021, 10.0))
    g0, g1 = plane_gbuffer(cam0), plane_gbuffer(cam1)
    g1["hit"][3:6, 5:9] = False                                                # some misses
    H, W = g0["hit"].shape
    prev = state(g0, 0.2 + rng.random((H, W, 3)), np.full((H, W), 8.0))
    prev["V"] = 0.05 + 0.1 * rng.random((H, W))
    spp = 8
    m = Moments(H, W)
    acc = np.zeros((H, W, 3))
    for b in range(4):
        acc = acc + 2 * (0.3 + 0.4 * rng.random((H, W, 3)))
        m.add(acc, 2 * (b + 1))
    return cam0, g1, prev, acc / spp, spp, m


def test_below_min_batches_it_is_todays_rule_exactly():
    cam0, g1, prev, c, spp, m = _synthetic_views()
    spec = np.zeros(4, bool)
    want = temporal_variance(cam0, g1, prev, spec, c, spp)
    assert np.isfinite(want[g1["hit"]]).sum() > 500
    for min_batches in (5, 9):
        got = temporal_measured_variance(cam0, g1, prev, spec, c, spp, m.cov(), m.B, min_batches=min_batches)
        assert np.array_equal(got, want, equal_nan=True)
    # at min_batches the rule is the pooled one: no NaN left, q where nothing is inherited, 0 on misses
    got = temporal_measured_variance(cam0, g1, prev, spec, c, spp, m.cov(), m.B, min_batches=4)
    hit = g1["hit"]
    assert np.isfinite(got).all() and not got[~hit].any() and not np.array_equal(got[hit], want[hit])
    q = temporal_measured_variance(None, g1, None, spec, c, spp, m.cov(), m.B)
    assert np.array_equal(got[np.isnan(want)], q[np.isnan(want)]) and (q[hit] > 0).all()
    no_v = {k: v for k, v in prev.items() if k != "V"}
    assert np.array_equal(temporal_measured_variance(cam0, g1, no_v, spec, c, spp, m.cov(), m.B), q)
    assert np.isnan(temporal_measured_variance(cam0, g1, no_v, spec, c, spp, m.cov(), m.B, min_batches=5)[hit]).all()


def test_inputs_of_the_device_estimator_test_meet_its_condition():
    """tests/test_gpu_temporal_measured.py's estimator test feeds the device estimator_samples(128, 128): here the same arrays go through
    the restatement's rule with the identity for a reprojection (view 1 through the new rule, V = q, on both sides; view 2 through
    either rule), and meet what that test asserts of the device: pooled relative RMS error below the unmeasured one's, both means
    within [0.9, 1.1]."""
    s = estimator_samples(128, 128)
    views, spp, H, W = s.shape
    s2, B = 0.09, 4

    def q_of(v):
        return _batch_means_q(s[v].reshape(B, spp // B, H * W))

    V1, mu1 = q_of(0), s[0].mean(0).ravel()
    l_c, q2 = s[1].mean(0).ravel(), q_of(1)
    (mt, et) = estimator_figures(update(V1, mu1, float(spp), l_c, float(spp)), s2)
    (mp, ep) = estimator_figures(pooled(V1, mu1, float(spp), l_c, float(spp), q2, float(B)), s2)
    print("view 2 of the device test's samples: unmeasured mean %.3f rel RMS %.3f, pooled mean %.3f rel RMS %.3f" % (mt, et, mp, ep))
    assert ep < et and 0.9 <= mt <= 1.1 and 0.9 <= mp <= 1.1, (mt, et, mp, ep)


def test_bad_arguments_are_refused_before_any_device_work(product):
    lib = product.load_library()
    err = lambda: lib.ptx_last_error().decode()
    fn = lib.ptx_denoise_temporal_measured
    INVALID = 1
    for bad, what in ((dict(passes=0), "passes"), (dict(phi_normal=0.0), "phi_normal")):
        dp = product.default_denoise_params(**bad)
        assert fn(None, None, None, ctypes.byref(dp), None, None, 0, 1) == INVALID and what in err()
    tp = product.default_temporal_params(max_history=-1)
    assert fn(None, None, None, None, ctypes.byref(tp), None, 0, 1) == INVALID and "max_history" in err()
    vp = product.default_variance_params(spatial_radius=4)
    assert fn(None, None, None, None, None, ctypes.byref(vp), 0, 1) == INVALID and "spatial_radius" in err()
    assert fn(None, None, None, None, None, None, 0, 0) == INVALID and "spp" in err()
    assert fn(None, None, None, None, None, None, 1, 1) == INVALID and "min_batches" in err()
    dp = product.default_denoise_params(demodulate=0)
    assert fn(None, None, None, ctypes.byref(dp), None, None, 0, 1) == INVALID and "demodulate" in err()
    assert fn(None, None, None, None, None, None, 0, 1) == INVALID and "null" in err()
    assert lib.ptx_abi_version() == 5                                          # additive: no struct or signature moved


def test_the_new_kernel_has_no_scratch_and_the_old_ones_are_still_there():
    found = kernels_named(resource_usage("resource-usage-temporal"), ("k_temporal_reproject", "k_reproject_variance", "k_reproject_measured"))
    assert len(found) == 3, list(found)
    for k, v in found.items():
        print(k, v)
        assert v.get("scratch") == 0, (k, v)
    assert found["k_reproject_measured"]["lds"] == 0
