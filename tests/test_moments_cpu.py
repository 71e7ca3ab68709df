"""CPU: the batch-means moments' definition (tests/moments_ref.py on synthetic iid samples), their C-ABI surface without a device, and what
the compiler made of their kernels.  The device is held to the same restatement by tests/test_gpu_moments.py."""
import ctypes

import numpy as np
import pytest

from moments_ref import LUM, Moments, quad, summary
from resource_usage import kernels_named, resource_usage

SIZES = (1, 2, 5, 12, 40)


def test_batch_means_are_unbiased_whatever_the_batch_sizes():
    """iid samples of three correlated channels in batches of unequal sizes: the mean of C is the samples' covariance and the mean of
    g^T C g / W the squared error of the frame's mean luminance, both within 2 %.  4096 pixels per state; the squared error of ONE such
    frame is a mean of 4096 chi-square(1) terms, known to sqrt(2 / 4096) = 2.2 % only, so 64 independent sequences (each with its own
    batch sizes) are pooled: 0.28 % for the squared error, and below 0.2 % for every entry of C (>= 11 batches each)."""
    rng = np.random.default_rng(20240607)
    P, runs = 4096, 64
    mu = np.array([0.8, 0.5, 0.3])
    L = np.array([[0.5, 0.0, 0.0], [0.3, 0.4, 0.0], [0.2, 0.1, 0.3]])
    cov = L @ L.T
    Csum, pred, err2, used = np.zeros((3, 3)), 0.0, 0.0, set()
    for _ in range(runs):
        ks = rng.choice(SIZES, 12)
        used.update(int(k) for k in ks)
        m = Moments(1, P)
        acc, n = np.zeros((1, P, 3)), 0
        for k in ks:
            acc = acc + (mu + rng.standard_normal((P, int(k), 3)) @ L.T).sum(1)
            n += int(k)
            m.add(acc, n)
        assert (m.W, m.B) == (n, len(ks)) and np.allclose(m.mean, acc / n, rtol=1e-12)
        C = m.cov()
        Csum += C.mean((0, 1))
        pred += (quad(C, LUM) / m.W).mean()
        err2 += (((m.mean - mu) @ LUM) ** 2).mean()
    Cbar = Csum / runs
    print("mean C / truth:\n%s\nmean g^T C g / W %.6g, squared error of the mean %.6g (ratio %.4f)" % (Cbar / cov, pred / runs, err2 / runs, pred / err2))
    assert used == set(SIZES)
    assert (np.abs(Cbar - cov) <= 0.02 * np.abs(cov)).all()
    assert abs(pred - err2) <= 0.02 * err2


def test_first_add_takes_the_buffer_as_one_batch_and_the_summary_by_hand():
    m = Moments(1, 2)
    a1 = np.array([[[4.0, 2.0, 0.0], [1.0, 1.0, 1.0]]])
    m.add(a1, 4)
    assert m.B == 1 and np.array_equal(m.mean, a1 / 4) and not m.M.any() and not m.cov().any()
    s = summary(m.mean, m.cov(), m.B, m.W)
    assert s["pixels"] == 0 and s["mean_rel_se"] == 0.0 and (s["samples"], s["batches"]) == (4, 1)
    # a second batch of 4 whose mean is 2 a1 / 4: two equally weighted points, C = k (x1 - x2)(x1 - x2)^T / 2
    m.add(3 * a1, 8)
    d = a1 / 4
    want = 4 * d[..., :, None] * d[..., None, :] / 2
    assert np.allclose(m.cov(), want, rtol=1e-14) and np.allclose(m.mean, 1.5 * a1 / 4)
    s = summary(m.mean, m.cov(), m.B, m.W, floor=0.05, threshold=0.3)
    rel = np.sqrt(quad(want, LUM) / 8) / np.maximum((1.5 * a1 / 4) @ LUM, 0.05)
    assert s["pixels"] == 2 and np.isclose(s["max_rel_se"], rel.max()) and np.isclose(s["mean_rel_se"], rel.mean())
    assert s["pixels_over"] == int((rel > 0.3).sum()) and np.isclose(s["mean_variance"], quad(want, LUM).mean())


def test_moments_structs_and_defaults(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    assert lib.ptx_sizeof_moments_params() == ctypes.sizeof(api.MomentsParams) == 8
    assert lib.ptx_sizeof_moments_summary() == ctypes.sizeof(api.MomentsSummary) == 64
    p = product.default_moments_params()
    assert (p.floor, p.threshold) == (float(np.float32(0.05)), float(np.float32(0.05)))     # stated in the header, not tuned
    assert product.default_moments_params(floor=0.5).floor == 0.5
    with pytest.raises(AttributeError):
        product.default_moments_params(bogus=1)
    assert lib.ptx_abi_version() == 5                    # no existing struct or entry point changed


def test_bad_moments_arguments_are_refused_before_any_device_work(product):
    lib = product.load_library()
    err = lambda: lib.ptx_last_error().decode()
    INVALID = 1
    out = ctypes.c_void_p()
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 16)):
        assert lib.ptx_moments_create(0, w, h, ctypes.byref(out)) == INVALID and "frame size" in err(), (w, h)
    assert lib.ptx_moments_create(0, 4, 4, None) == INVALID and "NULL" in err()
    assert lib.ptx_moments_create(-1, 4, 4, ctypes.byref(out)) == INVALID and "device" in err()
    assert not out.value
    if lib.ptx_device_count() < 1:                       # and with good arguments there is no CPU path
        assert lib.ptx_moments_create(0, 4, 4, ctypes.byref(out)) == 4 and "no HIP device" in err()
    assert lib.ptx_moments_reset(None) == INVALID and "null" in err()
    lib.ptx_moments_destroy(None)                        # a no-op
    z = np.zeros(3, np.float32)
    ptr = z.ctypes.data_as(ctypes.c_void_p)
    for total in (0, -3):                                # never increasing: the handle's count starts at 0
        assert lib.ptx_moments_add(None, None, total) == INVALID and "samples_total" in err()
        assert lib.ptx_moments_add_host(None, ptr, total) == INVALID and "samples_total" in err()
    assert lib.ptx_moments_add(None, None, 1) == INVALID and "null" in err()
    assert lib.ptx_moments_add_host(None, ptr, 1) == INVALID and "null" in err()
    assert lib.ptx_moments_read(None, None, None, None, None) == INVALID and "null" in err()
    s = product.MomentsSummary()
    for bad, what in ((dict(floor=0.0), "floor"), (dict(floor=float("nan")), "floor"), (dict(floor=float("inf")), "floor"),
                      (dict(threshold=-1.0), "threshold"), (dict(threshold=float("nan")), "threshold")):
        p = product.default_moments_params(**bad)
        assert lib.ptx_moments_summarize(None, ctypes.byref(p), ctypes.byref(s)) == INVALID and what in err(), bad
    assert lib.ptx_moments_summarize(None, None, ctypes.byref(s)) == INVALID and "null" in err()
    # ptx_denoise_measured: parameters, spp and min_batches before the handles
    bad_dp = product.default_denoise_params(passes=0)
    assert lib.ptx_denoise_measured(None, None, ctypes.byref(bad_dp), None, 0, 1) == INVALID and "passes" in err()
    bad_vp = product.default_variance_params(phi_luminance=0.0)
    assert lib.ptx_denoise_measured(None, None, None, ctypes.byref(bad_vp), 0, 1) == INVALID and "phi_luminance" in err()
    assert lib.ptx_denoise_measured(None, None, None, None, 0, 0) == INVALID and "spp" in err()
    assert lib.ptx_denoise_measured(None, None, None, None, 1, 1) == INVALID and "min_batches" in err()
    assert lib.ptx_denoise_measured(None, None, None, None, 0, 1) == INVALID and "null" in err()


def test_moments_kernels_do_not_spill():
    found = kernels_named(resource_usage("resource-usage-moments"), ("k_moments_add", "k_moments_summary", "k_moments_total", "k_moments_prep"))
    assert len(found) == 4, list(found)                  # the add, the summary's two stages, the filter's prep
    for k, v in found.items():
        assert v.get("scratch") == 0, (k, v)
        print(k, v)
    assert found["k_moments_add"]["lds"] == 0 and found["k_moments_prep"]["lds"] == 0
