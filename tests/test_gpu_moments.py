"""GPU: sample moments by batch means (include/mi355x_pathtracer.h: ptx_moments_*, ptx_denoise_measured).  The add kernel and the summary
against their float64 restatement (tests/moments_ref.py); the tracer path against the host path, with nothing else moving; the filter
on the measured variance against tests/variance_ref.py; quality and calibration against a long render; the C++ veneer and the headless
driver's stop rule."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, beq
from moments_ref import LUM, Moments, from_cov6, measured_v0, quad, summary
from variance_ref import denoise_buffers_variance

pytestmark = pytest.mark.gpu

TOL = 1e-4          # tests/test_gpu_denoise.py's bound, by its metric |gpu - ref| / (|ref| + 1e-3)


def _err(gpu, ref):
    ref = np.asarray(ref, np.float64)
    e = np.abs(np.asarray(gpu, np.float64) - ref) / (np.abs(ref) + 1e-3)
    return float(e.max()) if e.size else 0.0


def _scene(pt, name, res, depth=8):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))
    return s, o


def _image(T):
    return T.read_image().reshape(T.height, T.width, 3)


def _ids(g):
    return np.stack([g["material"], g["geom"]], -1)


def _frames(h, w, ks, seed):
    """fp32 accumulation buffers as a tracer leaves them: per pixel a colour in [0.05, 1]^3, per sample a relative noise of 0.5 common
    to the channels plus 0.2 of each channel's own (so a batch of k has 1 / sqrt(k) of it), summed in fp32.  [(buffer, samples_total)]"""
    rng = np.random.default_rng(seed)
    f = np.float32
    c = (0.05 + 0.95 * rng.random((h, w, 3))).astype(f)
    acc, n, out = np.zeros((h, w, 3), f), 0, []
    for k in ks:
        z = 0.5 * rng.standard_normal((h, w, 1)) + 0.2 * rng.standard_normal((h, w, 3))
        acc = (acc + (k * c * np.maximum(1 + z / np.sqrt(k), 0)).astype(f)).astype(f)
        n += k
        out.append((acc.copy(), n))
    return out


# 1 to 6 adds with k in {1, 3, 12, 100}; the last sequence's first add finds 1000 samples in the buffer (the first add takes everything
# as one batch), so that its batches of 1, 3 and 12 are differences of sums near 1024 x the per-sample value
SEQUENCES = ([1], [3, 100], [12, 1, 3], [100, 1, 100, 3], [1, 1, 1, 1, 1], [100] * 6, [100, 1, 100, 3, 12, 1], [1000, 1, 3, 12, 1, 3])


@pytest.mark.parametrize("shape", [(61, 97), (1, 1), (700, 3), (4, 64), (5, 65)])
def test_state_matches_the_restatement(gpu_product, shape):
    """mean and covariance after every add of every sequence against the restatement fed the same fp32 buffers (so the comparison is of
    the kernel, not of the cancellation in acc - snap); batches and samples exact.  4 x 64 is exactly one workgroup, 5 x 65 one pixel
    over in both directions.  Largest cov6 error measured on an MI355X: see DESIGN.md 10."""
    pt = gpu_product
    h, w = shape
    worst_mean = worst_cov = 0.0
    with pt.Moments(0, w, h) as m:
        for si, ks in enumerate(SEQUENCES):
            m.reset()
            ref = Moments(h, w)
            for acc, n in _frames(h, w, ks, seed=1000 * h + w + si):
                m.add_host(acc, n)
                ref.add(acc, n)
                r = m.read()
                assert r["samples"] == n == ref.W and (r["batches"] == ref.B).all(), (shape, ks, n)
                em, ec = _err(r["mean"], ref.mean), _err(r["cov"], ref.cov6())
                worst_mean, worst_cov = max(worst_mean, em), max(worst_cov, ec)
                assert em <= TOL and ec <= TOL, (shape, ks, n, em, ec)
                if ref.B < 2:
                    assert not r["cov"].any()
            with pytest.raises(pt.PathTracerError, match="does not exceed"):
                m.add_host(acc, n)                                    # not increasing: refused, and nothing moved
            again = m.read()
            assert all(beq(again[k], r[k]) for k in ("mean", "cov", "batches")) and again["samples"] == n
    print("%dx%d: largest error of mean %.3g, of cov6 %.3g" % (w, h, worst_mean, worst_cov))


@pytest.mark.parametrize("shape", [(5, 40), (61, 97), (360, 640)])
def test_summary_matches_the_restatement(gpu_product, shape):
    """every field within 1e-5 relative of the restatement's summary of the state the device holds, counts exact, two runs the same
    bits.  40 pixels wide is narrower than a workgroup; 640 x 360 leaves 900 partials for stage two's 256 threads.  The threshold is put
    in the middle of the widest gap between neighbouring pixels' rel near the median, so that "rel > threshold" is the same question in
    fp32 and in float64."""
    pt = gpu_product
    h, w = shape
    with pt.Moments(0, w, h) as m:
        s0 = m.summary()
        assert (s0["pixels"], s0["samples"], s0["batches"], s0["mean_rel_se"]) == (0, 0, 0, 0.0)
        for acc, n in _frames(h, w, [12, 3, 100, 12, 1], seed=h + w):
            m.add_host(acc, n)
        r = m.read()
        C = from_cov6(r["cov"])
        for floor in (0.05, 0.4):                                    # 0.4: the floor holds on the darker pixels
            rel = np.sort(summary(r["mean"], C, r["batches"], r["samples"], floor=floor)["rel"].ravel())
            mid = rel[len(rel) // 4: 3 * len(rel) // 4 + 2]
            i = int(np.argmax(np.diff(mid))) if len(mid) > 1 else 0
            thr = float(np.float32((mid[i] + mid[i + 1]) / 2)) if len(mid) > 1 else 0.0
            want = summary(r["mean"], C, r["batches"], r["samples"], floor=floor, threshold=thr)
            got, got2 = m.summary(floor=floor, threshold=thr), m.summary(floor=floor, threshold=thr)
            assert got == got2                                       # the same bits: no atomics, fixed order
            print("%dx%d floor %g threshold %.6g:" % (w, h, floor, thr), got)
            for k in ("pixels", "pixels_over", "samples", "batches"):
                assert got[k] == want[k], (k, got[k], want[k])
            assert got["pixels"] == h * w and 0 < got["pixels_over"] < h * w
            for k in ("mean_rel_se", "rms_rel_se", "max_rel_se", "mean_variance"):
                assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (k, got[k], want[k])


def test_tracer_path_is_the_host_path_and_nothing_else_moves(gpu_product):
    """Moments.add on the tracer's buffer after batches of 2, 2, 4 and 8 iterations equals add_host fed with read_image() after each, bit
    for bit; and the tracer that serves the handle stays bit-identical (image, statistics, later iterations) to one that never saw it,
    through ptx_render and through ptx_iterate with render-ahead on and off."""
    pt = gpu_product
    W, H = 160, 90
    for mode in ("render", True, False):
        sa, _ = _scene(pt, "cornellObj.txt", (W, H))
        sb, _ = _scene(pt, "cornellObj.txt", (W, H))
        with pt.Moments(0, W, H) as md, pt.Moments(0, W, H) as mh, pt.Tracer(sa) as A, pt.Tracer(sb) as B:
            if mode != "render":
                A.set_render_ahead(mode)
                B.set_render_ahead(mode)
            n = 0
            for count in (2, 2, 4, 8):
                for T in (A, B):
                    if mode == "render":
                        T.render(n + 1, count)
                    else:
                        for it in range(n + 1, n + count + 1):
                            T.pathtrace(it)
                n += count
                md.add(A, n)
                img = A.read_image()
                mh.add_host(img, n)
                assert beq(img, B.read_image()), (mode, n)
                assert A.stats()["rays_per_bounce"] == B.stats()["rays_per_bounce"], (mode, n)
            rd, rh = md.read(), mh.read()
            assert rd["samples"] == rh["samples"] == 16 and (rd["batches"] == 4).all()
            for k in ("mean", "cov", "batches"):
                assert beq(rd[k], rh[k]), (mode, k)
            assert rd["cov"].any() and md.summary() == mh.summary()
            for T in (A, B):                                         # later iterations
                T.pathtrace(17) if mode != "render" else T.render(17, 1)
            md.add(A, 17)
            assert beq(A.read_image(), B.read_image()) and A.stats()["rays_per_bounce"] == B.stats()["rays_per_bounce"], mode


def test_denoise_measured(gpu_product):
    pt = gpu_product
    W, H = 160, 90
    s, _ = _scene(pt, "cornellObj.txt", (W, H))
    with pt.Moments(0, W, H) as m, pt.Tracer(s) as T:
        ref = Moments(H, W)
        with pytest.raises(pt.PathTracerError, match="no add"):
            T.denoise_measured(m, 1)
        T.render(1, 4)
        n = 4
        m.add(T, n)
        ref.add(T.read_image(), n)
        # (a) one batch is below every min_batches: the spatial estimate everywhere, i.e. ptx_denoise_variance
        got, gv = T.denoise_measured(m, n), T.variance()
        want, wv = T.denoise_variance(n), T.variance()
        assert beq(got, want) and beq(gv["input"], wv["input"]) and beq(gv["output"], wv["output"])
        for _ in range(7):
            T.render(n + 1, 2)
            n += 2
            m.add(T, n)
            ref.add(T.read_image(), n)
        assert ref.B == 8
        g = T.gbuffer()
        hit = g["hit"]
        c = (_image(T) / np.float32(n)).astype(np.float32)
        for demod in (1, 0):
            for min_batches in (4, 9):
                got, gv = T.denoise_measured(m, n, min_batches=min_batches, demodulate=demod), T.variance()
                v0 = measured_v0(ref.cov(), ref.W, ref.B, hit, g["albedo"], demod, min_batches)
                assert np.isnan(v0[hit]).all() if min_batches == 9 else not np.isnan(v0).any()
                # (b) the restatement of the filter on the restatement's v0 (9 > 8 batches: the spatial estimate everywhere)
                want, want_v, want_v0 = denoise_buffers_variance(c, g["albedo"], g["normal"], g["position"], hit, ids=_ids(g),
                                                                 variance=None if min_batches == 9 else v0, demodulate=demod)
                e = _err(got, want), _err(gv["input"], want_v0), _err(gv["output"], want_v)
                print("demodulate %d min_batches %d: denoised %.3g, v0 %.3g, filtered variance %.3g" % ((demod, min_batches) + e))
                assert max(e) <= TOL, (demod, min_batches, e)
                assert not gv["input"][~hit].any() and not gv["output"][~hit].any()          # (c)
                if min_batches == 9:
                    assert beq(got, T.denoise_variance(n, demodulate=demod))
        assert (~hit).any() and not beq(T.denoise_measured(m, n), T.denoise_variance(n))
        with pt.Moments(0, W, H // 2) as other:
            other.add_host(np.zeros((H // 2, W, 3), np.float32), 1)
            with pytest.raises(pt.PathTracerError, match="size"):
                T.denoise_measured(other, n)
            with pytest.raises(pt.PathTracerError, match="size"):
                other.add(T, 2)
        with pytest.raises(pt.PathTracerError, match="spp"):
            T.denoise_measured(m, 0)
        with pytest.raises(TypeError, match="max_history"):
            T.denoise_measured(m, n, max_history=4)
    with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as Tt, pt.Moments(0, W, H) as m:
        Tt.render(1, 1)
        with pytest.raises(pt.PathTracerError, match="row tile"):
            m.add(Tt, 1)


@pytest.mark.parametrize("scene", ["cornell.txt", "cornellObj.txt"])
def test_on_a_stopped_camera_the_measured_variance_beats_the_spatial_estimate(gpu_product, scene):
    """the setup of test_gpu_variance.py's test_on_a_stopped_camera_it_beats_the_fixed_colour_weight, 1024 spp in batches of 16: the
    yardstick is ptx_denoise_variance on the same frame, no margin.  The ratios to the unfiltered frame are printed."""
    pt = gpu_product
    W = H = 256
    s, _ = _scene(pt, scene, (W, H), depth=8)
    with pt.Moments(0, W, H) as m, pt.Tracer(s) as T:
        for b in range(64):
            T.render(16 * b + 1, 16)
            m.add(T, 16 * (b + 1))
        cur = (_image(T) / np.float32(1024)).astype(np.float64)
        mden = T.denoise_measured(m, 1024).astype(np.float64)
        vden = T.denoise_variance(1024).astype(np.float64)
        hit = T.gbuffer()["hit"]
        print(scene, m.summary())
        T.render(1025, 16384 - 1024)
        gt = (_image(T) / np.float32(16384)).astype(np.float64)
    mse = lambda a: float(((a - gt)[hit] ** 2).mean())
    print("%s 256x256, 1024 spp against 16384: MSE unfiltered %.4g, measured variance %.4g (x %.3f), spatial estimate %.4g (x %.3f)" % (
        scene, mse(cur), mse(mden), mse(mden) / mse(cur), mse(vden), mse(vden) / mse(cur)))
    assert mse(mden) <= mse(vden), (mse(mden), mse(vden))


def test_predicted_error_is_calibrated(gpu_product):
    """cornell.txt at 128 x 128, 64 batches of 8: over the hit pixels (all have 64 batches) without the 1 % of largest predicted variance,
    the squared error of the mean luminance against 16384 further, independent samples, summed, over the summed prediction g^T C g / W,
    lies in [0.5, 2].  The expectation is 1 + 512 / 16384 (the ground truth's own variance); a lost or doubled factor of k or spp moves
    it by 8 x or more.  Measured on an MI355X: see DESIGN.md 10."""
    pt = gpu_product
    W = H = 128
    s, _ = _scene(pt, "cornell.txt", (W, H), depth=8)
    with pt.Moments(0, W, H) as m, pt.Tracer(s) as T:
        for b in range(64):
            T.render(8 * b + 1, 8)
            m.add(T, 8 * (b + 1))
        r = m.read()
        hit = T.gbuffer()["hit"]
        at512 = _image(T).astype(np.float64)
        T.render(513, 16384)
        gt = (_image(T).astype(np.float64) - at512) / 16384
    assert r["samples"] == 512 and (r["batches"] == 64).all()
    pred = quad(from_cov6(r["cov"]), LUM) / r["samples"]
    use = hit & (r["batches"] >= 2)
    cut = np.sort(pred[use])[int(np.ceil(0.99 * use.sum())) - 1]
    keep = use & (pred <= cut)
    assert keep.sum() >= 0.99 * use.sum() - 1
    err2 = ((r["mean"].astype(np.float64) - gt) @ LUM) ** 2
    ratio = err2[keep].sum() / pred[keep].sum()
    print("calibration: %d of %d hit pixels, sum err^2 %.6g, sum predicted %.6g, ratio %.4f (all hit pixels: %.4f)" % (
        keep.sum(), use.sum(), err2[keep].sum(), pred[keep].sum(), ratio, err2[use].sum() / pred[use].sum()))
    assert 0.5 <= ratio <= 2.0, ratio


def test_cpp_veneer_loop_matches_the_python_sequence(gpu_product, tmp_path):
    pt = gpu_product
    exe = tmp_path / "moments_veneer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "moments_veneer_check.cpp"),
                           "-L" + os.path.join(ROOT, "mygpuraytracer_amd"), "-lmi355x_pathtracer", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mygpuraytracer_amd") + ",-rpath,/opt/rocm/lib"])
    W, H, D, N, K, F, DX = 96, 64, 6, 8, 2, 2, 5.0
    scene = os.path.join(ROOT, "scenes", "cornellObj.txt")
    out = subprocess.check_output([str(exe), scene, str(W), str(H), str(D), str(N), str(K), str(F), "%g" % DX, str(tmp_path / "v")],
                                  text=True, timeout=300)
    assert "moments veneer ok" in out
    rd = lambda f, ext, dt: np.frombuffer(open("%s.f%d%s" % (tmp_path / "v", f, ext), "rb").read(), dt)
    s, o = _scene(pt, "cornellObj.txt", (W, H), depth=D)
    with pt.Moments(0, W, H) as m:
        for f in range(1, F + 1):
            if f > 1:
                s.orbit_events(o, [("left", DX, 0.0)])
            m.reset()                                                # pathtraceInit's
            with pt.Tracer(s) as T:
                for it in range(1, N + 1):
                    T.pathtrace(it)
                    if it % K == 0:
                        m.add(T, it)
                frame = T.denoise_measured(m, N)
                r = m.read()
                assert beq(rd(f, ".output", np.float32).reshape(H, W, 3), frame), f
                assert beq(rd(f, ".mean", np.float32).reshape(H, W, 3), r["mean"]) and beq(rd(f, ".cov", np.float32).reshape(H, W, 6), r["cov"]), f
                assert (r["batches"] == N // K).all() and not beq(frame, T.denoise_variance(N))


def test_headless_until_error(gpu_product, tmp_path):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    common = [exe, scene, "--res", "64", "64", "--pfm"]
    r = subprocess.run(common + ["--iterations", "512", "--until-error", "0.3", "--out", str(tmp_path / "u")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    checks = re.findall(r"^check: (\d+) iterations, (\d+) batches, mean rel se (\S+),", r.stdout, re.M)
    final = re.search(r"^until-error: (\d+) iterations, mean rel se (\S+) <= 0.3$", r.stdout, re.M)
    assert final, r.stdout
    n = int(final.group(1))
    assert n < 512 and n % 16 == 0 and n >= 32
    assert [int(c[0]) for c in checks] == list(range(16, n + 1, 16)) and [int(c[1]) for c in checks] == list(range(1, n // 16 + 1))
    assert float(checks[-1][2]) <= 0.3 and all(float(c[2]) > 0.3 or int(c[1]) < 2 for c in checks[:-1])
    p = subprocess.run(common + ["--iterations", str(n), "--out", str(tmp_path / "p")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "check:" not in p.stdout, p.stderr
    for ext in ("png", "pfm"):
        (fu,), (fp,) = glob.glob(str(tmp_path / ("u.*.%dsamp.%s" % (n, ext)))), glob.glob(str(tmp_path / ("p.*.%dsamp.%s" % (n, ext))))
        assert open(fu, "rb").read() == open(fp, "rb").read(), ext
    # --measured: the variance the run collected (here a batch every 16 iterations), and what it needs
    d = subprocess.run(common + ["--iterations", "64", "--denoise", "--measured", "--out", str(tmp_path / "m")], capture_output=True,
                       text=True, timeout=300)
    v = subprocess.run(common + ["--iterations", "64", "--denoise", "--variance", "--out", str(tmp_path / "s")], capture_output=True,
                       text=True, timeout=300)
    assert d.returncode == 0 and v.returncode == 0, d.stderr + v.stderr
    rb = lambda pat: open(glob.glob(str(tmp_path / pat))[0], "rb").read()
    assert rb("m.*.64samp.pfm") == rb("s.*.64samp.pfm") and rb("m.*.64samp.denoised.pfm") != rb("s.*.64samp.denoised.pfm")
    bad = subprocess.run([exe, scene, "--measured"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--denoise" in bad.stderr
