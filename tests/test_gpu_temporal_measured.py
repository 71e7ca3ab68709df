"""GPU: the temporal denoiser on the measured sample variance (include/mi355x_pathtracer.h: ptx_denoise_temporal_measured).  The tracer
path (V, v0, mix, denoised frame) against its float64 restatement (tests/temporal_measured_ref.py) over an orbit; the fall-back below
min_batches, bit for bit; without history it is ptx_denoise_measured; the pooled rule as an estimator on samples of known variance;
nothing else moves; determinism; refusals; the C++ veneer and the headless driver; the quality on the orbit, printed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, beq
from moments_ref import Moments
from temporal_measured_ref import estimator_figures, estimator_samples, temporal_measured_variance
from temporal_ref import camera_dict, mix, reproject, specular_flags, state
from variance_ref import atrous_variance, demodulated

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


def _step(s, o, T, dx, dy=0.0, moments=()):
    """a camera step restarts the accumulation: the moments start again with it"""
    s.orbit_events(o, [("left", dx, dy)])
    T.set_camera(s)
    T.reset_image()
    for m in moments:
        m.reset()


def _image(T):
    return T.read_image().reshape(T.height, T.width, 3)


def _batches(T, m, done, count, size, ref=None):
    """`count` batches of `size` iterations after the `done` the buffer holds, a Moments.add after each; -> the iterations it holds now"""
    for _ in range(count):
        T.render(done + 1, size)
        done += size
        m.add(T, done)
        if ref is not None:
            ref.add(T.read_image(), done)
    return done


def _state_after(T, tm, spp):
    """the history a call with V left in `tm`, as the restatement takes it"""
    r, g, var = tm.read(), T.gbuffer(), T.variance()
    n_dev = np.where(g["hit"] & (r["count"] > 0), spp + r["count"].astype(np.float64), float(spp))
    st = state(g, r["mix"], n_dev)
    st["V"] = var["input"].astype(np.float64) * n_dev
    return st


_ORBIT = {}


def _orbit(pt, res):
    """The orbit of the two tests below, run once per size: cornellObj.txt, 8 spp per view in 4 batches of 2, each followed by
    Moments.add, Moments.reset after every camera step.  Every view goes through ptx_denoise_temporal_measured and is compared with the
    restatement; mix and count are asserted here, as tests/test_gpu_variance.py bounds them, and so is the share of `near` pixels.
    -> one dict per view: label, pooled (pixels that pool V), e_in / e_out / e_v (v0, denoised frame, filtered variance by _err), over
    (pixels whose v0 is over TOL)."""
    if res in _ORBIT:
        return _ORBIT[res]
    W, H = res
    s, o = _scene(pt, "cornellObj.txt", (W, H))
    spec = specular_flags(s.dump()["materials"])
    dp, vp = pt.default_denoise_params(), pt.default_variance_params()
    geo = dict(phi_normal=dp.phi_normal, phi_position=dp.phi_position)
    ref = Moments(H, W)
    rows = []

    def check(T, tm, m, n_spp, prev, prev_cam, label):
        """one ptx_denoise_temporal_measured against the restatement; prev: the committed history (with "V", without, or None)"""
        frame = T.denoise_measured(m, n_spp, temporal=tm)
        r, g, var = tm.read(), T.gbuffer(), T.variance()
        hit = g["hit"]
        c = (_image(T) / np.float32(n_spp)).astype(np.float32)
        near = np.zeros((H, W), bool)
        if prev is None:
            assert not r["count"].any() and beq(r["mix"], c), label
            n = np.full((H, W), float(n_spp))
        else:
            h, nh, near = reproject(prev_cam, g, prev, spec)
            m_ref, n, _ = mix(_image(T), n_spp, hit, h, nh)
            assert near.sum() < 0.001 * W * H
            assert np.isclose(r["mix"][~near].astype(np.float64), m_ref[~near], rtol=1e-4, atol=1e-3).all(), label
            assert np.isclose(r["count"][~near], nh[~near], rtol=1e-4, atol=1e-3).all(), label
        assert ref.B == m.read()["batches"].max() >= 4 and ref.W == n_spp
        V = temporal_measured_variance(prev_cam, g, prev, spec, c, n_spp, ref.cov(), ref.B)
        assert np.isfinite(V).all()                                    # nothing is left to the spatial estimate
        v0 = V / n
        has_v = prev is not None and "V" in prev
        pooled = hit & (r["count"] > 0) if has_v else np.zeros((H, W), bool)
        if has_v:
            assert pooled.sum() > W * H // 4, label
        keep = ~near
        each = np.abs(var["input"].astype(np.float64) - v0) / (np.abs(v0) + 1e-3)
        e_in = _err(var["input"][keep], v0[keep])
        col, f = demodulated(r["mix"], g["albedo"], hit)
        # the filter on what the device fed it: its own mix and v0
        want, want_v = atrous_variance(col, var["input"], g["normal"], g["position"], hit, dp.passes, vp.phi_luminance, vp.epsilon,
                                       vp.prefilter, **geo)
        e_out, e_v = _err(frame, want * f), _err(var["output"], want_v)
        rows.append(dict(label=label, pooled=int(pooled.sum()), e_in=e_in, e_out=e_out, e_v=e_v, over=int((each[keep] > TOL).sum())))
        print("%dx%d %s: %d pixels pool V, %d take q; v0 %.3g (%d pixels over), denoised %.3g, filtered variance %.3g" % (
            W, H, label, pooled.sum(), (hit & ~pooled).sum(), e_in, rows[-1]["over"], e_out, e_v))
        assert not var["input"][~hit].any() and not var["output"][~hit].any()
        return _state_after(T, tm, n_spp)

    with pt.Temporal(0, W, H) as tm, pt.Moments(0, W, H) as m, pt.Tracer(s) as T:
        def view(n0=0, step=True):
            if step:
                _step(s, o, T, 8.0, 1.0, [m, ref])
            return _batches(T, m, n0, 4, 2, ref)

        n = view(step=False)
        st0, cam0 = check(T, tm, m, n, None, None, "frame 1 (no history)"), camera_dict(s.camera)
        n = view()
        check(T, tm, m, n, st0, cam0, "frame 2 (history with V)")
        n = view(n, step=False)                                        # the same segment, recomputed from the same history with 16 spp
        assert n == 16 and ref.B == 8
        check(T, tm, m, n, st0, cam0, "frame 2 again, 16 spp in 8 batches")
        n = view()
        T.denoise_temporal(tm, n)                                      # the old call: the state it leaves carries no V
        r, g = tm.read(), T.gbuffer()
        st2 = state(g, r["mix"], np.where(g["hit"] & (r["count"] > 0), n + r["count"].astype(np.float64), float(n)))
        cam2 = camera_dict(s.camera)
        n = view()
        check(T, tm, m, n, st2, cam2, "frame 4 (history without V: q, not the spatial estimate)")
        assert (tm.read()["count"] > 0).any()
        n = view()
        T.denoise_variance(n, tm)                                      # the old call with V: the two share one handle
        st4, cam4 = _state_after(T, tm, n), camera_dict(s.camera)
        n = view()
        check(T, tm, m, n, st4, cam4, "frame 6 (history from ptx_denoise_variance)")
    _ORBIT[res] = rows
    return rows


SIZES = [(160, 90), (97, 61)]       # 97 x 61: the last pixel of a row shares its mb record with padding, a wave edge falls at x = 64


@pytest.mark.parametrize("res", SIZES)
def test_tracer_path_matches_the_restatement_over_an_orbit(gpu_product, res):
    """mix and count (in _orbit), the denoised frame and the filtered variance of every view within TOL, and v0 within TOL on the views
    where no pixel pools a V (no history, a history without V): there V = q on every hit pixel."""
    rows = _orbit(gpu_product, res)
    assert len(rows) == 5 and [r["pooled"] > 0 for r in rows] == [False, True, True, False, True]
    for r in rows:
        assert r["e_out"] <= TOL and r["e_v"] <= TOL, r
        if not r["pooled"]:
            assert r["e_in"] <= TOL, r


@pytest.mark.parametrize("res", SIZES)
def test_v0_of_the_views_that_pool_matches_the_restatement(gpu_product, res):
    """v0 within TOL on the three views whose pixels pool a V, the pixels `reproject` flags as near excluded.
    This is the check that holds the kernel to double-precision weights for V_h and mu_h.  With the fp32 weights of the other two
    kernels it read 0.00055 at 160 x 90 (40 of 14400 pixels over TOL) and 0.00067 at 97 x 61, and so did ptx_denoise_variance with the
    handle on the same frames against variance_ref.temporal_variance: every such pixel is black in the current view (c = 0, q = 0, so
    its V is all history) with one bilinear tap of weight 5e-4 .. 5e-3 on a pixel whose V is about 3 (one of its 8 samples found the
    light) and the other taps on V = 0; at u near 100 an fp32 ulp is 8e-6 of a pixel, 2 % of such a weight.  Measured on an MI355X
    now: 1.8e-6 at the most."""
    rows = _orbit(gpu_product, res)
    for r in rows:
        if r["pooled"]:
            assert r["e_in"] <= TOL, r


def test_below_min_batches_it_is_denoise_variance_bit_for_bit(gpu_product):
    pt = gpu_product
    W, H = 97, 61
    s, o = _scene(pt, "cornellObj.txt", (W, H))
    with pt.Temporal(0, W, H) as ta, pt.Temporal(0, W, H) as tb, pt.Moments(0, W, H) as m, pt.Tracer(s) as T:
        for k in range(3):
            if k:
                _step(s, o, T, 6.0, 1.0, [m])
            n = _batches(T, m, 0, 2, 2)                                # two adds
            got, gv, gr = T.denoise_measured(m, n, min_batches=4, temporal=ta), T.variance(), ta.read()
            want, wv, wr = T.denoise_variance(n, tb), T.variance(), tb.read()
            assert beq(got, want) and beq(gv["input"], wv["input"]) and beq(gv["output"], wv["output"]), k
            for key in gr:
                assert beq(gr[key], wr[key]), (k, key)
            if k == 2:                                                 # and with two batches allowed it is another frame
                assert not beq(T.denoise_measured(m, n, min_batches=2, temporal=ta), want)
        assert (gr["count"] > 0).any()


def test_without_history_it_is_denoise_measured(gpu_product):
    pt = gpu_product
    W, H, spp = 97, 61, 8
    s, o = _scene(pt, "cornellObj.txt", (W, H))
    with pt.Temporal(0, W, H) as tm, pt.Moments(0, W, H) as m, pt.Tracer(s) as T:
        for k, extra in enumerate((dict(), dict(max_history=0))):      # a fresh handle, then a history that max_history = 0 ignores
            if k:
                _step(s, o, T, 6.0, 1.0, [m])
            assert _batches(T, m, 0, 4, 2) == spp                      # the moments' W == spp, B = 4
            got, gv = T.denoise_measured(m, spp, temporal=tm, **extra), T.variance()
            assert not tm.read()["count"].any()
            want, wv = T.denoise_measured(m, spp), T.variance()
            e = _err(got, want), _err(gv["input"], wv["input"]), _err(gv["output"], wv["output"])
            print("%s: denoised %.3g, v0 %.3g, filtered variance %.3g; bit-equal: %s" % (
                "max_history 0" if k else "fresh handle", e[0], e[1], e[2],
                beq(got, want) and beq(gv["input"], wv["input"]) and beq(gv["output"], wv["output"])))
            assert max(e) <= TOL, (k, e)
            assert gv["input"][T.gbuffer()["hit"]].any()


def test_the_pooled_rule_estimates_a_known_variance_better(gpu_product):
    """Samples of known variance through Tracer.write_image: sample j of a hit pixel is max(albedo, 1e-3) * s_j with s_j iid, mean 1,
    variance 0.09 (temporal_measured_ref.estimator_samples), so the demodulated luminance has exactly that variance.  Per view the
    cumulative sum after 4, 8, 12 and 16 samples is written, each followed by a Moments.add.  View 1 goes through the new call on two
    handles alike; view 2 through the new call on one and through ptx_denoise_variance on the other.  Over the hit pixels with
    count > 0, V = v0 (spp + count): the pooled relative RMS error is below the unmeasured one's, and both means of V / sigma^2 lie
    within [0.9, 1.1].  tests/test_temporal_measured_cpu.py runs the same arrays through the restatement's rule first.
    The orbit step is 0.02 window pixels: the camera differs, so the call starts a new segment, while every pixel reprojects to within
    a few hundredths of a pixel of itself.  That is on purpose.  A bilinear tap over four INDEPENDENT pixels averages their means, so
    Var(mu_h) = sigma^2 sum w^2 / n_h and E[e] = sigma^2 (1 + sum w^2) / 2 at n_h = spp: at a generic sub-pixel offset (mean sum w^2 =
    4 / 9) today's rule would read 0.86 sigma^2 through no fault of either estimator, only because this test's neighbouring pixels are
    independent where a renderer's history is a smooth signal.  With sum w^2 >= 0.9 that bias is below 3 %."""
    pt = gpu_product
    W = H = 128
    spp, s2 = 16, 0.09
    samples = estimator_samples(H, W, spp=spp, views=2, sigma2=s2)
    s, o = _scene(pt, "cornell.txt", (W, H))
    with pt.Temporal(0, W, H) as ta, pt.Temporal(0, W, H) as tb, pt.Moments(0, W, H) as m, pt.Tracer(s) as T:
        def feed(view):
            g = T.gbuffer()
            a = np.where(g["hit"][..., None], np.maximum(g["albedo"].astype(np.float64), 1e-3), 1.0)
            m.reset()
            for done in (4, 8, 12, 16):
                T.write_image((a * samples[view, :done].sum(0)[..., None]).astype(np.float32))
                m.add(T, done)
            return g["hit"]

        feed(0)
        T.denoise_measured(m, spp, temporal=ta)
        first = T.variance()["input"]
        T.denoise_measured(m, spp, temporal=tb)
        assert beq(first, T.variance()["input"])
        s.orbit_events(o, [("left", 0.02, 0.0)])
        T.set_camera(s)
        T.reset_image()
        hit = feed(1)
        out = {}
        for label, tm in (("pooled", ta), ("unmeasured", tb)):
            if label == "pooled":
                T.denoise_measured(m, spp, temporal=tm)
            else:
                T.denoise_variance(spp, tm)
            out[label + " read"] = tm.read()
            count, v0 = tm.read()["count"].astype(np.float64), T.variance()["input"].astype(np.float64)
            use = hit & (count > 0)
            assert use.sum() > hit.sum() // 2 and count[use].min() > 15.0
            out[label] = estimator_figures((v0 * (spp + count))[use], s2)
            print("%s: %d pixels, mean V / sigma^2 %.4f, relative RMS error %.4f" % ((label, use.sum()) + out[label]))
    for key, got in out.pop("pooled read").items():                    # only V differs: history, count and mix are the old call's bits
        assert beq(got, out["unmeasured read"][key]), key
    del out["unmeasured read"]
    assert out["pooled"][1] < out["unmeasured"][1], out
    assert 0.9 <= out["pooled"][0] <= 1.1 and 0.9 <= out["unmeasured"][0] <= 1.1, out


def test_nothing_else_moves(gpu_product):
    """the accumulation buffer, the statistics, later iterations and the moments state of a tracer that serves the new call are those
    of one that never saw it, render-ahead on and off"""
    pt = gpu_product
    W, H = 160, 90
    for ahead in (True, False):
        sa, oa = _scene(pt, "cornellObj.txt", (W, H))
        sb, ob = _scene(pt, "cornellObj.txt", (W, H))
        with pt.Temporal(0, W, H) as ta, pt.Moments(0, W, H) as ma, pt.Moments(0, W, H) as mb, pt.Tracer(sa) as A, pt.Tracer(sb) as B:
            A.set_render_ahead(ahead)
            B.set_render_ahead(ahead)
            for k in range(3):
                if k:
                    _step(sa, oa, A, 6.0, 1.0, [ma])
                    _step(sb, ob, B, 6.0, 1.0, [mb])
                for it in range(1, 9):
                    A.pathtrace(it)
                    B.pathtrace(it)
                    if it % 2 == 0:
                        ma.add(A, it)
                        mb.add(B, it)
                    if it in (4, 8):                                   # (at 4: two batches, the fall-back; at 8: four, the new kernel)
                        A.denoise_measured(ma, it, temporal=ta, read=(k == 1))
                assert beq(A.read_image(), B.read_image()), (ahead, k)
                assert A.stats()["rays_per_bounce"] == B.stats()["rays_per_bounce"], (ahead, k)
                ra, rb = ma.read(), mb.read()
                assert ra["samples"] == rb["samples"] == 8 and all(beq(ra[key], rb[key]) for key in ("mean", "cov", "batches")), (ahead, k)
            assert (ta.read()["count"] > 0).any()


def test_deterministic(gpu_product):
    pt = gpu_product
    W, H = 97, 61
    runs = []
    for _ in range(2):
        s, o = _scene(pt, "cornell.txt", (W, H))
        out = []
        with pt.Temporal(0, W, H) as tm, pt.Moments(0, W, H) as m, pt.Tracer(s) as T:
            for k in range(3):
                if k:
                    _step(s, o, T, 7.0, -2.0, [m])
                n = _batches(T, m, 0, 4, 2)
                out.append(T.denoise_measured(m, n, temporal=tm))
                out.extend(T.variance().values())
                out.extend(tm.read().values())
        runs.append(out)
    for a, b in zip(*runs):
        assert beq(a, b)


def test_refusals_raise_with_a_message_and_leave_everything_as_it_was(gpu_product):
    pt = gpu_product
    W = H = 64
    s, o = _scene(pt, "cornell.txt", (W, H))
    lib = pt.load_library()
    with pt.Tracer(s) as T, pt.Temporal(0, W, H) as tm, pt.Moments(0, W, H) as m:
        _batches(T, m, 0, 4, 1)
        T.denoise_measured(m, 4, temporal=tm)
        _step(s, o, T, 5.0, 0.0, [m])
        _batches(T, m, 0, 4, 1)
        frame = T.denoise_measured(m, 4, temporal=tm)
        var, hist = T.variance(), tm.read()
        assert (hist["count"] > 0).any()
        _step(s, o, T, 5.0, 0.0, [m])                                  # a call that got through would start a new segment
        _batches(T, m, 0, 4, 1)
        mom = m.read()
        with pytest.raises(pt.PathTracerError, match="spp"):
            T.denoise_measured(m, 0, temporal=tm)
        for bad, what in ((dict(phi_luminance=-1.0), "phi_luminance"), (dict(epsilon=0.0), "epsilon"), (dict(spatial_radius=4), "spatial_radius"),
                          (dict(max_history=-1), "max_history"), (dict(normal_cos=2.0), "normal_cos"), (dict(passes=0), "passes")):
            with pytest.raises(pt.PathTracerError, match=what):
                T.denoise_measured(m, 4, temporal=tm, **bad)
        with pytest.raises(pt.PathTracerError, match="demodulate"):
            T.denoise_measured(m, 4, temporal=tm, demodulate=0)
        with pytest.raises(pt.PathTracerError, match="min_batches"):
            T.denoise_measured(m, 4, min_batches=1, temporal=tm)
        for args in ((None, tm.h, m.h), (T.h, None, m.h), (T.h, tm.h, None)):
            assert lib.ptx_denoise_temporal_measured(*args, None, None, None, 0, 4) == 1
            assert "null" in lib.ptx_last_error().decode()
        with pt.Moments(0, W, H) as fresh:
            with pytest.raises(pt.PathTracerError, match="no add"):
                T.denoise_measured(fresh, 4, temporal=tm)
        with pt.Moments(0, W, H // 2) as other:
            other.add_host(np.zeros((H // 2, W, 3), np.float32), 1)
            with pytest.raises(pt.PathTracerError, match="moments handle's size"):
                T.denoise_measured(other, 4, temporal=tm)
        with pt.Temporal(0, W, H // 2) as other:
            with pytest.raises(pt.PathTracerError, match="temporal handle's size"):
                T.denoise_measured(m, 4, temporal=other)
        with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as Tt:
            Tt.render(1, 1)
            with pytest.raises(pt.PathTracerError, match="row tile"):
                Tt.denoise_measured(m, 4, temporal=tm)
        after_v, after_h, after_m = T.variance(), tm.read(), m.read()
        assert beq(T.read_denoised(), frame) and all(beq(var[k], after_v[k]) for k in var)
        assert all(beq(hist[k], after_h[k]) for k in hist)
        assert after_m["samples"] == mom["samples"] and all(beq(mom[k], after_m[k]) for k in ("mean", "cov", "batches"))


def test_cpp_veneer_loop_matches_the_python_sequence(gpu_product, tmp_path):
    pt = gpu_product
    exe = tmp_path / "temporal_measured_veneer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "temporal_measured_veneer_check.cpp"),
                           "-L" + os.path.join(ROOT, "mygpuraytracer_amd"), "-lmi355x_pathtracer", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mygpuraytracer_amd") + ",-rpath,/opt/rocm/lib"])
    W, H, D, N, K, F, DX = 96, 64, 6, 8, 2, 4, 5.0
    scene = os.path.join(ROOT, "scenes", "cornellObj.txt")
    out = subprocess.check_output([str(exe), scene, str(W), str(H), str(D), str(N), str(K), str(F), "%g" % DX, str(tmp_path / "v")],
                                  text=True, timeout=300)
    assert "temporal measured veneer ok" in out
    rd = lambda f: np.frombuffer(open("%s.f%d.output" % (tmp_path / "v", f), "rb").read(), np.float32).reshape(H, W, 3)
    s, o = _scene(pt, "cornellObj.txt", (W, H), depth=D)
    with pt.Temporal(0, W, H) as tm, pt.Moments(0, W, H) as m, pt.Temporal(0, W, H) as tv:
        for f in range(1, F + 1):
            if f > 1:
                s.orbit_events(o, [("left", DX, 0.0)])
            m.reset()                                                  # pathtraceInit's
            with pt.Tracer(s) as T:
                for it in range(1, N + 1):
                    T.pathtrace(it)
                    if it % K == 0:
                        m.add(T, it)
                frame = T.denoise_measured(m, N, temporal=tm)
                e = _err(rd(f), frame)
                print("frame %d: veneer against Python %.3g, bit-equal: %s" % (f, e, beq(rd(f), frame)))
                assert e <= TOL, (f, e)
                assert not beq(frame, T.denoise_variance(N, tv))
        assert (tm.read()["count"] > 0).any()


def test_headless_frames_with_measured(gpu_product, tmp_path):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    scene = os.path.join(ROOT, "scenes", "cornellObj.txt")
    F = 3
    common = [exe, scene, "--res", "64", "64", "--iterations", "8", "--frames", str(F), "--frame-step", "left:4,1", "--denoise", "--pfm"]
    runs = {}
    for prefix, extra in (("tm2", ["--temporal", "--measured", "--measure-every", "2"]), ("tm8", ["--temporal", "--measured", "--measure-every", "8"]),
                          ("tvm", ["--temporal", "--variance", "--measured", "--measure-every", "2"]), ("t", ["--temporal"]),
                          ("tv", ["--temporal", "--variance"])):
        r = subprocess.run(common + extra + ["--out", str(tmp_path / prefix)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (prefix, r.stderr)
        runs[prefix] = r.stdout
    rb = lambda n: open(tmp_path / n, "rb").read()
    assert "fell back" not in runs["tm2"] and runs["tm8"].count("fell back to the unmeasured variance estimate") == F
    for f in range(1, F + 1):
        for ext in ("png", "pfm"):
            assert rb("tm2.f%03d.%s" % (f, ext)) == rb("t.f%03d.%s" % (f, ext)), (f, ext)      # the traced frames are the same
        assert rb("tm2.f%03d.denoised.pfm" % f) != rb("t.f%03d.denoised.pfm" % f), f
        assert rb("tm2.f%03d.denoised.pfm" % f) != rb("tv.f%03d.denoised.pfm" % f), f
        assert rb("tm8.f%03d.denoised.pfm" % f) == rb("tv.f%03d.denoised.pfm" % f), f        # one batch: ptx_denoise_variance
        assert rb("tvm.f%03d.denoised.pfm" % f) == rb("tm2.f%03d.denoised.pfm" % f), f       # --measured implies --variance
    bad = subprocess.run(common + ["--until-error", "0.1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--until-error does not combine with --frames" in bad.stderr


@pytest.mark.parametrize("scene", ["cornell.txt", "cornellObj.txt"])
def test_quality_on_the_orbit_is_printed(gpu_product, scene):
    """the orbit of test_gpu_variance.py's test_on_the_orbit_it_beats_the_fixed_colour_weight (256 x 256, 8 views, steps of left:2,0.5,
    ground truth 1024 spp of the last view): the MSE of the last view's frame through the new call over that of ptx_denoise_variance
    with the handle on the same frames.  Printed, not asserted.  That orbit has 2 spp per view, which cannot make 4 batches: it is run
    (a) as it is, in 2 batches of 1 with min_batches = 2 (q has one degree of freedom), and (b) with 8 spp per view in 4 batches of 2
    at the default min_batches.  Measured on an MI355X: DESIGN.md 10."""
    pt = gpu_product
    W = H = 256
    for spp, size, min_batches in ((2, 1, 2), (8, 2, 4)):
        s, o = _scene(pt, scene, (W, H), depth=8)
        with pt.Temporal(0, W, H) as tn, pt.Temporal(0, W, H) as tv, pt.Moments(0, W, H) as m, pt.Tracer(s) as T:
            for f in range(8):
                if f:
                    _step(s, o, T, 2.0, 0.5, [m])
                _batches(T, m, 0, spp // size, size)
                nden = T.denoise_measured(m, spp, min_batches=min_batches, temporal=tn).astype(np.float64)
                vden = T.denoise_variance(spp, tv).astype(np.float64)
            hit = T.gbuffer()["hit"]
            T.render(spp + 1, 1024 - spp)
            gt = (_image(T) / np.float32(1024)).astype(np.float64)
        mse = lambda a: float(((a - gt)[hit] ** 2).mean())
        print("%s 256x256, 8 views x %d spp in %d batches of %d (min_batches %d): MSE measured + temporal %.4g, ptx_denoise_variance %.4g, ratio %.3f" % (
            scene, spp, spp // size, size, min_batches, mse(nden), mse(vden), mse(nden) / mse(vden)))
        assert np.isfinite(nden).all() and not beq(nden, vden)
