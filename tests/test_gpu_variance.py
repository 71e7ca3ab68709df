"""GPU: variance guidance of the a-trous denoiser (include/mi355x_pathtracer.h: ptx_denoise_variance ...).  The filter and the spatial
estimate against their float64 restatement (tests/variance_ref.py) on random buffers; the tracer path (V, v0, mix, denoised frame) over an
orbit, with the spatial fallback after a plain ptx_denoise_temporal and a same-segment recomputation; nothing else moves; determinism;
quality against the fixed-phi_color filter on the orbit and on a stopped camera; the C++ veneer and the headless driver."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from atrous_ref import random_frame
from conftest import ROOT, beq
from temporal_ref import camera_dict, mix, reproject, specular_flags, state
from variance_ref import atrous_variance, demodulated, denoise_buffers_variance, spatial_variance, temporal_variance

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


def _step(s, o, T, dx, dy=0.0):
    s.orbit_events(o, [("left", dx, dy)])
    T.set_camera(s)
    T.reset_image()


def _image(T):
    return T.read_image().reshape(T.height, T.width, 3)


def _ids(g):
    return np.stack([g["material"], g["geom"]], -1)


@pytest.mark.parametrize("shape", [(61, 97), (1, 1), (700, 3)])
def test_buffers_match_the_restatement(gpu_product, shape):
    pt = gpu_product
    h, w = shape
    f = random_frame(h, w, seed=h * 1000 + w)
    rng = np.random.default_rng(h + w)
    ids = rng.integers(0, 2, (h, w, 2)).astype(np.int32)
    var = (rng.random((h, w)) * 0.3).astype(np.float32)
    var[rng.random((h, w)) < 0.05] = 0.0
    worst = 0.0
    for passes in (1, 3, 5):
        for demod in (1, 0):
            for given, use_ids in ((True, False), (False, True), (False, False)):
                kw = dict(passes=passes, demodulate=demod)
                args = (f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"])
                got, gv = pt.denoise_buffers_variance(*args, ids=ids if use_ids else None, variance=var if given else None, **kw)
                ref, rv, _ = denoise_buffers_variance(*args, ids=ids if use_ids else None, variance=var if given else None, **kw)
                ec, ev = _err(got, ref), _err(gv, rv)
                print("%dx%d passes %d demodulate %d %s: colour %.3g, variance %.3g" % (
                    w, h, passes, demod, "given variance" if given else "spatial estimate" + (" with ids" if use_ids else ""), ec, ev))
                worst = max(worst, ec, ev)
                assert ec <= TOL and ev <= TOL, (shape, passes, demod, given, use_ids, ec, ev)
                assert not gv[~f["hit"]].any()
    print("largest error %.3g" % worst)


def test_tracer_path_matches_the_restatement_over_an_orbit(gpu_product):
    pt = gpu_product
    W, H, spp = 160, 90, 2
    s, o = _scene(pt, "cornellObj.txt", (W, H))
    spec = specular_flags(s.dump()["materials"])
    dp, vp = pt.default_denoise_params(), pt.default_variance_params()
    geo = dict(phi_normal=dp.phi_normal, phi_position=dp.phi_position)

    def check(T, tm, n_spp, prev, prev_cam, label):
        """one ptx_denoise_variance with the handle against the restatement; prev: the committed history (with "V", or None / without)"""
        frame = T.denoise_variance(n_spp, tm)
        r, g, var = tm.read(), T.gbuffer(), T.variance()
        hit = g["hit"]
        c = (_image(T) / np.float32(n_spp)).astype(np.float32)
        near = np.zeros((H, W), bool)
        if prev is None:
            assert not r["count"].any() and beq(r["mix"], c), label
            n = np.full((H, W), float(n_spp))
        else:
            h, nh, near = reproject(prev_cam, g, prev, spec)
            m, n, _ = mix(_image(T), n_spp, hit, h, nh)
            assert near.sum() < 0.001 * W * H
            assert np.isclose(r["mix"][~near].astype(np.float64), m[~near], rtol=1e-4, atol=1e-3).all(), label
            assert np.isclose(r["count"][~near], nh[~near], rtol=1e-4, atol=1e-3).all(), label
        col, f = demodulated(r["mix"], g["albedo"], hit)
        var_s = spatial_variance(col, g["normal"], g["position"], hit, _ids(g), vp.spatial_radius, **geo)
        if prev is not None and "V" in prev:
            V = temporal_variance(prev_cam, g, prev, spec, c, n_spp)
            inherits = np.isfinite(V) & hit
            v0 = np.where(np.isfinite(V), V / n, var_s)
            assert (inherits & (nh > 0)).sum() > W * H // 4, label
        else:
            inherits = np.zeros((H, W), bool)
            v0 = var_s
        keep = ~near
        e_in = _err(var["input"][keep], v0[keep])
        # the filter on what the device fed it: its own mix and v0
        want, want_v = atrous_variance(col, var["input"], g["normal"], g["position"], hit, dp.passes, vp.phi_luminance, vp.epsilon,
                                       vp.prefilter, **geo)
        e_out, e_v = _err(frame, want * f), _err(var["output"], want_v)
        print("%s: %d pixels inherit V, %d take the spatial estimate; v0 %.3g, denoised %.3g, filtered variance %.3g" % (
            label, inherits.sum(), (hit & ~inherits).sum(), e_in, e_out, e_v))
        assert e_in <= TOL and e_out <= TOL and e_v <= TOL, (label, e_in, e_out, e_v)
        assert not var["input"][~hit].any() and not var["output"][~hit].any()
        n_dev = np.where(hit & (r["count"] > 0), n_spp + r["count"].astype(np.float64), float(n_spp))
        st = state(g, r["mix"], n_dev)
        st["V"] = var["input"].astype(np.float64) * n_dev
        return st

    with pt.Temporal(0, W, H) as tm, pt.Tracer(s) as T:
        T.render(1, spp)
        st0, cam0 = check(T, tm, spp, None, None, "frame 1 (no history)"), camera_dict(s.camera)
        _step(s, o, T, 8.0, 1.0)
        T.render(1, spp)
        st1, cam1 = check(T, tm, spp, st0, cam0, "frame 2 (history with V)"), camera_dict(s.camera)
        T.render(spp + 1, 6)                                           # the same segment, recomputed from the same history with 8 spp
        st1 = check(T, tm, spp + 6, st0, cam0, "frame 2 again, 8 spp")
        _step(s, o, T, 8.0, 1.0)
        T.render(1, spp)
        T.denoise_temporal(tm, spp)                                    # the old call: the state it leaves carries no V
        r, g = tm.read(), T.gbuffer()
        st2 = state(g, r["mix"], np.where(g["hit"] & (r["count"] > 0), spp + r["count"].astype(np.float64), float(spp)))
        cam2 = camera_dict(s.camera)
        _step(s, o, T, 8.0, 1.0)
        T.render(1, spp)
        check(T, tm, spp, st2, cam2, "frame 4 (history without V: spatial fallback)")
        assert (tm.read()["count"] > 0).any()
        # without a handle: the spatial estimate of rgb / spp
        frame = T.denoise_variance(spp)
        g, var = T.gbuffer(), T.variance()
        c = (_image(T) / np.float32(spp)).astype(np.float32)
        col, f = demodulated(c, g["albedo"], g["hit"])
        v0 = spatial_variance(col, g["normal"], g["position"], g["hit"], _ids(g), vp.spatial_radius, **geo)
        want, _ = atrous_variance(col, var["input"], g["normal"], g["position"], g["hit"], dp.passes, vp.phi_luminance, vp.epsilon,
                                  vp.prefilter, **geo)
        assert _err(var["input"], v0) <= TOL and _err(frame, want * f) <= TOL


def test_nothing_else_moves(gpu_product):
    pt = gpu_product
    W, H = 160, 90
    for ahead in (True, False):
        sa, oa = _scene(pt, "cornellObj.txt", (W, H))
        sb, ob = _scene(pt, "cornellObj.txt", (W, H))
        with pt.Temporal(0, W, H) as ta, pt.Temporal(0, W, H) as tb, pt.Tracer(sa) as A, pt.Tracer(sb) as B:
            A.set_render_ahead(ahead)
            B.set_render_ahead(ahead)
            for k in range(4):
                if k:
                    _step(sa, oa, A, 6.0, 1.0)
                    _step(sb, ob, B, 6.0, 1.0)
                for it in (1, 2):
                    A.pathtrace(it)
                    B.pathtrace(it)
                before = A.read_image()
                # A: the new call before, between and after the old ones (k = 3: the new call is the segment's last)
                A.denoise_variance(2, ta)
                A.denoise_variance(2)
                a_t = A.denoise_temporal(ta, 2)
                ra = ta.read()
                A.denoise_variance(2, ta, phi_luminance=1.0)
                a_d = A.denoise(2)
                if k != 2:
                    A.denoise_variance(2, ta)
                else:
                    A.denoise_temporal(ta, 2)
                assert beq(a_t, B.denoise_temporal(tb, 2)), (ahead, k)
                rb = tb.read()
                for key in ra:
                    assert beq(ra[key], rb[key]), (ahead, k, key)
                assert beq(a_d, B.denoise(2)), (ahead, k)
                assert beq(A.read_image(), before) and beq(before, B.read_image()), (ahead, k)
                assert A.stats()["rays_per_bounce"] == B.stats()["rays_per_bounce"], (ahead, k)
            assert (rb["count"] > 0).any()


def test_deterministic(gpu_product):
    pt = gpu_product
    W, H = 128, 96
    runs = []
    for _ in range(2):
        s, o = _scene(pt, "cornell.txt", (W, H))
        out = []
        with pt.Temporal(0, W, H) as tm, pt.Tracer(s) as T:
            for k in range(3):
                if k:
                    _step(s, o, T, 7.0, -2.0)
                T.render(1, 2)
                out.append(T.denoise_variance(2, tm))
                out.extend(T.variance().values())
                out.extend(tm.read().values())
            out.append(T.denoise_variance(2))
            out.extend(T.variance().values())
        runs.append(out)
    for a, b in zip(*runs):
        assert beq(a, b)


@pytest.mark.parametrize("scene", ["cornell.txt", "cornellObj.txt"])
def test_on_the_orbit_it_beats_the_fixed_colour_weight(gpu_product, scene):
    """the setup of test_gpu_temporal.py's test_eight_frames_of_two_samples_beat_the_current_frame, every default: the yardstick is
    ptx_denoise_temporal on the same frames, no margin.  Against ptx_denoise_temporal at max_history = 4 (the fixed filter's best
    displayed frame): printed, not asserted."""
    pt = gpu_product
    W = H = 256
    s, o = _scene(pt, scene, (W, H), depth=8)
    with pt.Temporal(0, W, H) as tv, pt.Temporal(0, W, H) as tt, pt.Temporal(0, W, H) as t4, pt.Tracer(s) as T:
        for f in range(8):
            if f:
                _step(s, o, T, 2.0, 0.5)
            T.render(1, 2)
            vden = T.denoise_variance(2, tv).astype(np.float64)
            tden = T.denoise_temporal(tt, 2).astype(np.float64)
            t4den = T.denoise_temporal(t4, 2, max_history=4).astype(np.float64)
        hit = T.gbuffer()["hit"]
        T.render(3, 1022)
        gt = (_image(T) / np.float32(1024)).astype(np.float64)
    mse = lambda a: float(((a - gt)[hit] ** 2).mean())
    print("%s 256x256, 8 frames x 2 spp: MSE variance-guided %.4g, fixed phi_color %.4g (ratio %.3f), fixed at max_history 4 %.4g (ratio %.3f)" % (
        scene, mse(vden), mse(tden), mse(vden) / mse(tden), mse(t4den), mse(vden) / mse(t4den)))
    assert mse(vden) <= mse(tden), (mse(vden), mse(tden))


@pytest.mark.parametrize("scene", ["cornell.txt", "cornellObj.txt"])
def test_on_a_stopped_camera_it_beats_the_fixed_colour_weight(gpu_product, scene):
    pt = gpu_product
    W = H = 256
    s, o = _scene(pt, scene, (W, H), depth=8)
    with pt.Tracer(s) as T:
        T.render(1, 1024)
        cur = (_image(T) / np.float32(1024)).astype(np.float64)
        vden = T.denoise_variance(1024).astype(np.float64)
        sden = T.denoise(1024).astype(np.float64)
        hit = T.gbuffer()["hit"]
        T.render(1025, 16384 - 1024)
        gt = (_image(T) / np.float32(16384)).astype(np.float64)
    mse = lambda a: float(((a - gt)[hit] ** 2).mean())
    print("%s 256x256, 1024 spp against 16384: MSE unfiltered %.4g, variance-guided %.4g (x %.3f), fixed phi_color %.4g (x %.3f)" % (
        scene, mse(cur), mse(vden), mse(vden) / mse(cur), mse(sden), mse(sden) / mse(cur)))
    assert mse(vden) <= mse(sden), (mse(vden), mse(sden))


@pytest.mark.parametrize("temporal", [1, 0])
def test_cpp_veneer_loop_matches_the_python_sequence(gpu_product, tmp_path, temporal):
    pt = gpu_product
    exe = tmp_path / "variance_veneer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "variance_veneer_check.cpp"),
                           "-L" + os.path.join(ROOT, "mygpuraytracer_amd"), "-lmi355x_pathtracer", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mygpuraytracer_amd") + ",-rpath,/opt/rocm/lib"])
    W, H, D, N, F, DX = 96, 64, 6, 3, 4, 5.0
    scene = os.path.join(ROOT, "scenes", "cornellObj.txt")
    out = subprocess.check_output([str(exe), scene, str(W), str(H), str(D), str(N), str(F), "%g" % DX, str(tmp_path / "v"), str(temporal)],
                                  text=True, timeout=300)
    assert "variance veneer ok" in out
    rd = lambda f, ext, dt: np.frombuffer(open("%s.f%d%s" % (tmp_path / "v", f, ext), "rb").read(), dt)
    s, o = _scene(pt, "cornellObj.txt", (W, H), depth=D)
    with pt.Temporal(0, W, H) as tm:
        for f in range(1, F + 1):
            if f > 1:
                s.orbit_events(o, [("left", DX, 0.0)])
            with pt.Tracer(s) as T:
                T.render(1, N)
                frame = T.denoise_variance(N, tm if temporal else None)
                assert beq(rd(f, ".output", np.float32).reshape(H, W, 3), frame), f
                assert np.array_equal(rd(f, ".pbo", np.uint8).reshape(-1, 4), T.denoised_pbo(frame)), f
                if f == F:
                    assert not beq(frame, T.denoise_temporal(tm, N) if temporal else T.denoise(N))


def test_headless_frames_with_variance(gpu_product, tmp_path):
    pt = gpu_product
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    scene = os.path.join(ROOT, "scenes", "cornellObj.txt")
    W, H, N, F = 80, 48, 2, 4
    common = [exe, scene, "--res", str(W), str(H), "--iterations", str(N), "--frames", str(F), "--frame-step", "left:4,1", "--denoise", "--pfm"]
    for extra, prefix in ((["--temporal", "--variance"], "tv"), (["--variance", "--phi-luminance", "2"], "v2"), (["--temporal"], "t")):
        r = subprocess.run(common + extra + ["--out", str(tmp_path / prefix)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr

    def pfm(name):
        return np.frombuffer(open(tmp_path / name, "rb").read().split(b"\n", 3)[3], np.float32).reshape(H, W, 3)

    s = pt.Scene(scene, res=(W, H))                        # (the depth is the scene file's, as the driver's)
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))
    with pt.Temporal(0, W, H) as tm:
        for f in range(1, F + 1):
            if f > 1:
                s.orbit_events(o, [("left", 4.0, 1.0)])
            with pt.Tracer(s) as T:
                T.render(1, N)
                tv = T.denoise_variance(N, tm)
                v2 = T.denoise_variance(N, phi_luminance=2.0)
            for got, want in ((pfm("tv.f%03d.denoised.pfm" % f), tv), (pfm("v2.f%03d.denoised.pfm" % f), v2)):
                assert beq(got, want[::-1]), f                         # a .pfm stores its rows bottom up
    rb = lambda n: open(tmp_path / n, "rb").read()
    assert rb("tv.f%03d.denoised.png" % F) != rb("t.f%03d.denoised.png" % F)
    for f in range(1, F + 1):
        assert rb("tv.f%03d.png" % f) == rb("t.f%03d.png" % f)         # the traced frames are the same
    r = subprocess.run([exe, scene, "--variance"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--denoise" in r.stderr


def test_bad_arguments_raise_with_a_message(gpu_product):
    pt = gpu_product
    s, _ = _scene(pt, "cornell.txt", (64, 64))
    with pt.Tracer(s) as T, pt.Temporal(0, 64, 64) as tm:
        with pytest.raises(pt.PathTracerError, match="ptx_read_variance"):
            T.variance()
        T.render(1, 1)
        with pytest.raises(pt.PathTracerError, match="spp"):
            T.denoise_variance(0, tm)
        for bad, what in ((dict(phi_luminance=-1.0), "phi_luminance"), (dict(epsilon=0.0), "epsilon"), (dict(spatial_radius=4), "spatial_radius"),
                          (dict(max_history=-1), "max_history"), (dict(passes=0), "passes")):
            with pytest.raises(pt.PathTracerError, match=what):
                T.denoise_variance(1, tm, **bad)
        with pytest.raises(pt.PathTracerError, match="demodulate"):
            T.denoise_variance(1, tm, demodulate=0)
        T.denoise_variance(1, demodulate=0)                            # without a handle that is allowed
        with pt.Temporal(0, 64, 32) as other:
            with pytest.raises(pt.PathTracerError, match="size"):
                T.denoise_variance(1, other)
    with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as Tt:
        Tt.render(1, 1)
        with pytest.raises(pt.PathTracerError, match="row tile"):
            Tt.denoise_variance(1)
