"""GPU: temporal reuse in front of the a-trous denoiser (include/mi355x_pathtracer.h: ptx_denoise_temporal ...).  Without history it is
ptx_denoise bit for bit; the reprojection and mix against their float64 restatement (tests/temporal_ref.py); segments; the history
outliving the tracer; no side effect on what the tracer renders; determinism; a quality floor against a 1024-spp ground truth; and the
surfaces a user meets it through (Python, the C++ veneer, the headless driver, argument checks).  The comparisons with the restatement
here run at the default temporal parameters; tests/test_gpu_temporal_grid.py holds the kernels to it at every other value."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, beq
from temporal_ref import camera_dict, mix, reproject, specular_flags, state

pytestmark = pytest.mark.gpu

DENOISE_KEYS = ("passes", "demodulate", "phi_color", "phi_normal", "phi_position")


def _scene(pt, name, res, depth=8):
    """the scene with runCuda's camera, and the orbit state that camera came from (what the headless driver's --frames steps)"""
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))          # = apply_runcuda_camera, keeping the orbit state
    return s, o


def _step(s, o, T, dx, dy=0.0):
    s.orbit_events(o, [("left", dx, dy)])
    T.set_camera(s)
    T.reset_image()


def _image(T):
    return T.read_image().reshape(T.height, T.width, 3)


def _state_from_device(g, r, spp):
    """the state a call left, from what the device reports (its mix and n_h): the next step's restatement starts from it"""
    n = np.where(g["hit"] & (r["count"] > 0), spp + r["count"].astype(np.float64), float(spp))
    return state(g, r["mix"], n)


@pytest.mark.parametrize("scene", ["cornell.txt", "cornellObj.txt"])
def test_without_history_it_is_ptx_denoise(gpu_product, scene):
    pt = gpu_product
    W, H, spp = 128, 96, 3
    s, o = _scene(pt, scene, (W, H))
    with pt.Tracer(s) as T:
        T.render(1, spp)
        c = (_image(T) / np.float32(spp)).astype(np.float32)
        for prm in ({}, dict(passes=3, demodulate=0), dict(phi_color=4.0, max_history=4, normal_cos=0.5, plane_tolerance=0.1)):
            with pt.Temporal(0, W, H) as tm:
                got = T.denoise_temporal(tm, spp, **prm)
                r = tm.read()
            want = T.denoise(spp, **{k: v for k, v in prm.items() if k in DENOISE_KEYS})
            assert beq(got, want), prm
            assert not r["count"].any() and not r["history"].any() and beq(r["mix"], c), prm
        # max_history = 0: every call of an orbit sequence
        with pt.Temporal(0, W, H) as tm:
            for k in range(3):
                if k:
                    _step(s, o, T, 6.0, 2.0)
                    T.render(1, spp)
                got = T.denoise_temporal(tm, spp, max_history=0)
                assert beq(got, T.denoise(spp)), k
                assert not tm.read()["count"].any()


@pytest.mark.parametrize("scene", ["cornell.txt", "cornellObj.txt", "cornellSpaceship20k.txt"])
def test_reprojection_and_mix_match_the_restatement(gpu_product, scene):
    pt = gpu_product
    W, H, spp = 160, 90, 2
    s, o = _scene(pt, scene, (W, H))
    spec = specular_flags(s.dump()["materials"])
    with pt.Temporal(0, W, H) as tm, pt.Tracer(s) as T:
        T.render(1, spp)
        T.denoise_temporal(tm, spp, read=False)
        prev, prev_cam = _state_from_device(T.gbuffer(), tm.read(), spp), camera_dict(s.camera)
        for dx in (8.0, 40.0):                                         # about 3 and 14 degrees of orbit
            _step(s, o, T, dx, 1.0)
            T.render(1, spp)
            T.denoise_temporal(tm, spp, read=False)
            r, g = tm.read(), T.gbuffer()
            h, nh, near = reproject(prev_cam, g, prev, spec)
            m, _, _ = mix(_image(T), spp, g["hit"], h, nh)
            keep = ~near
            print("%s step %g: %d pixels near a threshold excluded of %d; %d hit pixels inherit, %d do not" % (
                scene, dx, near.sum(), W * H, (g["hit"] & (nh > 0)).sum(), (g["hit"] & (nh == 0)).sum()))
            assert near.sum() < 0.001 * W * H, near.sum()
            for name, got, ref in (("history", r["history"], h), ("count", r["count"], nh), ("mix", r["mix"], m)):
                ok = np.isclose(got[keep].astype(np.float64), ref[keep], rtol=1e-4, atol=1e-3)
                assert ok.all(), (name, np.abs(got[keep] - ref[keep]).max())
            assert (keep & g["hit"] & (nh > 0)).sum() > 0 and (keep & g["hit"] & (nh == 0)).sum() > 0
            plain = keep & (nh == 0)                                   # no history: mix is c exactly
            assert beq(r["mix"][plain], (_image(T) / np.float32(spp)).astype(np.float32)[plain])
            prev, prev_cam = _state_from_device(g, r, spp), camera_dict(s.camera)


def test_segments(gpu_product):
    pt = gpu_product
    W, H = 128, 96
    s, o = _scene(pt, "cornellObj.txt", (W, H))
    with pt.Temporal(0, W, H) as tm, pt.Tracer(s) as T:
        T.render(1, 2)
        T.denoise_temporal(tm, 2)
        _step(s, o, T, 6.0)
        T.render(1, 2)
        T.denoise_temporal(tm, 2)
        r1 = tm.read()
        assert (r1["count"] > 0).sum() > W * H // 4

        def check_mix(r, spp):
            c = (_image(T) / np.float32(spp)).astype(np.float32)
            nh = r["count"].astype(np.float64)
            want = (spp * c.astype(np.float64) + nh[..., None] * r["history"]) / (spp + nh)[..., None]
            use = nh > 0
            assert np.allclose(r["mix"][use], want[use], rtol=1e-5, atol=1e-6)
            assert beq(r["mix"][~use], c[~use])

        # the same camera again, more samples: the same history, mixed with the whole accumulation
        T.render(3, 2)
        T.denoise_temporal(tm, 4)
        r2 = tm.read()
        assert beq(r2["history"], r1["history"]) and beq(r2["count"], r1["count"])
        check_mix(r2, 4)
        # ptx_reset_image with the same camera, new iterations: still that history, nothing counted twice
        T.reset_image()
        T.render(5, 3)
        T.denoise_temporal(tm, 3)
        r3 = tm.read()
        assert beq(r3["history"], r1["history"]) and beq(r3["count"], r1["count"])
        check_mix(r3, 3)
        # ptx_temporal_reset: no history again, ptx_denoise bit for bit
        tm.reset()
        assert beq(T.denoise_temporal(tm, 3), T.denoise(3))
        assert not tm.read()["count"].any()


def test_the_history_outlives_the_tracer(gpu_product):
    pt = gpu_product
    W, H, spp = 96, 64, 2
    s, o = _scene(pt, "cornellObj.txt", (W, H))
    with pt.Temporal(0, W, H) as ta, pt.Temporal(0, W, H) as tb, pt.Tracer(s) as B:
        for k in range(4):
            if k:
                _step(s, o, B, 5.0, 1.0)
            with pt.Tracer(s) as A:                                    # the veneer loop: a new tracer per camera
                A.render(1, spp)
                a = A.denoise_temporal(ta, spp)
            B.render(1, spp)
            b = B.denoise_temporal(tb, spp)
            assert beq(a, b), k
            ra, rb = ta.read(), tb.read()
            for key in ra:
                assert beq(ra[key], rb[key]), (k, key)
        assert (rb["count"] > 0).any()


def test_no_side_effects_on_the_tracer(gpu_product):
    pt = gpu_product
    s, o = _scene(pt, "cornellObj.txt", (160, 90))
    for ahead in (True, False):
        with pt.Temporal(0, 160, 90) as tm, pt.Tracer(s) as A, pt.Tracer(s) as B:
            A.set_render_ahead(ahead)
            B.set_render_ahead(ahead)
            for it in range(1, 7):
                A.pathtrace(it)
                B.pathtrace(it)
                if it in (2, 3, 5):
                    before = A.read_image()
                    A.denoise_temporal(tm, it)
                    A.denoise_temporal(tm, it, max_history=3)
                    assert beq(A.read_image(), before)
                assert beq(A.read_image(), B.read_image()), (ahead, it)
                assert A.stats()["rays_per_bounce"] == B.stats()["rays_per_bounce"], (ahead, it)


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
                out.append(T.denoise_temporal(tm, 2))
                out.extend(tm.read().values())
        runs.append(out)
    for a, b in zip(*runs):
        assert beq(a, b)


@pytest.mark.parametrize("scene", ["cornell.txt", "cornellObj.txt"])
def test_eight_frames_of_two_samples_beat_the_current_frame(gpu_product, scene):
    pt = gpu_product
    W = H = 256
    s, o = _scene(pt, scene, (W, H), depth=8)
    with pt.Temporal(0, W, H) as tm, pt.Tracer(s) as T:
        for f in range(8):
            if f:
                _step(s, o, T, 2.0, 0.5)
            T.render(1, 2)                                             # the reference's loop: iteration restarts at 1
            tden = T.denoise_temporal(tm, 2).astype(np.float64)
        r = tm.read()
        cur = (_image(T) / np.float32(2)).astype(np.float64)
        sden = T.denoise(2).astype(np.float64)
        hit = T.gbuffer()["hit"]
        T.render(3, 1022)
        gt = (_image(T) / np.float32(1024)).astype(np.float64)
    mse = lambda a: float(((a - gt)[hit] ** 2).mean())
    r_mix, r_den = mse(r["mix"].astype(np.float64)) / mse(cur), mse(tden) / mse(sden)
    print("%s 256x256, 8 frames x 2 spp: MSE current %.4g, mix %.4g (ratio %.3f); spatial %.4g, temporal denoised %.4g (ratio %.3f); "
          "%.1f %% of hit pixels inherit, mean n_h %.2f" % (scene, mse(cur), mse(r["mix"].astype(np.float64)), r_mix, mse(sden), mse(tden),
                                                            r_den, 100.0 * (r["count"][hit] > 0).mean(), r["count"][hit].mean()))
    assert r_mix <= 0.5, r_mix
    assert r_den <= 0.8, r_den


def test_cpp_veneer_loop_matches_the_python_sequence(gpu_product, tmp_path):
    pt = gpu_product
    exe = tmp_path / "temporal_veneer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "temporal_veneer_check.cpp"),
                           "-L" + os.path.join(ROOT, "mygpuraytracer_amd"), "-lmi355x_pathtracer", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mygpuraytracer_amd") + ",-rpath,/opt/rocm/lib"])
    W, H, D, N, F, DX = 96, 64, 6, 3, 3, 5.0
    scene = os.path.join(ROOT, "scenes", "cornellObj.txt")
    out = subprocess.check_output([str(exe), scene, str(W), str(H), str(D), str(N), str(F), "%g" % DX, str(tmp_path / "v")], text=True,
                                  timeout=300)
    assert "temporal veneer ok" in out
    rd = lambda f, ext, dt: np.frombuffer(open("%s.f%d%s" % (tmp_path / "v", f, ext), "rb").read(), dt)
    s, o = _scene(pt, "cornellObj.txt", (W, H), depth=D)
    with pt.Temporal(0, W, H) as tm:
        for f in range(1, F + 1):
            if f > 1:
                s.orbit_events(o, [("left", DX, 0.0)])
            with pt.Tracer(s) as T:
                T.render(1, N)
                frame = T.denoise_temporal(tm, N)
                assert beq(rd(f, ".output", np.float32).reshape(H, W, 3), frame), f
                assert np.array_equal(rd(f, ".pbo", np.uint8).reshape(-1, 4), T.denoised_pbo(frame)), f
        assert (tm.read()["count"] > 0).any()


def test_headless_frames_with_temporal_reuse(gpu_product, tmp_path):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    scene = os.path.join(ROOT, "scenes", "cornellObj.txt")
    common = [exe, scene, "--res", "80", "48", "--iterations", "2", "--frames", "3", "--frame-step", "left:4,1", "--denoise"]
    for extra, prefix in ((["--temporal"], "t"), ([], "s")):
        r = subprocess.run(common + extra + ["--out", str(tmp_path / prefix)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    names = sorted(p for p in os.listdir(tmp_path) if p.startswith("t."))
    assert names == ["t.f%03d%s.png" % (f, d) for f in (1, 2, 3) for d in (".denoised", "")], names
    rb = lambda n: open(tmp_path / n, "rb").read()
    for n in names:
        assert rb(n)[:8] == b"\x89PNG\r\n\x1a\n"
    assert rb("t.f001.denoised.png") == rb("s.f001.denoised.png")   # no history on the first frame
    for f in (1, 2, 3):
        assert rb("t.f%03d.png" % f) == rb("s.f%03d.png" % f)       # the traced frames are the same
    assert rb("t.f003.denoised.png") != rb("s.f003.denoised.png")
    r = subprocess.run([exe, scene, "--temporal"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--denoise" in r.stderr


def test_bad_arguments_raise_with_a_message(gpu_product):
    pt = gpu_product
    s, _ = _scene(pt, "cornell.txt", (64, 64))
    with pt.Tracer(s) as T, pt.Temporal(0, 64, 64) as tm:
        with pytest.raises(pt.PathTracerError, match="ptx_temporal_read"):
            tm.read()
        T.render(1, 1)
        with pytest.raises(pt.PathTracerError, match="spp"):
            T.denoise_temporal(tm, 0)
        for bad, what in ((dict(max_history=-1), "max_history"), (dict(normal_cos=2.0), "normal_cos"),
                          (dict(plane_tolerance=-1.0), "plane_tolerance"), (dict(passes=0), "passes")):
            with pytest.raises(pt.PathTracerError, match=what):
                T.denoise_temporal(tm, 1, **bad)
        with pt.Temporal(0, 64, 32) as other:
            with pytest.raises(pt.PathTracerError, match="size"):
                T.denoise_temporal(other, 1)
        if pt.load_library().ptx_device_count() > 1:
            with pt.Temporal(1, 64, 64) as elsewhere:
                with pytest.raises(pt.PathTracerError, match="device"):
                    T.denoise_temporal(elsewhere, 1)
    with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as Tt, pt.Temporal(0, 64, 64) as tm:
        Tt.render(1, 1)
        with pytest.raises(pt.PathTracerError, match="row tile"):
            Tt.denoise_temporal(tm, 1)
