"""GPU: the a-trous denoiser (include/mi355x_pathtracer.h: ptx_denoise ...).  The G-buffer against the CPU oracle bit for bit, the
filter against its float64 restatement (tests/atrous_ref.py), no side effect on what the tracer renders, a quality floor against a
1024-spp ground truth, and the surfaces a user meets it through (Python, the C++ veneer, the headless driver, argument checks)."""
import os
import subprocess

import numpy as np
import pytest

from atrous_ref import atrous, random_frame
from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture()
def O(oracle_lib):
    oracle_lib.set_libm(1)
    yield oracle_lib
    oracle_lib.set_libm(0)


def _scene(pt, name, res, depth=8):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s


def _params(**kw):
    """the library's defaults with overrides, as keyword arguments of atrous() / denoise() / denoise_buffers()"""
    import mygpuraytracer_amd as pt
    p = pt.default_denoise_params(**kw)
    return dict(passes=p.passes, demodulate=bool(p.demodulate), phi_color=p.phi_color, phi_normal=p.phi_normal, phi_position=p.phi_position)


def _within(gpu, ref):
    err = np.abs(gpu.astype(np.float64) - ref)
    ok = err <= TOL * (np.abs(ref) + 1e-3)
    return bool(ok.all()), float((err / (np.abs(ref) + 1e-3)).max())


@pytest.mark.parametrize("scene,res", [("cornell.txt", (200, 200)), ("cornellObj.txt", (160, 90)), ("cornellSpaceship20k.txt", (160, 90))])
def test_gbuffer_bit_identical_to_the_oracle(gpu_product, O, scene, res):
    pt = gpu_product
    s = _scene(pt, scene, res)
    d = s.dump()
    O.create(d, d["textures"])
    O.set_options(aa=0, dof=0)
    O.pt_init()
    O.pt_generate(1)
    op = O.paths()
    oi = O.compute_intersections(op)
    with pt.Tracer(s) as T:                          # (antialiasing on: the G-buffer never jitters)
        g = T.gbuffer()
    H, W = res[1], res[0]
    hit = (oi["t"] > 0).reshape(H, W)
    assert hit.sum() > H * W // 4
    assert np.array_equal(g["hit"], hit)
    assert beq(g["t"][hit], oi["t"].reshape(H, W)[hit])
    assert beq(g["normal"][hit], oi["normal"].reshape(H, W, 3)[hit])
    assert beq(g["material"][hit], oi["materialId"].reshape(H, W)[hit]) and beq(g["geom"][hit], oi["geomId"].reshape(H, W)[hit])
    pos = (op["origin"] + oi["t"][:, None] * op["direction"]).astype(np.float32).reshape(H, W, 3)     # float32, no contraction
    assert beq(g["position"][hit], pos[hit])
    for k in ("position", "normal", "albedo", "t", "material", "geom"):
        assert not g[k][~hit].any(), k
    # albedo: the apps variant's AOV of iteration 1 (write_albedo); the first hit does not depend on the depth
    O.set_apps_variant(1)
    O.set_depth(1)
    O.pt_init()
    O.iterate(1)
    assert beq(g["albedo"].reshape(-1, 3), O.albedo())
    O.set_apps_variant(0)
    # antialiasing and depth of field change nothing: the guides are the sharp pinhole view
    with pt.Tracer(s, antialiasing=1, depth_of_field=1) as T2:
        g2 = T2.gbuffer()
    for k in g:
        assert beq(g2[k], g[k]), k


@pytest.mark.parametrize("h,w", [(61, 97), (1, 1), (3, 700)])
def test_filter_matches_the_restatement_on_random_buffers(gpu_product, h, w):
    pt = gpu_product
    f = random_frame(h, w, 100 + w)
    worst = 0.0
    for passes in (1, 3, 5):
        for demod in (False, True):
            prm = _params(passes=passes, demodulate=demod)
            got = pt.denoise_buffers(f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"], **prm)
            ref = atrous(f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"], **prm)
            ok, e = _within(got, ref)
            worst = max(worst, e)
            assert ok, (passes, demod, e)
            assert np.array_equal(got[~f["hit"]], f["rgb"][~f["hit"]])
    print("random %dx%d: max relative error %.3g" % (w, h, worst))


def test_filter_matches_the_restatement_on_a_rendered_frame(gpu_product):
    pt = gpu_product
    s = _scene(pt, "cornellObj.txt", (480, 270))
    with pt.Tracer(s) as T:
        T.render(1, 4)
        img = T.read_image()
        g = T.gbuffer()
        rgb = (img / np.float32(4)).astype(np.float32).reshape(270, 480, 3)
        worst = 0.0
        for passes in (1, 3, 5):
            for demod in (False, True):
                prm = _params(passes=passes, demodulate=demod)
                got = T.denoise(4, **prm)
                ref = atrous(rgb, g["albedo"], g["normal"], g["position"], g["hit"], **prm)
                ok, e = _within(got, ref)
                worst = max(worst, e)
                assert ok, (passes, demod, e)
                # the tracer-level call is the filter alone fed with its own G-buffer and image / spp
                assert beq(got, pt.denoise_buffers(rgb, g["albedo"], g["normal"], g["position"], g["hit"], **prm))
        print("C4 480x270 4 spp: max relative error %.3g" % worst)


def test_denoise_is_deterministic_and_leaves_the_tracer_alone(gpu_product):
    pt = gpu_product
    s = _scene(pt, "cornellObj.txt", (160, 90))
    for ahead in (True, False):
        with pt.Tracer(s) as A, pt.Tracer(s) as B:
            A.set_render_ahead(ahead)
            B.set_render_ahead(ahead)
            for it in range(1, 7):
                A.pathtrace(it)
                B.pathtrace(it)
                if it in (2, 5):
                    before = A.read_image()
                    d1 = A.denoise(it)
                    d2 = A.denoise(it)
                    assert beq(d1, d2)
                    assert beq(A.read_image(), before)
                assert beq(A.read_image(), B.read_image()), (ahead, it)
                assert A.stats()["rays_per_bounce"] == B.stats()["rays_per_bounce"], (ahead, it)


def test_set_camera_makes_the_next_denoise_use_the_new_view(gpu_product):
    pt = gpu_product
    s = _scene(pt, "cornellObj.txt", (128, 96))
    with pt.Tracer(s) as T:
        T.render(1, 2)
        g0 = T.gbuffer()
        T.denoise(2)
        o = s.orbit_init()
        s.orbit_events(o, [("left", 40.0, 10.0)])
        T.set_camera(s)
        g1 = T.gbuffer()
        assert not beq(g1["position"], g0["position"])
        with pt.Tracer(s) as fresh:
            gf = fresh.gbuffer()
        for k in g1:
            assert beq(g1[k], gf[k]), k
        T.reset_image()
        T.render(1, 2)
        rgb = (T.read_image() / np.float32(2)).astype(np.float32).reshape(96, 128, 3)
        assert beq(T.denoise(2), pt.denoise_buffers(rgb, gf["albedo"], gf["normal"], gf["position"], gf["hit"]))


@pytest.mark.parametrize("scene", ["cornell.txt", "cornellObj.txt"])
def test_denoised_4spp_frame_halves_the_error(gpu_product, scene):
    pt = gpu_product
    s = _scene(pt, scene, (256, 256))
    with pt.Tracer(s) as T:
        T.render(1, 4)
        noisy = (T.read_image() / np.float32(4)).reshape(256, 256, 3).astype(np.float64)
        den = T.denoise(4).astype(np.float64)
        hit = T.gbuffer()["hit"]
        T.render(5, 1020)
        gt = (T.read_image() / np.float32(1024)).reshape(256, 256, 3).astype(np.float64)
    mse = lambda a: float(((a - gt)[hit] ** 2).mean())
    ratio = mse(den) / mse(noisy)
    print("%s 256x256: MSE noisy %.4g, denoised %.4g, ratio %.3f" % (scene, mse(noisy), mse(den), ratio))
    assert ratio <= 0.5, ratio


def test_cpp_veneer_gpudenoise_then_sendtogpu(gpu_product, tmp_path):
    pt = gpu_product
    exe = tmp_path / "denoise_veneer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "denoise_veneer_check.cpp"),
                           "-L" + os.path.join(ROOT, "mygpuraytracer_amd"), "-lmi355x_pathtracer", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mygpuraytracer_amd") + ",-rpath,/opt/rocm/lib"])
    W, H, D, N = 96, 64, 6, 4
    scene = os.path.join(ROOT, "scenes", "cornellObj.txt")
    out = subprocess.check_output([str(exe), scene, str(W), str(H), str(D), str(N), str(tmp_path / "v")], text=True)
    assert "denoise veneer ok" in out
    rd = lambda ext, dt: np.frombuffer(open(str(tmp_path / "v") + ext, "rb").read(), dt)
    s = pt.Scene(scene, res=(W, H), depth=D)
    s.apply_runcuda_camera()
    with pt.Tracer(s) as T:
        T.render(1, N)
        frame = T.denoise(N)
        assert beq(rd(".output", np.float32).reshape(H, W, 3), frame)
        pbo = T.denoised_pbo(frame)                  # k_pbo of that frame (iter 1: no division)
        assert np.array_equal(rd(".pbo", np.uint8).reshape(-1, 4), pbo)
        assert np.array_equal(rd(".pbo_dev", np.uint8).reshape(-1, 4), pbo)
        import torch
        dpbo = torch.full((W * H, 4), 7, dtype=torch.uint8, device="cuda:0")
        T.denoised_pbo_from_device(dpbo.data_ptr())
        T.synchronize()
        assert np.array_equal(dpbo.cpu().numpy(), pbo)
        assert T.device_denoised_ptr()


def test_headless_driver_writes_the_denoised_frame(gpu_product, tmp_path):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    W, H = 80, 48
    r = subprocess.run([exe, os.path.join(ROOT, "scenes", "cornellObj.txt"), "--res", str(W), str(H), "--iterations", "4", "--denoise",
                        "--denoise-passes", "3", "--pfm", "--out", str(tmp_path / "h")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    pngs = sorted(p for p in os.listdir(tmp_path) if p.endswith(".denoised.png"))
    assert len(pngs) == 1, os.listdir(tmp_path)
    data = open(tmp_path / pngs[0], "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    assert (int.from_bytes(data[16:20], "big"), int.from_bytes(data[20:24], "big")) == (W, H)
    pfm = open(tmp_path / pngs[0].replace(".png", ".pfm"), "rb").read()
    assert pfm.startswith(b"PF\n%d %d\n" % (W, H)) and len(pfm) == len(b"PF\n%d %d\n-1.0\n" % (W, H)) + W * H * 12
    # the PFM holds the tracer's denoised frame (bottom row first), with the driver's --denoise-passes
    pt = gpu_product
    s = _scene(pt, "cornellObj.txt", (W, H))
    with pt.Tracer(s) as T:
        T.render(1, 4)
        want = T.denoise(4, passes=3)
    got = np.frombuffer(pfm[-W * H * 12:], np.float32).reshape(H, W, 3)[::-1]
    assert beq(got, want)


def test_bad_arguments_raise_with_a_message(gpu_product):
    pt = gpu_product
    s = _scene(pt, "cornell.txt", (64, 64))
    with pt.Tracer(s) as T:
        with pytest.raises(pt.PathTracerError, match="ptx_read_denoised"):
            T.read_denoised()
        T.render(1, 1)
        for bad, what in ((dict(), "spp"), (dict(passes=0), "passes"), (dict(passes=11), "passes"), (dict(phi_color=0.0), "phi"),
                          (dict(phi_normal=-1.0), "phi"), (dict(phi_position=0.0), "phi")):
            with pytest.raises(pt.PathTracerError, match=what):
                T.denoise(0 if not bad else 1, **bad)
    with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as Tt:
        Tt.render(1, 1)
        with pytest.raises(pt.PathTracerError, match="row tile"):
            Tt.denoise(1)
        with pytest.raises(pt.PathTracerError, match="row tile"):
            Tt.gbuffer()
