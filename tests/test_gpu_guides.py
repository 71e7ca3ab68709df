"""GPU: the denoiser's sampled guides (include/mi355x_pathtracer.h: ptx_set_guide_samples; DESIGN.md 10 "Sampled guides").  k_guides
against the numpy restatement (tests/guides_ref.py) fed by the CPU oracle's camera rays and intersections, bit for bit; the default
mode untouched; the filter entry points fed by the new guides; the refusals; the C++ veneer and the headless driver; and the quality
claim the mode exists for, against a 1024-spp frame."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, beq
from guides_ref import oracle_samples, sampled_guides

pytestmark = pytest.mark.gpu

TOL = 1e-4          # tests/test_gpu_denoise.py's bound, by its metric |gpu - ref| / (|ref| + 1e-3)
FIELDS = ("normal", "position", "t", "hit", "material", "geom", "albedo")


@pytest.fixture()
def O(oracle_lib):
    oracle_lib.set_libm(1)
    yield oracle_lib
    oracle_lib.set_libm(0)


def _scene(pt, name, res, depth=8):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s


def _err(gpu, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(gpu, np.float64) - ref) / (np.abs(ref) + 1e-3)).max())


def _ids(g):
    return np.stack([g["material"], g["geom"]], -1)


def _oracle(O, s, aa, dof):
    d = s.dump()
    O.create(d, d["textures"])
    O.set_options(aa=aa, dof=dof)
    O.pt_init()
    return d


def _same_as_the_restatement(T, ref, W, H, what, albedo=True):
    g = T.gbuffer()
    g["coverage"] = T.guide_coverage()
    for k in FIELDS + ("coverage",):
        if k == "albedo" and not albedo:
            continue
        want = ref[k].reshape((H, W) + ref[k].shape[1:])
        assert beq(g[k], want.astype(g[k].dtype)), (what, k, int((g[k] != want).sum()))
    return g


@pytest.mark.parametrize("aa,dof", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("res", [(37, 23), (1, 1)])
def test_cornell_guides_are_the_restatement_bit_for_bit(gpu_product, O, res, aa, dof):
    pt = gpu_product
    W, H = res
    s = _scene(pt, "cornell.txt", res)
    d = _oracle(O, s, aa, dof)
    samples = {first: list(oracle_samples(O, d, first, 5)) for first in (1, 7)}      # computed once, shared by every K
    partial = 0
    with pt.Tracer(s, antialiasing=aa, depth_of_field=dof) as T:
        for first in (1, 7):
            for K in (1, 2, 5):
                T.set_guide_samples(K, first)
                assert T.guide_samples() == (K, first)
                ref = sampled_guides(samples[first][:K])
                _same_as_the_restatement(T, ref, W, H, (first, K))
                partial += int(((ref["coverage"] > 0) & (ref["coverage"] < 1)).sum() + ref["mixed"].sum())
    if res != (1, 1):
        assert partial > 0          # (the cases meet pixels that more than one surface, or a surface and the background, share)


def test_mesh_scene_guides_are_the_restatement_bit_for_bit(gpu_product, O):
    pt = gpu_product
    W, H = 160, 90
    s = _scene(pt, "cornellObj.txt", (W, H))
    d = _oracle(O, s, 1, 1)
    ref = sampled_guides(oracle_samples(O, d, 1, 3))
    with pt.Tracer(s, antialiasing=1, depth_of_field=1) as T:
        T.set_guide_samples(3)
        _same_as_the_restatement(T, ref, W, H, "cornellObj")
    assert ref["mixed"].any() and ref["hit"].sum() > W * H // 4


def test_textured_bvh_scene_one_sample_and_the_albedo_aov(gpu_product, O):
    pt = gpu_product
    W, H = 160, 90
    s = _scene(pt, "cornellSpaceship20k.txt", (W, H))
    d = _oracle(O, s, 1, 1)
    ref = sampled_guides(oracle_samples(O, d, 1, 1, albedo=None))
    with pt.Tracer(s, antialiasing=1, depth_of_field=1) as T:
        T.set_guide_samples(1, 1)
        g = _same_as_the_restatement(T, ref, W, H, "ship", albedo=False)
    # the albedo: the apps variant's AOV of iteration 1 under the same jitter and lens (the seed holds the depth: it stays)
    O.set_apps_variant(1)
    O.pt_init()
    O.iterate(1)
    aov = O.albedo()
    O.set_apps_variant(0)
    assert beq(g["albedo"].reshape(-1, 3), aov)
    assert len(np.unique(g["albedo"].reshape(-1, 3), axis=0)) > 50          # (textured: more albedos than materials)


def test_the_default_is_the_pixel_centre_mode_untouched(gpu_product):
    pt = gpu_product
    s = _scene(pt, "cornellObj.txt", (96, 64))
    with pt.Tracer(s, depth_of_field=1) as A, pt.Tracer(s, depth_of_field=1) as B:
        assert A.guide_samples() == (0, 1)
        A.render(1, 3)
        B.render(1, 3)
        ga, da = A.gbuffer(), A.denoise(3)
        B.set_guide_samples(4)
        gs, ds = B.gbuffer(), B.denoise(3)
        assert not beq(gs["normal"], ga["normal"]) and not beq(ds, da)
        B.set_guide_samples(0)
        gb, db = B.gbuffer(), B.denoise(3)
        for k in ga:
            assert beq(ga[k], gb[k]), k
        assert beq(da, db)
        assert beq(B.guide_coverage(), gb["hit"].astype(np.float32))
    # nothing jitters and one sample: the pixel-centre record
    with pt.Tracer(s, antialiasing=0, depth_of_field=0) as C:
        gc = C.gbuffer()
        C.set_guide_samples(1)
        g1 = C.gbuffer()
        for k in gc:
            assert beq(gc[k], g1[k]), k
        assert beq(C.guide_coverage(), gc["hit"].astype(np.float32))


def test_the_filters_take_the_sampled_guides(gpu_product):
    pt = gpu_product
    W, H, N = 96, 64, 8
    s = _scene(pt, "cornell.txt", (W, H))
    with pt.Tracer(s, antialiasing=1, depth_of_field=1) as T, pt.Moments(0, W, H) as m:
        T.set_guide_samples(N)
        for it in range(1, N + 1):
            T.pathtrace(it)
            if it % 2 == 0:
                m.add(T, it)
        g = T.gbuffer()
        guides = (g["albedo"], g["normal"], g["position"], g["hit"])
        rgb = (T.read_image() / np.float32(N)).astype(np.float32).reshape(H, W, 3)
        e = _err(T.denoise(N), pt.denoise_buffers(rgb, *guides))
        assert e <= TOL, e
        got = T.denoise_measured(m, N)
        v0 = T.variance()["input"]
        want, _ = pt.denoise_buffers_variance(rgb, *guides, ids=_ids(g), variance=v0)
        e = _err(got, want)
        assert e <= TOL, e
        # more guide samples than the frame has: accepted
        T.set_guide_samples(2 * N)
        T.denoise(N)


def test_camera_and_depth_changes_recompute_the_guides(gpu_product):
    pt = gpu_product
    s = _scene(pt, "cornellObj.txt", (64, 48))
    with pt.Tracer(s, antialiasing=1, depth_of_field=1) as T:
        T.set_guide_samples(3, 2)
        g0 = T.gbuffer()
        s.set_trace_depth(5)                             # the rays' seed holds the depth: other jitter, other guides
        T.set_camera(s)
        g1 = T.gbuffer()
        assert not beq(g1["position"], g0["position"])
        o = s.orbit_init()
        s.orbit_events(o, [("left", 40.0, 10.0)])
        T.set_camera(s)
        g2, c2 = T.gbuffer(), T.guide_coverage()
        assert not beq(g2["position"], g1["position"])
        with pt.Tracer(s, antialiasing=1, depth_of_field=1) as fresh:
            fresh.set_guide_samples(3, 2)
            gf, cf = fresh.gbuffer(), fresh.guide_coverage()
        for k in g2:
            assert beq(g2[k], gf[k]), k
        assert beq(c2, cf)


def test_sampled_guides_leave_the_tracer_alone_and_repeat(gpu_product):
    pt = gpu_product
    s = _scene(pt, "cornellObj.txt", (160, 90))
    with pt.Tracer(s, depth_of_field=1) as A, pt.Tracer(s, depth_of_field=1) as B:
        A.set_guide_samples(4)
        for it in range(1, 6):
            A.pathtrace(it)
            B.pathtrace(it)
            if it in (2, 4):
                before = A.read_image()
                d1, g1 = A.denoise(it), A.gbuffer()
                A.set_guide_samples(0)
                A.set_guide_samples(4)                   # stale: computed again
                d2, g2 = A.denoise(it), A.gbuffer()
                assert beq(d1, d2)
                for k in g1:
                    assert beq(g1[k], g2[k]), k
                assert beq(A.read_image(), before)
            assert beq(A.read_image(), B.read_image()), it
            assert A.stats()["rays_per_bounce"] == B.stats()["rays_per_bounce"], it


def test_refusals_raise_with_their_messages(gpu_product):
    pt = gpu_product
    W, H = 64, 64
    s = _scene(pt, "cornell.txt", (W, H))
    with pt.Tracer(s) as T, pt.Temporal(0, W, H) as h, pt.Moments(0, W, H) as m:
        for (count, first), what in (((1, 0), "ptx_set_guide_samples: iter_first"), ((-1, 1), "ptx_set_guide_samples: count"),
                                     ((4097, 1), "ptx_set_guide_samples: count 4097 exceeds the cap of 4096")):
            with pytest.raises(pt.PathTracerError, match=what):
                T.set_guide_samples(count, first)
        assert T.guide_samples() == (0, 1)
        T.set_guide_samples(4096)                        # the cap itself is accepted (nothing is computed until a denoise or a read)
        T.set_guide_samples(2)
        T.render(1, 2)
        m.add(T, 2)
        with pytest.raises(pt.PathTracerError, match="ptx_denoise_temporal: sampled guides are on"):
            T.denoise_temporal(h, 2)
        with pytest.raises(pt.PathTracerError, match="ptx_denoise_variance: sampled guides are on"):
            T.denoise_variance(2, temporal=h)
        with pytest.raises(pt.PathTracerError, match="ptx_denoise_temporal_measured: sampled guides are on"):
            T.denoise_measured(m, 2, temporal=h)
        T.denoise_variance(2)                            # without a history it runs
        T.set_guide_samples(0)
        T.denoise_temporal(h, 2)                         # ... and the temporal path is as it was
    with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as Tt:
        with pytest.raises(pt.PathTracerError, match="ptx_set_guide_samples: this tracer renders a row tile"):
            Tt.set_guide_samples(2)
        with pytest.raises(pt.PathTracerError, match="row tile"):
            Tt.guide_coverage()


def test_cpp_veneer_guide_samples_is_the_c_abi_frame(gpu_product, tmp_path):
    pt = gpu_product
    exe = tmp_path / "guides_veneer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "guides_veneer_check.cpp"),
                           "-L" + os.path.join(ROOT, "mygpuraytracer_amd"), "-lmi355x_pathtracer", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mygpuraytracer_amd") + ",-rpath,/opt/rocm/lib"])
    W, H, D, N, K = 96, 64, 6, 4, 3
    scene = os.path.join(ROOT, "scenes", "cornellObj.txt")
    out = subprocess.check_output([str(exe), scene, str(W), str(H), str(D), str(N), str(K), str(tmp_path / "v")], text=True)
    assert "guides veneer ok" in out
    rd = lambda ext: np.frombuffer(open(str(tmp_path / "v") + ext, "rb").read(), np.float32).reshape(H, W, 3)
    s = pt.Scene(scene, res=(W, H), depth=D)
    s.apply_runcuda_camera()
    with pt.Tracer(s, antialiasing=1, depth_of_field=1) as T, pt.Moments(0, W, H) as m:
        T.set_guide_samples(K)
        for it in range(1, N + 1):
            T.pathtrace(it)
            m.add(T, it)
        assert beq(rd(".plain"), T.denoise(N))
        assert beq(rd(".measured"), T.denoise_measured(m, N))
        T.set_guide_samples(0)
        assert not beq(rd(".plain"), T.denoise(N))


def test_headless_driver_guide_samples(gpu_product, tmp_path):
    pt = gpu_product
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    W, H = 80, 48
    scene = os.path.join(ROOT, "scenes", "cornellObj.txt")
    r = subprocess.run([exe, scene, "--res", str(W), str(H), "--iterations", "6", "--dof", "--denoise", "--guide-samples", "4", "--pfm",
                        "--out", str(tmp_path / "h")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    pfms = sorted(p for p in os.listdir(tmp_path) if p.endswith(".denoised.pfm"))
    assert len(pfms) == 1 and os.path.exists(tmp_path / pfms[0].replace(".pfm", ".png")), os.listdir(tmp_path)
    pfm = open(tmp_path / pfms[0], "rb").read()
    got = np.frombuffer(pfm[-W * H * 12:], np.float32).reshape(H, W, 3)[::-1]
    s = _scene(pt, "cornellObj.txt", (W, H))
    with pt.Tracer(s, depth_of_field=1) as T:
        T.render(1, 6)
        T.set_guide_samples(4)
        assert beq(got, T.denoise(6))
    r = subprocess.run([exe, scene, "--res", str(W), str(H), "--iterations", "2", "--denoise", "--temporal", "--guide-samples", "2",
                        "--out", str(tmp_path / "t")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--guide-samples does not combine with --temporal" in r.stderr


def guide_quality(pt, O, aa, dof, measured=False, spp=16, truth=1024, res=(128, 128)):
    """MSE against a `truth`-spp frame of the same tracer of the spp-sample frame denoised with K = spp sampled guides and with the
    pixel-centre guides, default parameters: (whole frame, mixed pixels) x (sampled, centre), and the number of mixed pixels -- those
    with 0 < coverage < 1 or more than one geom id among their samples."""
    W, H = res
    s = _scene(pt, "cornell.txt", res)
    d = _oracle(O, s, aa, dof)
    ref = sampled_guides(oracle_samples(O, d, 1, spp, albedo=None))
    mixed = (((ref["coverage"] > 0) & (ref["coverage"] < 1)) | ref["mixed"]).reshape(H, W)
    with pt.Tracer(s, antialiasing=aa, depth_of_field=dof) as T, pt.Moments(0, W, H) as m:
        for it in range(1, spp // 2 + 1):
            T.render(2 * it - 1, 2)
            m.add(T, 2 * it)
        run = (lambda: T.denoise_measured(m, spp)) if measured else (lambda: T.denoise(spp))
        centre = run().astype(np.float64)
        T.set_guide_samples(spp)
        sampled = run().astype(np.float64)
        assert beq(T.guide_coverage().reshape(-1), ref["coverage"])
        T.render(spp + 1, truth - spp)
        gt = (T.read_image() / np.float32(truth)).reshape(H, W, 3).astype(np.float64)
    mse = lambda a, mask: float(((a - gt)[mask] ** 2).mean())
    whole = np.ones((H, W), bool)
    return dict(whole=(mse(sampled, whole), mse(centre, whole)), mixed=(mse(sampled, mixed), mse(centre, mixed)), pixels=int(mixed.sum()))


def test_sampled_guides_lower_the_error_of_a_depth_of_field_frame(gpu_product, O):
    """cornell.txt 128x128, antialiasing and depth of field on, 16 spp, default parameters, against 1024 spp.  Measured on one MI355X:
    whole frame 0.005873 against 0.006142 with the pixel-centre guides (0.956), the 4065 mixed pixels 0.006862 against 0.008679
    (0.791).  DESIGN.md 10 "Sampled guides" has the other cases, two of which (the plain filter with only one of antialiasing and
    depth of field on) come out above 1."""
    q = guide_quality(gpu_product, O, 1, 1)
    print("aa + dof: whole frame MSE sampled %.5g centre %.5g (ratio %.3f); %d mixed pixels: sampled %.5g centre %.5g (ratio %.3f)" %
          (q["whole"] + (q["whole"][0] / q["whole"][1], q["pixels"]) + q["mixed"] + (q["mixed"][0] / q["mixed"][1],)))
    assert q["pixels"] > 0
    assert q["whole"][0] < q["whole"][1], q
    assert q["mixed"][0] < q["mixed"][1], q


def test_headless_driver_guide_samples_on_an_adaptive_frame(gpu_product, tmp_path):
    """mi355x_pathtrace --adaptive E --adaptive-denoise --guide-samples K: the denoised PFM holds Tracer.denoise_adaptive's frame after
    the same Adaptive.render with the guides of iterations 1 .. min(K, the worst tile's count)"""
    import glob
    pt = gpu_product
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    (W, H), E, B, CAP, K = (768, 24), 0.3, 8, 2048, 6
    r = subprocess.run([exe, scene, "--res", str(W), str(H), "--depth", "4", "--iterations", str(CAP), "--dof", "--adaptive", str(E),
                        "--measure-every", str(B), "--adaptive-denoise", "--guide-samples", str(K), "--pfm", "--out", str(tmp_path / "a")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    s = _scene(pt, "cornell.txt", (W, H), depth=4)
    with pt.Tracer(s, depth_of_field=1) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        rounds = a.render(T, m, batch=B, max_iterations=CAP, target=E)
        centre = T.denoise_adaptive(a, m)
        assert rounds[-1]["samples_max"] >= K
        T.set_guide_samples(K)
        want = T.denoise_adaptive(a, m)
        assert not beq(want, centre)
    n = len(rounds) * B
    got = np.frombuffer(open(glob.glob(str(tmp_path / ("a.*.%dsamp.denoised.pfm" % n)))[0], "rb").read()[-W * H * 12:], np.float32)
    assert beq(got.reshape(H, W, 3)[::-1], want)
