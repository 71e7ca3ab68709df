"""GPU: the denoiser's guides followed through mirrors and glass (include/mi355x_pathtracer.h: ptx_set_guide_bounces; DESIGN.md 10
"Guides through mirrors and glass").  k_guides_follow against the numpy restatement (tests/guide_bounces_ref.py) on the CPU oracle, bit
for bit, over the small scenes that module writes; the records of rays that are never followed against the library as it is without
the mode; staleness and refusals; the filter entry points fed by the new guides; and the quality claim the mode exists for, against a
1024-spp frame."""
import os

import numpy as np
import pytest

from conftest import ROOT, beq
from guide_bounces_ref import SCENE_BASE, followed, followed_samples, mesh_mirror, write_scene
from guides_ref import oracle_samples, sampled_guides

pytestmark = pytest.mark.gpu

TOL = 1e-4          # tests/test_gpu_denoise.py's bound, by its metric |gpu - ref| / (|ref| + 1e-3) (tests/test_gpu_guides.py, test_gpu_variance.py)
FIELDS = ("normal", "position", "t", "hit", "material", "geom", "albedo")
RES = (97, 61)
PTX_ERR_INVALID, PTX_ERR_UNSUPPORTED = 1, 5


@pytest.fixture()
def O(oracle_lib):
    oracle_lib.set_libm(1)
    yield oracle_lib
    oracle_lib.set_libm(0)


def _err(gpu, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(gpu, np.float64) - ref) / (np.abs(ref) + 1e-3)).max())


def _ids(g):
    return np.stack([g["material"], g["geom"]], -1)


def _load(pt, tmp_path, name, res=RES, depth=8):
    path, names = write_scene(tmp_path, name, res, depth)
    s = pt.Scene(path, base_dir=SCENE_BASE)
    s.apply_runcuda_camera()
    d = s.dump()
    if name == "e":
        mesh_mirror(d, names)
    return s, d, names


def _tracer(pt, s, d, name, **opt):
    """scene (e)'s mirror on a mesh exists only in the dumped scene: that tracer is made from the arrays"""
    return pt.Tracer.from_pod(d, **opt) if name == "e" else pt.Tracer(s, **opt)


def _oracle(O, d, aa, dof):
    O.create(d, d["textures"])
    O.set_options(aa=aa, dof=dof)
    O.pt_init()


def _read(T):
    g = T.gbuffer()
    g["coverage"] = T.guide_coverage()
    return g


def _same_as_the_restatement(T, ref, what):
    g = _read(T)
    h, w = g["hit"].shape
    for k in FIELDS + ("coverage",):
        want = ref[k].reshape((h, w) + ref[k].shape[1:])
        assert beq(g[k], want.astype(g[k].dtype)), (what, k, int((g[k] != want).sum()))
    return g


# ---- 1. rays that are never followed ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list("abcdefg"))
def test_pixels_whose_rays_are_never_followed_keep_their_record(gpu_product, O, tmp_path, name):
    pt = gpu_product
    s, d, names = _load(pt, tmp_path, name)
    for K in (0, 3):
        with _tracer(pt, s, d, name, antialiasing=1, depth_of_field=1) as T:
            assert T.guide_bounces() == 0
            if K:
                T.set_guide_samples(K)
            g0 = _read(T)                                # never set: the library as it is
            if K:                                        # no sample's first hit is followed (the oracle's camera rays are the tracer's)
                _oracle(O, d, 1, 1)
                keep = np.ones(RES[0] * RES[1], bool)
                for smp in oracle_samples(O, d, 1, K, albedo=None):
                    keep &= ~((smp["t"] > 0) & followed(d, smp["material"], smp["geom"]))
                keep = keep.reshape(RES[1], RES[0])
            else:
                keep = ~(g0["hit"] & followed(d, g0["material"].reshape(-1), g0["geom"].reshape(-1)).reshape(g0["hit"].shape))
            assert keep.sum() > RES[0] * RES[1] // 4
            if name == "g":
                assert keep.all()
            moved = 0
            for B in (1, 8):
                T.set_guide_bounces(B)
                assert T.guide_bounces() == B and T.guide_samples() == (K, 1)
                g = _read(T)
                for k in g0:
                    assert beq(g[k][keep], g0[k][keep]), (name, K, B, k)
                    moved += int(not beq(g[k], g0[k]))
            if name == "g":                              # nothing to follow
                assert moved == 0, (name, K)
            elif name != "d":                            # (d: the continued rays miss, the record stays the mirror's)
                assert moved > 0, (name, K)
            T.set_guide_bounces(0)
            g = _read(T)
            for k in g0:
                assert beq(g[k], g0[k]), (name, K, "back to 0", k)


# ---- 2. the restatement, bit for bit ------------------------------------------------------------------------------------------------
#        scene, frame, depth, (K, iter_first), the values of B
GRID = [("a", RES, 8, (0, 1), (1, 8)), ("b", RES, 8, (0, 1), (1, 8)), ("d", RES, 8, (0, 1), (1, 8)), ("e", RES, 8, (0, 1), (1, 8)),
        ("f", RES, 8, (0, 1), (1, 8)), ("c", RES, 8, (0, 1), (1, 2, 3, 8)),
        ("a", RES, 2, (0, 1), (5,)), ("a", RES, 1, (0, 1), (5,)),
        ("a", RES, 8, (3, 2), (1, 8)), ("b", RES, 8, (3, 2), (1, 8)),
        ("a", (1, 1), 8, (0, 1), (1, 8)), ("a", (3, 130), 8, (0, 1), (1, 8))]


LONGEST = dict(a=1, d=1, e=1, f=1, b=2, c=64)        # continuations the scene has use for: one mirror, into and out of the glass, any number


@pytest.mark.parametrize("name,res,depth,mode,bounces", GRID, ids=["%s-%dx%d-d%d-K%d-B%s" % (n, r[0], r[1], dp, m[0], "_".join(map(str, b)))
                                                                   for n, r, dp, m, b in GRID])
def test_records_are_the_restatement_bit_for_bit(gpu_product, O, tmp_path, name, res, depth, mode, bounces):
    pt = gpu_product
    K, first = mode
    s, d, names = _load(pt, tmp_path, name, res, depth)
    _oracle(O, d, 1 if K else 0, 1 if K else 0)          # the pixel-centre mode: no jitter, no lens, one ray
    with _tracer(pt, s, d, name, antialiasing=1, depth_of_field=1) as T:
        if K:
            T.set_guide_samples(K, first)
        for B in bounces:
            stats = []
            ref = sampled_guides(followed_samples(O, d, first if K else 1, K if K else 1, B, stats=stats))
            for k in ("normal", "position", "t", "albedo"):
                assert np.isfinite(ref[k]).all(), (name, B, k)      # no pixel is left out
            T.set_guide_bounces(B)
            _same_as_the_restatement(T, ref, (name, res, depth, mode, B))
            most = max(int(r["continuations"].max()) for r in stats)
            want = min(B, depth - 1)
            if res != (1, 1):                            # (the one pixel's ray passes the mirror)
                assert most == min(want, LONGEST[name]), (name, B, most)


# ---- 3. staleness and refusals ------------------------------------------------------------------------------------------------------
def test_changing_the_bounces_or_the_camera_recomputes(gpu_product, tmp_path):
    pt = gpu_product
    s, d, names = _load(pt, tmp_path, "a")
    with pt.Tracer(s) as T:
        g0 = _read(T)
        T.set_guide_bounces(8)
        g8 = _read(T)
        assert not beq(g8["position"], g0["position"]) and not beq(g8["geom"], g0["geom"])
        T.set_guide_bounces(8)                           # the same value: the same guides
        for k in g8:
            assert beq(_read(T)[k], g8[k]), k
        o = s.orbit_init()
        s.orbit_events(o, [("left", 30.0, 8.0)])
        T.set_camera(s)
        moved = _read(T)
        assert not beq(moved["position"], g8["position"])
        with pt.Tracer(s) as fresh:
            fresh.set_guide_bounces(8)
            want = _read(fresh)
        for k in want:
            assert beq(moved[k], want[k]), k
        s.set_trace_depth(1)                             # depth 1: no continuation is left, the first surface again
        T.set_camera(s)
        with pt.Tracer(s) as fresh:
            want = _read(fresh)
        got = _read(T)
        for k in want:
            assert beq(got[k], want[k]), k


def test_refusals_and_their_codes(gpu_product, tmp_path):
    pt = gpu_product
    s, d, names = _load(pt, tmp_path, "b", (64, 64))
    L = pt.load_library()
    with pt.Tracer(s) as T, pt.Temporal(0, 64, 64) as h, pt.Moments(0, 64, 64) as m:
        for bad, what in ((-1, b"bounces must be >= 0"), (65, b"bounces 65 exceeds the cap of 64")):
            assert L.ptx_set_guide_bounces(T.h, bad) == PTX_ERR_INVALID and what in L.ptx_last_error()
            with pytest.raises(pt.PathTracerError, match="ptx_set_guide_bounces"):
                T.set_guide_bounces(bad)
        assert L.ptx_set_guide_bounces(None, 1) == PTX_ERR_INVALID and L.ptx_get_guide_bounces(None, None) == PTX_ERR_INVALID
        assert T.guide_bounces() == 0
        T.set_guide_bounces(64)                          # the cap itself is accepted
        T.set_guide_bounces(3)
        T.render(1, 2)
        m.add(T, 2)
        dp, tp, vp = pt.default_denoise_params(), pt.default_temporal_params(), pt.default_variance_params()
        import ctypes as C
        assert L.ptx_denoise_temporal(T.h, h.h, C.byref(dp), C.byref(tp), 2) == PTX_ERR_UNSUPPORTED
        assert L.ptx_denoise_variance(T.h, h.h, C.byref(dp), C.byref(tp), C.byref(vp), 2) == PTX_ERR_UNSUPPORTED
        assert L.ptx_denoise_temporal_measured(T.h, h.h, m.h, C.byref(dp), C.byref(tp), C.byref(vp), 0, 2) == PTX_ERR_UNSUPPORTED
        with pytest.raises(pt.PathTracerError, match="ptx_denoise_temporal: followed guides are on"):
            T.denoise_temporal(h, 2)
        with pytest.raises(pt.PathTracerError, match="ptx_denoise_variance: followed guides are on"):
            T.denoise_variance(2, temporal=h)
        with pytest.raises(pt.PathTracerError, match="ptx_denoise_temporal_measured: followed guides are on"):
            T.denoise_measured(m, 2, temporal=h)
        T.denoise_variance(2)                            # without a history it runs
        T.set_guide_bounces(0)
        T.denoise_temporal(h, 2)                         # ... and the three work again
        T.denoise_variance(2, temporal=h)
        T.denoise_measured(m, 2, temporal=h)
    with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as Tt:
        assert L.ptx_set_guide_bounces(Tt.h, 2) == PTX_ERR_INVALID
        with pytest.raises(pt.PathTracerError, match="ptx_set_guide_bounces: this tracer renders a row tile"):
            Tt.set_guide_bounces(2)


# ---- 4. the filters take the guides as they are; the tracer is left alone -----------------------------------------------------------
def test_the_filters_take_the_followed_guides_and_the_tracer_is_left_alone(gpu_product, tmp_path):
    pt = gpu_product
    (W, H), N = RES, 8
    s, d, names = _load(pt, tmp_path, "b")
    with pt.Tracer(s) as T, pt.Tracer(s) as plain, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a, pt.Moments(0, W, H) as ma:
        T.set_guide_bounces(8)
        for it in range(1, N + 1):
            T.pathtrace(it)
            plain.pathtrace(it)
            if it % 2 == 0:
                m.add(T, it)
            if it == N // 2:
                T.denoise(it)                            # (a filter call between iterations changes nothing that follows)
        assert beq(T.read_image(), plain.read_image())   # the mode never set: the same frame, the same statistics
        assert T.stats()["rays_per_bounce"] == plain.stats()["rays_per_bounce"] and T.stats()["rays_total"] == plain.stats()["rays_total"]
        g, g0 = T.gbuffer(), plain.gbuffer()
        assert not beq(g["albedo"], g0["albedo"])
        guides = (g["albedo"], g["normal"], g["position"], g["hit"])
        rgb = (T.read_image() / np.float32(N)).astype(np.float32).reshape(H, W, 3)
        got = T.denoise(N)
        e = _err(got, pt.denoise_buffers(rgb, *guides))
        print("denoise against ptx_denoise_buffers on the read-back guides: %.3g" % e)
        assert e <= TOL, e
        assert not beq(got, plain.denoise(N))
        got = T.denoise_variance(N)
        want, _ = pt.denoise_buffers_variance(rgb, *guides, ids=_ids(g))
        e = _err(got, want)
        print("denoise_variance against ptx_denoise_variance_buffers on the read-back guides: %.3g" % e)
        assert e <= TOL, e
        got = T.denoise_measured(m, N)
        v0 = T.variance()["input"]
        want, _ = pt.denoise_buffers_variance(rgb, *guides, ids=_ids(g), variance=v0)
        e = _err(got, want)
        print("denoise_measured against ptx_denoise_variance_buffers with its v0: %.3g" % e)
        assert e <= TOL, e
        assert beq(T.read_image(), plain.read_image())
        # an adaptive frame (no buffers form): it runs on the followed guides and differs from the first-surface ones
        T.reset_image()
        a.render(T, ma, batch=4, max_iterations=8, target=0.05)
        followed_frame = T.denoise_adaptive(a, ma)
        T.set_guide_bounces(0)
        assert np.isfinite(followed_frame).all() and not beq(followed_frame, T.denoise_adaptive(a, ma))


def test_headless_driver_guide_bounces_one_frame_and_through_the_veneer(gpu_product, tmp_path):
    """mi355x_pathtrace --denoise --guide-bounces B: the single frame sets the tracer itself, --frames goes through the veneer's
    GPUdenoise with guideBounces() = B; both are Tracer.denoise after set_guide_bounces(B)"""
    import ctypes
    import subprocess
    pt = gpu_product
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    scene = os.path.join(ROOT, "scenes", "cornellGlass.txt")
    W, H, N, F = 80, 48, 4, 2
    common = [exe, scene, "--res", str(W), str(H), "--iterations", str(N), "--denoise", "--guide-bounces", "8", "--pfm"]
    for extra, prefix in (([], "one"), (["--frames", str(F), "--frame-step", "left:4,1"], "fr")):
        r = subprocess.run(common + extra + ["--out", str(tmp_path / prefix)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr

    def pfm(name):
        return np.frombuffer(open(tmp_path / name, "rb").read()[-W * H * 12:], np.float32).reshape(H, W, 3)[::-1]      # rows bottom up

    one = sorted(p for p in os.listdir(tmp_path) if p.startswith("one") and p.endswith(".denoised.pfm"))
    assert len(one) == 1, os.listdir(tmp_path)
    s = pt.Scene(scene, res=(W, H))                        # (the depth is the scene file's, as the driver's)
    s.apply_runcuda_camera()
    with pt.Tracer(s) as T:
        T.render(1, N)
        first_surface = T.denoise(N)
        T.set_guide_bounces(8)
        assert beq(pfm(one[0]), T.denoise(N)) and not beq(pfm(one[0]), first_surface)
    s = pt.Scene(scene, res=(W, H))                        # --frames: the orbit camera from the scene file's own
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))
    for f in range(1, F + 1):
        if f > 1:
            s.orbit_events(o, [("left", 4.0, 1.0)])
        with pt.Tracer(s) as T:
            T.render(1, N)
            first_surface = T.denoise(N)
            T.set_guide_bounces(8)
            got = pfm("fr.f%03d.denoised.pfm" % f)
            assert beq(got, T.denoise(N)), (f, "the first-surface frame" if beq(got, first_surface) else "neither frame")


# ---- 5. quality ---------------------------------------------------------------------------------------------------------------------
def _quality_scene(tmp_path, case):
    """scenes/cornell.txt, scenes/cornellGlass.txt, or "cornell mirror": cornell.txt with its sphere on the scene's own specular
    material 4 (which cornell.txt defines and puts on no object), written next to the test's other scenes"""
    if case != "cornell mirror":
        return os.path.join(ROOT, "scenes", case)
    text = open(os.path.join(ROOT, "scenes", "cornell.txt")).read()
    assert text.count("sphere\nmaterial 1\n") == 1
    path = os.path.join(str(tmp_path), "cornell_mirror.txt")
    with open(path, "w") as f:
        f.write(text.replace("sphere\nmaterial 1\n", "sphere\nmaterial 4\n"))
    return path


def guide_bounces_quality(pt, path, spp=16, truth=1024, res=(128, 128), bounces=8):
    """MSE against a `truth`-spp frame of the same tracer, over the followed pixels (those whose first-surface guide names a material
    the chain follows), of the spp-sample frame filtered with the followed guides and with the first-surface ones, default
    parameters: {filter: (followed, first surface)}, the number of followed pixels, and whether the two frames of each filter are
    the same bits."""
    W, H = res
    s = pt.Scene(path, base_dir=SCENE_BASE, res=res, depth=8)
    s.apply_runcuda_camera()
    d = s.dump()
    out = {}
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m:
        g0 = T.gbuffer()
        mask = g0["hit"] & followed(d, g0["material"].reshape(-1), g0["geom"].reshape(-1)).reshape(H, W)
        for it in range(1, spp // 2 + 1):
            T.render(2 * it - 1, 2)
            m.add(T, 2 * it)
        frames = {}
        for B in (bounces, 0):
            T.set_guide_bounces(B)
            frames["denoise", B] = T.denoise(spp)
            frames["denoise_measured", B] = T.denoise_measured(m, spp)
        noisy = (T.read_image() / np.float32(spp)).reshape(H, W, 3).astype(np.float64)
        T.render(spp + 1, truth - spp)
        gt = (T.read_image() / np.float32(truth)).reshape(H, W, 3).astype(np.float64)
    mse = lambda f: float(((f.astype(np.float64) - gt)[mask] ** 2).mean()) if mask.any() else float("nan")
    for kind in ("denoise", "denoise_measured"):
        out[kind] = (mse(frames[kind, bounces]), mse(frames[kind, 0]))
        out[kind + " same bits"] = beq(frames[kind, bounces], frames[kind, 0])
    out["unfiltered"] = mse(noisy)
    out["pixels"] = int(mask.sum())
    return out


@pytest.mark.parametrize("case", ["cornell.txt", "cornellGlass.txt", "cornell mirror"])
def test_followed_guides_lower_the_error_inside_the_mirror_and_the_glass(gpu_product, tmp_path, case):
    """128 x 128, depth 8, 16 spp, default parameters, against the same tracer continued to 1024 spp, over the followed pixels.
    The prediction, stated before measuring: on the followed pixels denoise_measured with bounces = 8 has less error than with
    bounces = 0 -- inside the silhouette the first-surface guides agree with everything, so only the colour weight holds the filter
    back, while the followed guides carry the edges of the room seen in the sphere.  Only that ratio is asserted; the plain filter's
    is printed.  DESIGN.md 10 "Guides through mirrors and glass" has the table as it came out.
    cornell.txt: its sphere is DIFFUSE (material 1; the scene's one specular material, 4, is on no object), so no pixel is followed,
    the two sets of guides are the same bits and there is no error to compare: the prediction cannot be evaluated there, and the
    case asserts exactly that state instead -- zero followed pixels, bit-identical frames.  "cornell mirror" is that scene with the
    sphere on material 4, the mirror sphere the mode was asked for.
    Measured on one MI355X (222 followed pixels each; bounces 8 / bounces 0): cornellGlass.txt denoise_measured 0.0019247 / 0.0025687
    (0.749), denoise 0.0023764 / 0.0023580 (1.008); cornell mirror denoise_measured 0.032780 / 0.049781 (0.658), denoise 0.030584 /
    0.067655 (0.452); unfiltered 0.031752 and 0.039591."""
    q = guide_bounces_quality(gpu_product, _quality_scene(tmp_path, case))
    for kind in ("denoise", "denoise_measured"):
        print("%s %s: %d followed pixels, MSE followed guides %.5g first surface %.5g (ratio %.3f); unfiltered %.5g" %
              (case, kind, q["pixels"], q[kind][0], q[kind][1], q[kind][0] / q[kind][1] if q["pixels"] else float("nan"), q["unfiltered"]))
    if case == "cornell.txt":
        assert q["pixels"] == 0 and q["denoise same bits"] and q["denoise_measured same bits"], q
        return
    assert q["pixels"] > 200
    assert q["denoise_measured"][0] < q["denoise_measured"][1], q
