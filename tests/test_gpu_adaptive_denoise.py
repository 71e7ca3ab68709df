"""GPU: the variance-guided filter on an adaptively sampled frame (include/mi355x_pathtracer.h: ptx_denoise_adaptive; k_adaptive_prep
of csrc/pt_adaptive.hip).  A frame of one count against ptx_denoise_measured bit for bit; frames of mixed counts against the float64
restatement (tests/adaptive_denoise_ref.py); nothing else moving; the refusals; quality against a long render; the C++ veneer and the
headless driver."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, beq
from adaptive_denoise_ref import denoise_adaptive
from adaptive_ref import TiledMoments, num_tiles, pixel_rel, resolve, tile_error, tile_of
from variance_ref import denoise_buffers_variance

pytestmark = pytest.mark.gpu

TOL = 1e-4          # tests/test_gpu_denoise.py's and tests/test_gpu_moments.py's bound, by their metric |gpu - ref| / (|ref| + 1e-3)
ODD = (97, 61)      # 23 whole tiles and one of 29 pixels; tile boundaries in mid-row, (rb, gb) records that straddle two tiles
WIDE = (768, 24)    # three tiles to a row; cornell.txt leaves tiles at both ends that see nothing


def _err(gpu, ref):
    ref = np.asarray(ref, np.float64)
    e = np.abs(np.asarray(gpu, np.float64) - ref) / (np.abs(ref) + 1e-3)
    return float(e.max()) if e.size else 0.0


def _scene(pt, name, res, depth=4, zoom=None):
    """zoom: the camera's distance from its lookAt (cornell.txt: 10.5 as loaded, the open side of the box at 5.5)"""
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    if zoom is None:
        s.apply_runcuda_camera()
    else:
        o = s.orbit_init()
        s.orbit_events(o, [("right", (zoom - o.zoom) * res[1])])       # the right-button drag: zoom += dy / height
    return s


def _ids(g):
    return np.stack([g["material"], g["geom"]], -1)


def _guides(g):
    return g["albedo"], g["normal"], g["position"], g["hit"]


def next_target(e, active):
    """a target that stops the lower half of the active tiles: the geometric mean of the two errors in the middle of theirs (one active
    tile: below its error, so that it goes on)"""
    v = np.sort(np.asarray(e, np.float64)[np.asarray(active, bool)])
    assert len(v) and (v > 0).all()
    i = len(v) // 2
    return float(np.float32(np.sqrt(v[i - 1] * v[i]) if len(v) > 1 else 0.9 * v[0]))


ROUNDS = (8, 8, 12, 5, 7)


def mixed_state(pt, T, m, a, seed):
    """tests/test_gpu_adaptive.py's synthetic buffers (every tile with a noise level of its own) through T.write_image + a.add, a select
    after each add from the second on that stops about half of the active tiles.  Returns the buffer, the counts per tile and the
    float64 restatement of the moments fed the same buffers."""
    W, H, tp = T.width, T.height, pt.tile_pixels()
    nt = num_tiles(H, W, tp)
    tile = tile_of(H, W, tp)
    rng = np.random.default_rng(seed)
    f = np.float32
    scale = 0.15 + 1.7 * rng.random(nt)
    c = (0.05 + 0.95 * rng.random((H, W, 3))).astype(f)
    acc = np.zeros((H, W, 3), f)
    samples, active = np.zeros(nt, np.int64), np.ones(nt, bool)
    ref = TiledMoments(H, W, tp)
    for rnd, k in enumerate(ROUNDS, 1):
        z = (0.5 * rng.standard_normal((H, W, 1)) + 0.2 * rng.standard_normal((H, W, 3))) * scale[tile][..., None]
        gain = (k * c * np.maximum(1 + z / np.sqrt(k), 0)).astype(f)
        acc = (acc + np.where(active[tile][..., None], gain, f(0))).astype(f)
        T.write_image(acc)
        a.add(m, T, k)
        samples = samples + k * active
        ref.add(acc, samples)
        if rnd >= 2 and rnd < len(ROUNDS):
            e, has = tile_error(pixel_rel(ref.mean, ref.cov(), ref.B_pixels(), ref.W_pixels(), 0.05), tp)
            assert has.all()
            a.select(m, T, target=next_target(e, active), min_batches=2)
            active = a.read()["tile_active"]                          # (the device's decision is the one that counts)
    assert beq(a.read()["samples"], samples[tile].astype(np.int32)) and (ref.W == samples).all()
    return acc, samples, ref


def test_uniform_counts_give_the_measured_filters_bits(gpu_product):
    """cornellObj.txt at 97 x 61, the same 4 batches of 2 iterations on two tracers: one feeds a Moments through add and filters with
    denoise_measured, the other goes through Adaptive.add without a select (every tile stays active) and filters with denoise_adaptive.
    Frame, v0 and filtered variance are equal, demodulating or not; and the handle's frame is the resolve."""
    pt = gpu_product
    W, H = ODD
    tp = pt.tile_pixels()
    sa, sb = _scene(pt, "cornellObj.txt", ODD, 8), _scene(pt, "cornellObj.txt", ODD, 8)
    with pt.Tracer(sa) as A, pt.Tracer(sb) as B, pt.Moments(0, W, H) as ma, pt.Moments(0, W, H) as mb, pt.Adaptive(0, W, H) as a:
        for b in range(4):
            A.render(2 * b + 1, 2)
            B.render(2 * b + 1, 2)
            ma.add(A, 2 * (b + 1))
            a.add(mb, B, 2)
        assert beq(A.read_image(), B.read_image())
        for demod in (1, 0):
            want, wv = A.denoise_measured(ma, 8, demodulate=demod), A.variance()
            got, gv = B.denoise_adaptive(a, mb, demodulate=demod), B.variance()
            assert np.array_equal(got, want) and np.array_equal(gv["input"], wv["input"]) and np.array_equal(gv["output"], wv["output"]), demod
            assert want.any() and wv["input"].any() and not beq(want, A.denoise_variance(8, demodulate=demod))
        assert beq(a.read()["mean"], resolve(B.read_image(), [8] * a.num_tiles, H, W, tp))


@pytest.mark.parametrize("size", [ODD, (257, 3), (64, 4)])
def test_mixed_counts_match_the_restatement(gpu_product, size):
    """Five adds on synthetic buffers handed to a cornell.txt tracer (a real G-buffer), about half of the active tiles stopped after each
    from the second on.  97 x 61: 24 tiles, the last of 29 pixels; 257 x 3: 4 tiles, the last of 3 pixels, every row crossing a tile
    boundary at an odd pixel; 64 x 4: one workgroup, one tile; the camera of these two stands 1 in front of the box, or its walls
    would fill a few pixels of so wide a frame.  Frame, v0 and filtered variance within 1e-4 of the restatement for
    both colour spaces, with min_batches = 4 (tiles below it and at it, where there is more than one tile) and = 6, above every tile's
    (the all-spatial restatement); v0 and the filtered variance exactly 0 on miss pixels; two runs the same bits."""
    pt = gpu_product
    W, H = size
    tp = pt.tile_pixels()
    s = _scene(pt, "cornell.txt", size, zoom=None if size == ODD else 6.0)
    nt = num_tiles(H, W, tp)
    tile = tile_of(H, W, tp)
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        assert a.num_tiles == T.num_tiles == nt
        acc, samples, ref = mixed_state(pt, T, m, a, seed=W * H)
        g = T.gbuffer()
        hit = g["hit"]
        B = ref.B
        print("%dx%d: %d tiles, samples per tile %s, batches %s, %d of %d pixels hit" % (W, H, nt, sorted(set(samples.tolist())),
                                                                                      sorted(set(B.tolist())), hit.sum(), hit.size))
        # the state is a demanding one (one tile has one count: 64 x 4 checks the single-tile frame)
        assert hit.any() and (~hit).any()
        assert B.max() == len(ROUNDS) < 6
        if nt > 1:
            assert len(set(samples.tolist())) >= 3 and (B < 4).any() and (B >= 4).any()
            hb = B[tile][hit]
            assert (hb < 4).any() and (hb >= 4).any()                # ... among the hit pixels too
        want_mean = resolve(acc, samples, H, W, tp)
        worst = 0.0
        for demod in (1, 0):
            for mb in (4, 6):
                got, gv = T.denoise_adaptive(a, m, min_batches=mb, demodulate=demod), T.variance()
                want, want_v, want_v0, fallback = denoise_adaptive(acc, samples, ref.cov(), ref.B_pixels(), *_guides(g), ids=_ids(g),
                                                                   tile_px=tp, min_batches=mb, demodulate=demod)
                assert np.array_equal(fallback, hit & (ref.B_pixels() < mb))
                e = _err(got, want), _err(gv["input"], want_v0), _err(gv["output"], want_v)
                print("%dx%d demodulate %d min_batches %d: denoised %.3g, v0 %.3g, filtered variance %.3g" % ((W, H, demod, mb) + e))
                worst = max(worst, *e)
                assert max(e) <= TOL, (size, demod, mb, e)
                assert not gv["input"][~hit].any() and not gv["output"][~hit].any()
                if mb == 6:                                          # above every tile's B: the spatial estimate on every hit pixel
                    sp, sp_v, sp_v0 = denoise_buffers_variance(want_mean.astype(np.float64), *_guides(g), ids=_ids(g), variance=None,
                                                               demodulate=demod)
                    assert (fallback == hit).all()
                    assert max(_err(got, sp), _err(gv["input"], sp_v0), _err(gv["output"], sp_v)) <= TOL, (size, demod)
                again, av = T.denoise_adaptive(a, m, min_batches=mb, demodulate=demod), T.variance()
                assert beq(again, got) and beq(av["input"], gv["input"]) and beq(av["output"], gv["output"])
                assert beq(a.read()["mean"], want_mean)
        print("%dx%d: largest error %.3g" % (W, H, worst))


def test_one_pixel_frame(gpu_product):
    """1 x 1: one tile of one pixel, the call succeeds and equals the restatement -- with the camera inside the box, where the pixel
    hits a wall, and where the scene file puts it, where the pixel (half a frame off the axis) misses: the colour passes through, the
    variances are 0"""
    pt = gpu_product
    tp = pt.tile_pixels()
    seen = set()
    for zoom in (4.0, None):
        s = _scene(pt, "cornell.txt", (1, 1), zoom=zoom)
        with pt.Tracer(s) as T, pt.Moments(0, 1, 1) as m, pt.Adaptive(0, 1, 1) as a:
            assert a.num_tiles == 1
            ref = TiledMoments(1, 1, tp)
            acc = np.zeros((1, 1, 3), np.float32)
            for i, k in enumerate((4, 4, 8, 2), 1):
                acc = (acc + np.float32(k) * np.float32([0.3 + 0.1 * i, 0.5 - 0.05 * i, 0.2 + 0.02 * i * i])).astype(np.float32)
                T.write_image(acc)
                a.add(m, T, k)
                ref.add(acc, ref.W + k)
            g = T.gbuffer()
            seen.add(bool(g["hit"][0, 0]))
            for demod in (1, 0):
                got, gv = T.denoise_adaptive(a, m, demodulate=demod), T.variance()
                want, want_v, want_v0, _ = denoise_adaptive(acc, ref.W, ref.cov(), ref.B_pixels(), *_guides(g), ids=_ids(g), tile_px=tp,
                                                            demodulate=demod)
                e = _err(got, want), _err(gv["input"], want_v0), _err(gv["output"], want_v)
                print("1x1 hit %d demodulate %d: %s" % (g["hit"][0, 0], demod, e))
                assert max(e) <= TOL, (zoom, demod, e)
                if not g["hit"][0, 0]:
                    assert beq(got, resolve(acc, ref.W, 1, 1, tp)) and not gv["input"].any() and not gv["output"].any()
                else:
                    assert gv["input"][0, 0] > 0
            assert beq(a.read()["mean"], resolve(acc, ref.W, 1, 1, tp))
    print("1x1: hit states seen", seen)
    assert seen == {True, False}


def _state(T, m, a):
    st = T.stats()
    st.pop("loop_ms_total")
    r, ar = m.read(), a.read()
    return dict(image=T.read_image(), stats=st, mean=r["mean"], cov=r["cov"], batches=r["batches"], W=m.read_samples(), total=r["samples"],
                samples=ar["samples"], active=ar["tile_active"], error=ar["tile_error"])


def _same(x, y):
    return all((x[k] == y[k]) if isinstance(x[k], (dict, int)) else beq(x[k], y[k]) for k in x)


def _rounds(T, m, a, first, rounds, k, mode):
    it = first
    for _ in range(rounds):
        if mode == "render":
            T.render(it, k)
        else:
            for j in range(it, it + k):
                T.pathtrace(j)
        it += k
        a.add(m, T, k)
        st = a.select(m, T, target=0.05, min_batches=2)
    return it, st


@pytest.mark.parametrize("mode", ["render", True, False])
def test_nothing_else_moves(gpu_product, mode):
    """cornell.txt at 768 x 24, three rounds of 4 iterations at target 0.05 (the tiles that see nothing stop after the second) on two tracers (ptx_render; ptx_iterate with render-ahead on
    and off); one of them is then filtered, twice.  Its accumulation buffer, statistics, moments state, counts, flags and errors are
    bit-identical before and after, and two further rounds on both leave the same bits in all of them."""
    pt = gpu_product
    W, H = WIDE
    sa, sb = _scene(pt, "cornell.txt", WIDE), _scene(pt, "cornell.txt", WIDE)
    with pt.Tracer(sa) as A, pt.Tracer(sb) as B, pt.Moments(0, W, H) as ma, pt.Moments(0, W, H) as mb, pt.Adaptive(0, W, H) as aa, \
            pt.Adaptive(0, W, H) as ab:
        if mode != "render":
            A.set_render_ahead(mode)
            B.set_render_ahead(mode)
        na, st = _rounds(A, ma, aa, 1, 3, 4, mode)
        nb, _ = _rounds(B, mb, ab, 1, 3, 4, mode)
        assert 0 < st["tiles_active"] < st["tiles"], st              # the mask is at work
        before = _state(A, ma, aa)
        assert _same(before, _state(B, mb, ab))
        out = A.denoise_adaptive(aa, ma)
        assert out.any() and beq(out, A.denoise_adaptive(aa, ma, read=False) or A.read_denoised())
        assert _same(before, _state(A, ma, aa)), mode
        na, sta = _rounds(A, ma, aa, na, 2, 4, mode)
        nb, stb = _rounds(B, mb, ab, nb, 2, 4, mode)
        assert sta == stb and _same(_state(A, ma, aa), _state(B, mb, ab)), mode
        assert len(set(_state(A, ma, aa)["samples"].ravel().tolist())) > 1


def test_refusals(gpu_product):
    pt = gpu_product
    W, H = 96, 64
    s = _scene(pt, "cornellObj.txt", (W, H))
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        with pytest.raises(pt.PathTracerError, match="no add"):      # a fresh pair
            T.denoise_adaptive(a, m)
        with pt.Adaptive(0, W, H // 2) as other:
            with pytest.raises(pt.PathTracerError, match="size"):
                T.denoise_adaptive(other, m)
        with pt.Moments(0, W, H // 2) as other:
            with pytest.raises(pt.PathTracerError, match="size"):
                T.denoise_adaptive(a, other)
        T.render(1, 4)
        a.add(m, T, 4)
        T.render(5, 4)
        a.add(m, T, 4)
        with pytest.raises(pt.PathTracerError, match="min_batches"):
            T.denoise_adaptive(a, m, min_batches=1)
        with pytest.raises(TypeError, match="max_history"):
            T.denoise_adaptive(a, m, max_history=4)
        with pytest.raises(TypeError, match="bogus"):
            T.denoise_adaptive(a, m, bogus=1)
        with pytest.raises(pt.PathTracerError, match="passes"):
            T.denoise_adaptive(a, m, passes=0)
        with pytest.raises(pt.PathTracerError, match="tiled add"):   # the one-count entry point keeps refusing this handle
            T.denoise_measured(m, 8)
        assert T.denoise_adaptive(a, m, min_batches=2).any()
        m.reset()
        with pytest.raises(pt.PathTracerError, match="reset both"):  # the two handles are out of step now
            T.denoise_adaptive(a, m)
        a.reset()
        with pytest.raises(pt.PathTracerError, match="no add"):
            T.denoise_adaptive(a, m)
    with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as Tt, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        with pytest.raises(pt.PathTracerError, match="row tile"):
            Tt.denoise_adaptive(a, m)


@pytest.mark.parametrize("scene", ["cornell.txt", "cornellObj.txt"])
def test_end_to_end_the_measured_variance_beats_the_spatial_estimate(gpu_product, scene):
    """256 x 256, depth 8: Adaptive.render in batches of 16 to target 0.05 (the run ends by itself), then denoise_adaptive; the yardstick
    is the existing spatial-estimate filter (denoise_buffers_variance, variance=None) on the same resolved frame and G-buffer, against
    16384 uniform iterations, over the hit pixels, no margin.  The ratios to the unfiltered frame are printed."""
    pt = gpu_product
    W = H = 256
    CAP = 65536         # (8192 leave cornell.txt with 66 of 256 tiles active, the worst at 0.079)
    s = _scene(pt, scene, (W, H), depth=8)
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        rounds = a.render(T, m, batch=16, max_iterations=CAP, target=0.05)
        last = rounds[-1]
        assert last["tiles_active"] == 0 and len(rounds) * 16 < CAP, "the cap of %d iterations ended the run: %s" % (CAP, last)
        aden = T.denoise_adaptive(a, m).astype(np.float64)
        cur32 = a.read()["mean"]
        g = T.gbuffer()
        hit = g["hit"]
        sden = pt.denoise_buffers_variance(cur32, *_guides(g), ids=_ids(g), variance=None)[0].astype(np.float64)
        cur = cur32.astype(np.float64)
        T.clear_active_tiles()
        T.reset_image()
        T.render(100001, 16384)
        gt = (T.read_image().reshape(H, W, 3) / np.float32(16384)).astype(np.float64)
    mse = lambda x: float(((x - gt)[hit] ** 2).mean())
    print("%s 256x256, %d rounds of 16, %d to %d samples per tile (%.1f per pixel) against 16384: MSE unfiltered %.4g, measured variance "
          "%.4g (x %.3f), spatial estimate %.4g (x %.3f)" % (scene, len(rounds), last["samples_min"], last["samples_max"],
                                                            last["samples_total"] / (W * H), mse(cur), mse(aden), mse(aden) / mse(cur),
                                                            mse(sden), mse(sden) / mse(cur)))
    assert mse(aden) <= mse(sden), (mse(aden), mse(sden))


def test_cpp_veneer_frame_is_the_c_abi_sequences(gpu_product, tmp_path):
    """pathtrace() x 24 with momentsBatch() = 4, adaptiveTarget() = 0.2 and adaptiveDenoise() on, two views: adaptiveDenoisedFrame()
    equals Tracer.denoise_adaptive after the same calls through the C ABI, and the resolved frame comes with it"""
    pt = gpu_product
    exe = tmp_path / "adaptive_denoise_veneer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "adaptive_denoise_veneer_check.cpp"),
                           "-L" + os.path.join(ROOT, "mygpuraytracer_amd"), "-lmi355x_pathtracer", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mygpuraytracer_amd") + ",-rpath,/opt/rocm/lib"])
    (W, H), D, N, K, F, DX, E = WIDE, 4, 24, 4, 2, 5.0, 0.2
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    out = subprocess.check_output([str(exe), scene, str(W), str(H), str(D), str(N), str(K), str(F), "%g" % DX, "%g" % E, str(tmp_path / "v")],
                                  text=True, timeout=300)
    assert "adaptive denoise veneer ok" in out
    rd = lambda f, ext, dt: np.frombuffer(open("%s.f%d%s" % (tmp_path / "v", f, ext), "rb").read(), dt)
    s = pt.Scene(scene, res=(W, H), depth=D)
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))
    with pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        for f in range(1, F + 1):
            if f > 1:
                s.orbit_events(o, [("left", DX, 0.0)])
            m.reset()                                                # pathtraceInit's
            a.reset()
            with pt.Tracer(s) as T:
                T.set_render_ahead(True)
                for it in range(1, N + 1):
                    T.pathtrace(it)
                    if it % K == 0:
                        a.add(m, T, K)
                        st = a.select(m, T, target=E)
                frame = T.denoise_adaptive(a, m)
                r = a.read()
            assert st["tiles_active"] < st["tiles"] and len(set(r["samples"].ravel().tolist())) > 1, f
            assert beq(rd(f, ".denoised", np.float32).reshape(H, W, 3), frame) and frame.any(), f
            assert beq(rd(f, ".frame", np.float32).reshape(H, W, 3), r["mean"]) and not beq(frame, r["mean"]), f


def test_headless_adaptive_denoise(gpu_product, tmp_path):
    """mi355x_pathtrace --adaptive 0.3 --adaptive-denoise --pfm at 768 x 24: the denoised PFM next to the resolved one holds
    Tracer.denoise_adaptive's frame after the same Adaptive.render, with the driver's --denoise-passes and --phi-luminance"""
    pt = gpu_product
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    (W, H), E, K, CAP = WIDE, 0.3, 8, 2048
    r = subprocess.run([exe, scene, "--res", str(W), str(H), "--depth", "4", "--iterations", str(CAP), "--adaptive", str(E), "--measure-every", str(K),
                        "--adaptive-denoise", "--denoise-passes", "3", "--phi-luminance", "2.5", "--pfm", "--out", str(tmp_path / "a")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    s = _scene(pt, "cornell.txt", WIDE)
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        rounds = a.render(T, m, batch=K, max_iterations=CAP, target=E)
        want = T.denoise_adaptive(a, m, passes=3, phi_luminance=2.5)
        mean = a.read()["mean"]
        assert not beq(want, T.denoise_adaptive(a, m))               # the two options reached the filter
    n = len(rounds) * K
    assert rounds[-1]["tiles_active"] == 0 and n < CAP
    pfm = lambda pat: np.frombuffer(open(glob.glob(str(tmp_path / pat))[0], "rb").read()[-W * H * 12:], np.float32).reshape(H, W, 3)[::-1]
    assert beq(pfm("a.*.%dsamp.denoised.pfm" % n), want)             # (a .pfm stores its rows bottom up)
    assert beq(pfm("a.*.%dsamp.pfm" % n), mean)
    assert len(glob.glob(str(tmp_path / ("a.*.%dsamp.denoised.png" % n)))) == 1 and "denoised.pfm" in r.stdout
