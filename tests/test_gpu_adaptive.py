"""GPU: adaptive sampling by tiles (include/mi355x_pathtracer.h: ptx_moments_add_host_tiled, ptx_adaptive_*).  The tiled moments add, the
tile error, the decision, the status and the resolve against their float64 restatement (tests/adaptive_ref.py); the whole loop on a
frame in which most tiles see nothing; the refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, beq
from adaptive_ref import TiledMoments, decide, num_tiles, pixel_rel, resolve, status, tile_error, tile_of
from moments_ref import from_cov6
from test_gpu_active_tiles import WIDE, ODD, _scene, _sees, tile_of_pixel

pytestmark = pytest.mark.gpu

TOL = 1e-4          # tests/test_gpu_moments.py's bound, by its metric |gpu - ref| / (|ref| + 1e-3)
KS = (0, 1, 3, 12, 100)


def _err(gpu, ref):
    ref = np.asarray(ref, np.float64)
    e = np.abs(np.asarray(gpu, np.float64) - ref) / (np.abs(ref) + 1e-3)
    return float(e.max()) if e.size else 0.0


def schedule(h, w, tp, nadds, seed):
    """nadds rows of one k per tile, each drawn from KS"""
    return np.random.default_rng(seed).choice(KS, (nadds, num_tiles(h, w, tp)))


def tiled_frames(h, w, tp, ks_rows, seed, scale=None):
    """fp32 accumulation buffers as a masked tracer leaves them (tests/test_gpu_moments.py's _frames, tile by tile): per pixel a colour in
    [0.05, 1]^3, per sample a relative noise of 0.5 common to the channels plus 0.2 of each channel's own, times the tile's `scale`;
    tile t gains ks[t] samples per add and nothing where that is 0.  [(buffer, samples per tile)]"""
    rng = np.random.default_rng(seed)
    f = np.float32
    tile = tile_of(h, w, tp)
    c = (0.05 + 0.95 * rng.random((h, w, 3))).astype(f)
    sc = np.ones(num_tiles(h, w, tp)) if scale is None else np.asarray(scale, np.float64)
    acc, n, out = np.zeros((h, w, 3), f), np.zeros(num_tiles(h, w, tp), np.int64), []
    for ks in ks_rows:
        k = np.asarray(ks)[tile][..., None].astype(np.float64)
        z = (0.5 * rng.standard_normal((h, w, 1)) + 0.2 * rng.standard_normal((h, w, 3))) * sc[tile][..., None]
        gain = np.where(k > 0, k * c * np.maximum(1 + z / np.sqrt(np.maximum(k, 1)), 0), 0.0).astype(f)
        acc = (acc + gain).astype(f)
        n = n + np.asarray(ks)
        out.append((acc.copy(), n.copy()))
    return out


def _state(m):
    r = m.read()
    return dict(mean=r["mean"], cov=r["cov"], batches=r["batches"], W=m.read_samples())


def straddling_pairs(h, w, tp):
    """the (rb, gb) records whose two pixels lie in different tiles: [(even pixel, its row neighbour)]"""
    tile = tile_of(h, w, tp)
    return [(y, x) for y in range(h) for x in range(0, w - 1, 2) if tile[y, x] != tile[y, x + 1]]


@pytest.mark.parametrize("shape", [(61, 97), (1, 1), (700, 3), (4, 64), (5, 65), (2, 256), (3, 257)])
def test_tiled_add_matches_the_restatement(gpu_product, shape):
    """1 to 6 adds in which every tile draws its own k from {0, 1, 3, 12, 100}: mean and covariance within the bound of
    tests/test_gpu_moments.py, batches and the per-pixel W exact, and the pixels of a tile with k = 0 bit-identical before and after
    -- their half of an (rb, gb) record shared with a pixel of another tile included (97, 65 and 257 wide: pairs straddle tiles)."""
    pt = gpu_product
    h, w = shape
    tp = pt.tile_pixels()
    tile = tile_of(h, w, tp)
    pairs = straddling_pairs(h, w, tp)
    odd_wide = shape in ((61, 97), (5, 65), (3, 257))             # odd widths beyond one tile: some pair straddles two tiles
    assert pairs or not odd_wide
    worst_mean = worst_cov = 0.0
    half_kept = 0
    with pt.Moments(0, w, h) as m:
        assert num_tiles(h, w, tp) == -(-h * w // tp)
        for nadds in range(1, 7):
            for rep in range(2):
                seed = 100000 * h + 100 * w + 10 * nadds + rep
                rows = schedule(h, w, tp, nadds, seed)
                m.reset()
                ref = TiledMoments(h, w, tp)
                before = _state(m)
                assert not any(v.any() for v in before.values())
                for (acc, n), ks in zip(tiled_frames(h, w, tp, rows, seed), rows):
                    m.add_host_tiled(acc, n)
                    ref.add(acc, n)
                    after = _state(m)
                    assert beq(after["W"], ref.W_pixels().astype(np.int32)) and beq(after["batches"], ref.B_pixels().astype(np.int32)), (shape, rows)
                    assert m.read()["samples"] == ref.W.max()
                    em, ec = _err(after["mean"], ref.mean), _err(after["cov"], np.stack([ref.cov()[..., i, j] for i, j in
                                                                                        ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))], -1))
                    worst_mean, worst_cov = max(worst_mean, em), max(worst_cov, ec)
                    assert em <= TOL and ec <= TOL, (shape, rows, em, ec)
                    assert not after["cov"][after["batches"] < 2].any()
                    idle = (np.asarray(ks) == 0)[tile]
                    for key in after:
                        assert beq(after[key][idle], before[key][idle]), (shape, rows, key)
                    for y, x in pairs:                               # one half idle with a covariance to keep, the other advancing
                        for a, b in ((x, x + 1), (x + 1, x)):
                            if idle[y, a] and not idle[y, b] and after["cov"][y, a, 4:].any():
                                half_kept += 1
                    before = after
                if n.any():
                    with pytest.raises(pt.PathTracerError, match="below"):
                        m.add_host_tiled(acc, n - (n > 0))           # a total went down: refused, and nothing moved
                with pytest.raises(pt.PathTracerError, match="ntiles"):
                    m.add_host_tiled(acc, np.append(n, 1))
                assert all(beq(v, after[k]) for k, v in _state(m).items())
    assert half_kept > 0 or not odd_wide
    print("%dx%d: largest error of mean %.3g, of cov6 %.3g; %d shared records kept one half" % (w, h, worst_mean, worst_cov, half_kept))


@pytest.mark.parametrize("shape", [(61, 97), (5, 65)])
def test_tiled_add_with_one_k_is_the_plain_add(gpu_product, shape):
    pt = gpu_product
    h, w = shape
    nt = num_tiles(h, w, pt.tile_pixels())
    rows = [[k] * nt for k in (12, 1, 100, 3, 3)]
    with pt.Moments(0, w, h) as a, pt.Moments(0, w, h) as b:
        for acc, n in tiled_frames(h, w, pt.tile_pixels(), rows, seed=h * w):
            a.add_host_tiled(acc, n)
            b.add_host(acc, int(n[0]))
            sa, sb = _state(a), _state(b)
            assert all(beq(sa[k], sb[k]) for k in sa), n[0]
            assert a.read()["samples"] == b.read()["samples"] and a.summary() == b.summary()
        with pytest.raises(pt.PathTracerError, match="tiled add"):
            a.add_host(acc, int(n[0]) + 1)


def _restated(m, floor, tp):
    """e_T and has-an-estimate per tile, in float64 from the moments state the device holds"""
    r = m.read()
    return tile_error(pixel_rel(r["mean"], from_cov6(r["cov"]), r["batches"], m.read_samples(), floor), tp)


def _target_in_the_widest_gap(e):
    """a target no tile's error is closer to than 1e-3 relative: the middle of the widest relative gap between neighbouring errors"""
    v = np.unique(e[e > 0])
    assert len(v) >= 2
    i = int(np.argmax(v[1:] / v[:-1]))
    target = float(np.float32(np.sqrt(v[i] * v[i + 1])))
    assert (np.abs(e - target) > 1e-3 * target).all(), (target, e)          # no tile is left out
    return target


def test_select_matches_the_restatement(gpu_product):
    """Three rounds on synthetic buffers handed to a 97 x 61 tracer (24 tiles, the last one of 29 pixels), each tile with its own noise
    level: e_T within 1e-5, every tile's decision, the status counts exactly, the same bits from a second run; min_batches and
    max_samples each force their decision; and the tracer renders under the mask the select left."""
    pt = gpu_product
    W, H = ODD
    tp = pt.tile_pixels()
    s = _scene(pt, "cornell.txt", ODD)
    nt = num_tiles(H, W, tp)
    scale = 0.15 + 1.7 * np.random.default_rng(7).random(nt)
    tile = tile_of(H, W, tp).ravel()
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        assert a.num_tiles == T.num_tiles == nt
        samples, batches, active = np.zeros(nt, np.int64), np.zeros(nt, np.int64), np.ones(nt, bool)
        rng = np.random.default_rng(11)
        f = np.float32
        c = (0.05 + 0.95 * rng.random((H, W, 3))).astype(f)
        acc = np.zeros((H, W, 3), f)
        stopped_any = False
        for rnd, k in enumerate((8, 8, 12, 5), 1):
            z = (0.5 * rng.standard_normal((H, W, 1)) + 0.2 * rng.standard_normal((H, W, 3))) * scale[tile].reshape(H, W, 1)
            gain = (k * c * np.maximum(1 + z / np.sqrt(k), 0)).astype(f)
            acc = (acc + np.where(active[tile].reshape(H, W, 1), gain, f(0))).astype(f)
            T.write_image(acc)
            a.add(m, T, k)
            samples += k * active
            batches += active
            assert beq(m.read_samples().ravel(), samples[tile].astype(np.int32)) and beq(m.read()["batches"].ravel(), batches[tile].astype(np.int32))
            e, has = _restated(m, 0.05, tp)
            assert has.all() == (rnd >= 2)
            target = _target_in_the_widest_gap(e) if rnd >= 2 else 0.02
            st = a.select(m, T, target=target, min_batches=2)
            rd = a.read()
            want_active = decide(samples, batches, e, target, 2, 1 << 20)
            print("round %d: target %.6g, %s" % (rnd, target, st))
            assert (np.abs(rd["tile_error"] - e) <= 1e-5 * e).all(), (rd["tile_error"], e)
            assert (rd["tile_active"] == want_active).all()
            want = status(samples, want_active, e, has, H, W, tp, rnd if rnd < 3 else rnd + 1)
            for key, v in want.items():
                assert (abs(st[key] - v) <= 1e-5 * v) if key == "worst_error" else (st[key] == v), (key, st[key], v)
            assert beq(rd["samples"].ravel(), samples[tile].astype(np.int32))
            if rnd == 2:                                             # the same bits from a second run
                st2, rd2 = a.select(m, T, target=target, min_batches=2), a.read()
                assert {**st2, "rounds": 0} == {**st, "rounds": 0} and st2["rounds"] == st["rounds"] + 1
                assert beq(rd2["tile_error"], rd["tile_error"]) and beq(rd2["tile_active"], rd["tile_active"])
                assert 0 < want_active.sum() < nt
            stopped_any |= not want_active.all()
            active = want_active
        assert stopped_any and len(set(samples.tolist())) > 1
        # the resolve: acc / samples of the pixel's tile, in fp32
        a.resolve(T)
        assert beq(a.read()["mean"], resolve(acc, samples, H, W, tp))
        # min_batches and max_samples each force their decision
        st = a.select(m, T, target=target, min_batches=100)
        assert st["tiles_active"] == nt and st["pixels_active"] == W * H and a.read()["tile_active"].all()
        st = a.select(m, T, target=1e-9, min_batches=100, max_samples=int(samples.min()))
        assert st["tiles_active"] == 0 and st["pixels_active"] == 0 and not a.read()["tile_active"].any()
        some = samples < samples.max()
        st = a.select(m, T, target=1e-9, min_batches=2, max_samples=int(samples.max()))
        assert (a.read()["tile_active"] == some).all() and st["tiles_active"] == some.sum()
        # ... and that is the tracer's mask now
        T.reset_image()
        T.render(1, 4)
        img = T.read_image()
        assert not img[~some[tile]].any() and img[some[tile]].any()


def test_resolve_of_a_handle_without_samples_is_black(gpu_product):
    """tiles of 0 samples read 0 whatever the buffer holds, the partial last tile's too"""
    pt = gpu_product
    W, H = ODD
    s = _scene(pt, "cornell.txt", ODD)
    with pt.Tracer(s) as T, pt.Adaptive(0, W, H) as a:
        T.render(1, 2)
        assert T.read_image().any()
        a.resolve(T)
        r = a.read()
        assert not r["mean"].any() and not r["samples"].any() and r["tile_active"].all()


def test_adaptive_render_end_to_end(gpu_product):
    """cornell.txt at 768 x 24, depth 4, batches of 8, target 0.05: the run ends by itself with every tile at its target, the tiles that
    see nothing stop at min_batches x batch samples, and the frame holds fewer pixel-samples than a uniform render that gave every tile
    the worst tile's count.  The squared errors against 4096 iterations are printed, nothing is asserted on them."""
    pt = gpu_product
    W, H = WIDE
    CAP, BATCH, TARGET = 16384, 8, 0.05
    s = _scene(pt, "cornell.txt", WIDE)
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        sees = _sees(pt, s, T)
        p = pt.default_adaptive_params(target=TARGET)
        rounds = a.render(T, m, batch=BATCH, max_iterations=CAP, params=p)
        last = rounds[-1]
        assert last["tiles_active"] == 0, "the cap of %d iterations ended the run: %s" % (CAP, last)
        assert len(rounds) * BATCH < CAP and last["rounds"] == len(rounds)
        r = a.read()
        spt = r["samples"].ravel()[::pt.tile_pixels()]
        assert ((r["tile_error"] <= TARGET) | (spt == p.max_samples)).all()
        assert (spt[~sees] == p.min_batches * BATCH).all() and (spt >= p.min_batches * BATCH).all()
        assert last["samples_total"] == int(r["samples"].sum()) < last["samples_max"] * W * H
        assert [x["tiles_active"] for x in rounds] == sorted((x["tiles_active"] for x in rounds), reverse=True)
        assert beq(r["mean"], resolve(T.read_image(), spt, H, W, pt.tile_pixels()))
        frame = r["mean"].reshape(-1, 3).astype(np.float64)
        uniform = max(1, round(last["samples_total"] / (W * H)))
        T.clear_active_tiles()
        T.reset_image()
        T.render(200001, uniform)
        flat = T.read_image().astype(np.float64) / uniform
        T.reset_image()
        T.render(100001, 4096)
        ref = T.read_image().astype(np.float64) / 4096
    print("%d rounds, %d pixel-samples (%.1f per pixel; worst tile %d, uniform at that count %d): MSE against 4096 iterations: adaptive %.4g, "
          "uniform %d iterations %.4g" % (len(rounds), last["samples_total"], last["samples_total"] / (W * H), last["samples_max"],
                                          last["samples_max"] * W * H, ((frame - ref) ** 2).mean(), uniform, ((flat - ref) ** 2).mean()))


def test_refusals(gpu_product):
    pt = gpu_product
    W, H = 96, 64
    s = _scene(pt, "cornellObj.txt", (W, H))
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a, pt.Temporal(0, W, H) as tm:
        with pt.Adaptive(0, W, H // 2) as other:
            for call in (lambda: other.add(m, T, 1), lambda: other.select(m, T), lambda: other.resolve(T)):
                with pytest.raises(pt.PathTracerError, match="size|no add"):
                    call()
        with pt.Moments(0, W, H // 2) as other:
            with pytest.raises(pt.PathTracerError, match="size"):
                a.add(other, T, 1)
        with pytest.raises(pt.PathTracerError, match="no add"):
            a.select(m, T)
        for bad in (dict(target=0.0), dict(floor=0.0), dict(min_batches=1), dict(max_samples=0)):
            with pytest.raises(pt.PathTracerError, match=list(bad)[0]):
                a.select(m, T, **bad)
        with pytest.raises(pt.PathTracerError, match="k must"):
            a.add(m, T, 0)
        T.render(1, 4)
        a.add(m, T, 4)
        T.render(5, 4)
        a.add(m, T, 4)
        # a tiled moments handle is not for the filter, which assumes one spp and one B for the frame
        with pytest.raises(pt.PathTracerError, match="tiled add"):
            T.denoise_measured(m, 8)
        with pytest.raises(pt.PathTracerError, match="tiled add"):
            T.denoise_measured(m, 8, temporal=tm)
        with pytest.raises(pt.PathTracerError, match="tiled add"):
            m.add(T, 9)
        m.reset()
        with pytest.raises(pt.PathTracerError, match="reset both"):   # the two handles are out of step now
            a.add(m, T, 4)
        a.reset()
        m.add(T, 8)
        assert T.denoise_measured(m, 8).any() and T.denoise_measured(m, 8, temporal=tm).any()
    with pt.Tracer(s, antialiasing=0) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        T.render(1, 2)
        a.add(m, T, 2)
        with pytest.raises(pt.PathTracerError, match="code 5.*cache"):
            a.select(m, T)
        T.render(3, 2)                                               # and the tracer goes on, unmasked
        assert T.read_image().any()


def test_cpp_veneer_loop_matches_the_c_abi_sequence(gpu_product, tmp_path):
    """pathtrace() x 24 with momentsBatch() = 4 and adaptiveTarget() = 0.2, two views: the resolved frame, the per-pixel counts and the
    last status equal those of the same calls through the C ABI"""
    pt = gpu_product
    exe = tmp_path / "adaptive_veneer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "adaptive_veneer_check.cpp"),
                           "-L" + os.path.join(ROOT, "mygpuraytracer_amd"), "-lmi355x_pathtracer", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mygpuraytracer_amd") + ",-rpath,/opt/rocm/lib"])
    (W, H), D, N, K, F, DX, E = WIDE, 4, 24, 4, 2, 5.0, 0.2
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    out = subprocess.check_output([str(exe), scene, str(W), str(H), str(D), str(N), str(K), str(F), "%g" % DX, "%g" % E, str(tmp_path / "v")],
                                  text=True, timeout=300)
    assert "adaptive veneer ok" in out
    rd = lambda f, ext, dt: np.frombuffer(open("%s.f%d%s" % (tmp_path / "v", f, ext), "rb").read(), dt)
    s = pt.Scene(scene, res=(W, H), depth=D)
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))
    stopped = 0
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
                a.resolve(T)
                r = a.read()
            assert beq(rd(f, ".frame", np.float32).reshape(H, W, 3), r["mean"]) and r["mean"].any(), f
            assert beq(rd(f, ".samples", np.int32).reshape(H, W), r["samples"]), f
            got = pt.AdaptiveStatus.from_buffer_copy(rd(f, ".status", np.uint8).tobytes())
            assert {k: getattr(got, k) for k, _ in pt.AdaptiveStatus._fields_} == st, f
            stopped += st["tiles_active"] < st["tiles"]
    assert stopped == F                                              # the mask was at work in both views


def test_headless_adaptive(gpu_product, tmp_path):
    """mi355x_pathtrace --adaptive: one line per round with the counts Adaptive.render reports for the same run, the closing line, the
    frame written; and the combinations it refuses"""
    pt = gpu_product
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    (W, H), E, K, CAP = WIDE, 0.3, 8, 2048
    r = subprocess.run([exe, scene, "--res", str(W), str(H), "--depth", "4", "--iterations", str(CAP), "--adaptive", str(E), "--measure-every", str(K),
                        "--pfm", "--out", str(tmp_path / "a")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    lines = re.findall(r"^round (\d+): (\d+) iterations, (\d+) of (\d+) tiles active, (\d+) pixel-samples so far", r.stdout, re.M)
    s = _scene(pt, "cornell.txt", WIDE)
    with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
        rounds = a.render(T, m, batch=K, max_iterations=CAP, target=E)
    assert rounds[-1]["tiles_active"] == 0 and len(rounds) * K < CAP
    assert [tuple(int(v) for v in x) for x in lines] == [(x["rounds"], x["rounds"] * K, x["tiles_active"], x["tiles"], x["samples_total"]) for x in rounds]
    last = rounds[-1]
    assert re.search(r"^adaptive: every tile at its target after %d iterations: %d pixel-samples, \S+ %% of the %d of a uniform render" % (
        len(rounds) * K, last["samples_total"], last["samples_max"] * W * H), r.stdout, re.M), r.stdout
    n = len(rounds) * K
    assert len(list(tmp_path.glob("a.*.%dsamp.png" % n))) == 1 and len(list(tmp_path.glob("a.*.%dsamp.pfm" % n))) == 1
    for extra in (["--denoise"], ["--until-error", "0.1"], ["--per-call"], ["--checkpoint", str(tmp_path / "c")], ["--frames", "2"]):
        bad = subprocess.run([exe, scene, "--adaptive", "0.1"] + extra, capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and "--adaptive does not combine" in bad.stderr, extra
