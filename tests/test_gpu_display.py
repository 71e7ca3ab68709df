"""GPU: the display transform (ptx_display_*, csrc/pt_display.hip) against its float64 restatement (tests/display_ref.py): block
luminances and the metered exposure, every tone x transfer pair, the quantisers bit for bit from the device's own fp32 z, the
reference setting against ptx_write_pbo, adaptation, the sources a frame can come from, the refusals, and the veneer and the driver."""
import glob
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import display_ref as dr
from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

TOL = 1e-4          # tests/test_gpu_denoise.py's bound, by its metric |gpu - ref| / (|ref| + 1e-3)
BLOCK_TOL = 1e-4    # an fp32 sum of at most 529 non-negative terms in any order is within 528 * 2^-24 = 3.2e-5; three times that
SIZES = ((1, 1), (7, 7), (8, 8), (37, 23), (97, 61))
SAMPLES = 3
_BUFFERS = {}


def _buffer(w, h):
    """The random HDR frame of one size and what the restatement makes of it, computed once: a log-normal luminance over six decades
    (one decade per sigma, cut at three), about 30 % exact zeros, block (0, 0) all zero, and a few NaN, negative, +inf and 1e30 entries"""
    if (w, h) in _BUFFERS:
        return _BUFFERS[(w, h)]
    rng = np.random.default_rng(1000 * w + h)
    lum = 10.0 ** np.clip(rng.normal(0.0, 1.0, (h, w)), -3.0, 3.0)
    rgb = (lum[..., None] * rng.uniform(0.2, 1.8, (h, w, 3))).astype(np.float32)
    rgb[rng.random((h, w)) < 0.3] = 0.0
    rows, cols = dr.block_grid(w, h)
    n = w * h
    flat = rgb.reshape(-1)
    if n >= 64:
        bad = rng.choice(3 * n, 12, replace=False)
        flat[bad[0:3]] = np.nan
        flat[bad[3:6]] = -2.5
        flat[bad[6:9]] = np.inf
        flat[bad[9:12]] = 1e30
    if rows:
        rgb[rows[0]:rows[1], cols[0]:cols[1]] = 0.0
    blocks = dr.block_means(rgb, SAMPLES, w, h)
    # the > 1e-8 decision must not depend on rounding
    assert not ((blocks > 0.5e-8) & (blocks < 2e-8)).any()
    out = dict(rgb=rgb, blocks=blocks, meter=dr.meter(blocks))
    _BUFFERS[(w, h)] = out
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _scene(pt, name, res, depth=4):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s


def _metric(gpu, ref):
    return float((np.abs(np.asarray(gpu, np.float64) - ref) / (np.abs(ref) + 1e-3)).max())


@pytest.mark.parametrize("w,h", SIZES)
def test_block_averages_and_status(gpu_product, w, h):
    pt = gpu_product
    b = _buffer(w, h)
    want = b["meter"]
    with pt.Display(w, h) as D:
        assert D.status() == dict(metered=1.0, applied=1.0, log2_mean=0.0, blocks_used=0, blocks_total=want["blocks_total"], frames=0)
        D.host(b["rgb"], SAMPLES)
        got, st = D.blocks(), D.status()
        D.host(b["rgb"], SAMPLES)                        # the same buffer again: the same bits
        assert beq(got, D.blocks())
        st2 = D.status()
        assert st2.pop("frames") == 2 and st.pop("frames") == 1 and st == st2
        assert all(struct.pack("f", st[k]) == struct.pack("f", st2[k]) for k in ("metered", "applied", "log2_mean"))
    assert got.shape == b["blocks"].shape
    if got.size:
        zero = b["blocks"] == 0
        assert zero[0, 0] and (got[zero] == 0).all()
        assert (~zero).any() or (w, h) == (8, 8)                      # (8 x 8 is its one block, the zero one)
        rel = np.abs(got.astype(np.float64) - b["blocks"])[~zero] / b["blocks"][~zero]
        print("%d x %d: block averages within %.3g relative" % (w, h, rel.max(initial=0.0)))
        assert rel.max(initial=0.0) <= BLOCK_TOL
    assert (st["blocks_used"], st["blocks_total"]) == (want["blocks_used"], want["blocks_total"])
    assert abs(st["metered"] - want["metered"]) <= BLOCK_TOL * want["metered"], (st, want)
    assert st["applied"] == st["metered"]
    if w < 8 or h < 8:
        assert st["metered"] == 1.0 and st["blocks_total"] == 0
    else:
        assert st["blocks_used"] < st["blocks_total"] and abs(st["log2_mean"] - want["log2_mean"]) <= 1e-3


def test_a_black_frame_meters_one(gpu_product):
    with gpu_product.Display(37, 23) as D:
        codes = D.host(np.zeros((23, 37, 3), np.float32))
        st = D.status()
        assert st["metered"] == 1.0 and st["applied"] == 1.0 and st["blocks_used"] == 0 and st["blocks_total"] == 2 and not codes.any()
        assert not D.blocks().any()


@pytest.mark.parametrize("w,h", ((37, 23), (97, 61)))
@pytest.mark.parametrize("transfer", ("linear", "srgb"))
@pytest.mark.parametrize("tone", ("clamp", "reinhard", "aces"))
def test_map_against_the_restatement(gpu_product, tone, transfer, w, h):
    """z of every tone x transfer pair, with the restatement fed the handle's own applied exposure"""
    pt = gpu_product
    b = _buffer(w, h)
    d = _dev(b["rgb"])
    with pt.Display(w, h) as D:
        D.device(d.data_ptr(), SAMPLES, tone=tone, transfer=transfer, exposure=1.5, white=3.0, keep_float=1)
        z, codes = D.read(float_frame=True)
        applied = D.status()["applied"]
    E = float(np.float32(applied) * np.float32(1.5))
    from mygpuraytracer_amd import api
    ref = dr.display(b["rgb"], SAMPLES, E, api._DISPLAY_NAMES["tone"][tone], api._DISPLAY_NAMES["transfer"][transfer], white=3.0)
    m = _metric(z, ref)
    print("%s %s %d x %d: z within %.3g by the denoiser tests' metric (exposure %.6g)" % (tone, transfer, w, h, m, E))
    assert m <= TOL
    assert z.min() == 0.0 and 0.5 < z.max() <= 1.0 + 1e-6                             # the exposure landed the frame inside the range
    assert np.array_equal(codes, dr.quantise(z, w, h, 1, 0))


@pytest.mark.parametrize("w,h", ((37, 23), (97, 61), (8, 8), (1, 1)))
@pytest.mark.parametrize("quantize,dither", ((0, 0), (1, 0), (1, 1)))
def test_codes_are_the_quantiser_of_the_devices_own_z(gpu_product, quantize, dither, w, h):
    import torch
    pt = gpu_product
    b = _buffer(w, h)
    d = _dev(b["rgb"])
    with pt.Display(w, h) as D:
        kw = dict(quantize=quantize, dither=dither)
        D.device(d.data_ptr(), SAMPLES, keep_float=1, **kw)
        z, codes = D.read(float_frame=True)
        assert np.array_equal(codes, dr.quantise(z, w, h, quantize, dither)) and not codes[..., 3].any()
        if w * h > 64:
            assert len(np.unique(codes[..., :3])) > 8
        D.device(d.data_ptr(), SAMPLES, **kw)                        # without the float frame
        assert np.array_equal(D.read(), codes)
        with pytest.raises(pt.PathTracerError, match="keep_float"):
            D.read(float_frame=True)
        pbo = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda:0")
        D.device(d.data_ptr(), SAMPLES, pbo=pbo.data_ptr(), keep_float=1, **kw)      # into a caller's buffer
        assert beq(D.read_float(), z)
        torch.cuda.synchronize()
        assert np.array_equal(pbo.cpu().numpy(), codes)
        with pytest.raises(pt.PathTracerError, match="caller's buffer"):
            D.read()
    if quantize and w * h > 64:
        other = dr.quantise(z, w, h, 1, 1 - dither)
        assert not np.array_equal(other, codes)                      # the dither is not a no-op


@pytest.mark.parametrize("w,h", ((37, 23), (97, 61)))
def test_unaligned_pointers_take_the_per_pixel_form_with_the_same_codes(gpu_product, w, h):
    import torch
    pt = gpu_product
    b = _buffer(w, h)
    n = w * h
    d = _dev(b["rgb"])
    shifted = torch.zeros(3 * n + 8, dtype=torch.float32, device="cuda:0")
    shifted[1:1 + 3 * n] = d.reshape(-1)
    assert d.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 0
    with pt.Display(w, h) as D:
        for kw in (dict(), dict(keep_float=1, dither=1, tone="reinhard")):
            D.device(d.data_ptr(), SAMPLES, **kw)
            codes = D.read()
            z = D.read_float() if kw else None
            D.device(shifted.data_ptr() + 4, SAMPLES, **kw)          # the frame 4 bytes off the 16-byte grid
            assert np.array_equal(D.read(), codes)
            assert z is None or beq(D.read_float(), z)
            pbo = torch.full((4 * n + 16,), 7, dtype=torch.uint8, device="cuda:0")
            D.device(d.data_ptr(), SAMPLES, pbo=pbo.data_ptr() + 4, **kw)            # the caller's codes off it
            torch.cuda.synchronize()
            host = pbo.cpu().numpy()
            assert np.array_equal(host[4:4 + 4 * n].reshape(h, w, 4), codes) and (host[:4] == 7).all() and (host[4 + 4 * n:] == 7).all()


REFERENCE_SETTING = dict(meter="manual", exposure=1.0, tone="clamp", transfer="linear", quantize=0)


def test_the_reference_setting_is_ptx_write_pbo(gpu_product):
    pt = gpu_product
    W, H = 37, 23
    s = _scene(pt, "cornell.txt", (W, H))
    with pt.Tracer(s) as T, pt.Display(W, H) as D:
        T.render(1, 2)
        want = T.pbo(2)
        D.tracer(T, 2, **REFERENCE_SETTING)
        assert np.array_equal(D.read().reshape(-1, 4), np.asarray(want).reshape(-1, 4)) and np.asarray(want).any()
        assert D.status()["frames"] == 0                              # manual: nothing was metered
        with pytest.raises(pt.PathTracerError, match="no metered frame"):
            D.blocks()
        rng = np.random.default_rng(5)
        rgb = rng.uniform(-0.5, 1.5, (H, W, 3)).astype(np.float32)   # finite, below 0 and above 1
        rgb[0, :8] = np.array([0.0, 1.0, 0.5, 1.0 / 255, 254.5 / 255, 2.0 / 255, 1e-9, 0.999999], np.float32)[:, None]
        assert np.array_equal(D.host(rgb, **REFERENCE_SETTING).reshape(-1, 4), T.denoised_pbo(rgb))
        assert np.array_equal(D.host(rgb * np.float32(7), 7, **REFERENCE_SETTING), dr.reference_setting_codes(rgb * np.float32(7), 7, W, H))


def test_adaptation_follows_the_recurrence_and_reset_jumps(gpu_product):
    pt = gpu_product
    w, h = 97, 61
    rgb = np.nan_to_num(_buffer(w, h)["rgb"], nan=0.0, posinf=50.0).clip(0.0, 50.0)     # (so that scaling the buffer scales its luminances)
    with pt.Display(w, h) as D:
        seen = []
        for scale in (1.0, 8.0, 0.125):
            D.host(rgb * np.float32(scale), adapt=0.5)
            seen.append(D.status())
        assert [s["frames"] for s in seen] == [1, 2, 3]
        assert seen[0]["applied"] == seen[0]["metered"]
        for k in (1, 2):
            assert abs(seen[k]["metered"] / seen[0]["metered"] - (0.125, 8.0)[k - 1]) < 1e-3
            want = dr.adapt(seen[k - 1]["applied"], seen[k]["metered"], 0.5)
            assert abs(seen[k]["applied"] - want) <= 1e-6 * want, (k, seen, want)
            assert abs(seen[k]["applied"] - seen[k]["metered"]) > 0.1 * seen[k]["metered"]
        D.host(rgb, meter="manual", exposure=2.0)                     # a manual frame in between leaves the state alone
        assert D.status() == seen[2]
        D.reset()
        assert D.status()["frames"] == 0 and D.status()["applied"] == 1.0
        D.host(rgb * np.float32(8), adapt=0.5)
        st = D.status()
        assert st["frames"] == 1 and st["applied"] == st["metered"] == seen[1]["metered"]
        D.host(rgb, adapt=1.0)                                        # no inertia: applied is the metered exposure itself
        st = D.status()
        assert st["frames"] == 2 and st["applied"] == st["metered"] == seen[0]["metered"]


def test_sources(gpu_product):
    """the denoised frame, the adaptive resolved frame and a multi-device tracer's assembled frame give the host path's codes"""
    pt = gpu_product
    W, H = 37, 23
    s = _scene(pt, "cornell.txt", (W, H))
    with pt.Display(W, H) as D, pt.Display(W, H) as Dh:
        with pt.Tracer(s) as T:
            T.render(1, 4)
            with pytest.raises(pt.PathTracerError, match="no ptx_denoise"):
                D.tracer(T, 4, source="denoised")
            den = T.denoise(4)
            D.tracer(T, 4, source="denoised", dither=1)
            assert np.array_equal(D.read(), Dh.host(den, dither=1)) and D.read().any()
            assert D.status() == Dh.status()
            D.tracer(T, 4)                                            # the accumulation buffer over its samples
            assert np.array_equal(D.read(), Dh.host(T.read_image(), 4))
        with pt.Tracer(s) as T, pt.Moments(0, W, H) as m, pt.Adaptive(0, W, H) as a:
            a.render(T, m, batch=4, max_iterations=8, target=0.5)
            D.device(a.device_frame_ptr(), 1, T.stream_ptr())
            mean = a.read()["mean"]
            assert np.array_equal(D.read(), Dh.host(mean)) and mean.any()
        with pt.MultiTracer(s, [0, 0, 0]) as M:
            M.render(1, 2)
            M.assemble()
            D.device(M.device_image_ptr(), 2)
            img = M.read_image()
            assert np.array_equal(D.read(), Dh.host(img, 2)) and img.any()


def test_refusals(gpu_product):
    pt = gpu_product
    W, H = 37, 23
    s = _scene(pt, "cornell.txt", (W, H))
    with pt.Display(W, H) as D, pt.Display(W + 1, H) as other:
        with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as T:
            T.render(1, 1)
            with pytest.raises(pt.PathTracerError, match="row tile"):
                D.tracer(T, 1)
        with pt.Tracer(s) as T:
            T.render(1, 1)
            with pytest.raises(pt.PathTracerError, match="size 38 x 23 differs"):
                other.tracer(T, 1)
            with pytest.raises(pt.PathTracerError, match="spp"):
                D.tracer(T, 0)
            with pytest.raises(pt.PathTracerError, match="source"):
                D.tracer(T, 1, source=5)
            with pytest.raises(pt.PathTracerError, match="no display call"):
                D.read()
        with pytest.raises(ValueError):
            other.host(np.zeros((H, W, 3), np.float32))
        d = _dev(np.zeros((H, W, 3), np.float32))
        nan = float("nan")
        for bad, what in ((dict(meter=2), "meter"), (dict(tone=3), "tone"), (dict(transfer=-1), "transfer"), (dict(quantize=2), "quantize"),
                          (dict(dither=2), "dither"), (dict(keep_float=2), "keep_float"), (dict(adapt=0.0), "adapt"), (dict(adapt=1.01), "adapt"),
                          (dict(adapt=nan), "adapt"), (dict(key=0.0), "key"), (dict(white=-1.0), "white"), (dict(exposure=0.0), "exposure"),
                          (dict(exposure=float("inf")), "exposure")):
            with pytest.raises(pt.PathTracerError, match=what):
                D.device(d.data_ptr(), 1, **bad)
            with pytest.raises(pt.PathTracerError, match=what):
                D.host(np.zeros((H, W, 3), np.float32), **bad)
        for samples in (0, -1, nan):
            with pytest.raises(pt.PathTracerError, match="samples"):
                D.device(d.data_ptr(), samples)
        with pytest.raises(pt.PathTracerError, match="null"):
            D.device(0, 1)
        assert D.status()["frames"] == 0                              # nothing of all that was enqueued


def test_the_tracer_is_untouched(gpu_product):
    """frames, statistics and later iterations of a tracer that serves display calls are those of one that never saw them, through
    ptx_render and through ptx_iterate with render-ahead on and off"""
    pt = gpu_product
    W, H = 80, 45
    for mode in ("render", True, False):
        sa, sb = _scene(pt, "cornellObj.txt", (W, H), depth=8), _scene(pt, "cornellObj.txt", (W, H), depth=8)
        with pt.Display(W, H) as D, pt.Tracer(sa) as A, pt.Tracer(sb) as B:
            if mode != "render":
                A.set_render_ahead(mode)
                B.set_render_ahead(mode)
            n = 0
            for count in (2, 3):
                for T in (A, B):
                    if mode == "render":
                        T.render(n + 1, count)
                    else:
                        for it in range(n + 1, n + count + 1):
                            T.pathtrace(it)
                n += count
                D.tracer(A, n, keep_float=1, adapt=0.5)
                D.tracer(A, n, **REFERENCE_SETTING)
                assert np.array_equal(D.read().reshape(-1, 4), np.asarray(B.pbo(n)).reshape(-1, 4)), (mode, n)
                assert beq(A.read_image(), B.read_image()), (mode, n)
                assert A.stats()["rays_per_bounce"] == B.stats()["rays_per_bounce"], (mode, n)
            for T in (A, B):
                T.pathtrace(n + 1) if mode != "render" else T.render(n + 1, 1)
            D.tracer(A, n + 1)
            assert beq(A.read_image(), B.read_image()) and A.stats()["rays_per_bounce"] == B.stats()["rays_per_bounce"], mode


def test_cpp_veneer_preview_off_is_the_parents_and_on_is_the_display_stage(gpu_product, tmp_path):
    pt = gpu_product
    exe = tmp_path / "display_veneer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "display_veneer_check.cpp"),
                           "-L" + os.path.join(ROOT, "mygpuraytracer_amd"), "-lmi355x_pathtracer", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mygpuraytracer_amd") + ",-rpath,/opt/rocm/lib"])
    (W, H), D_, N = (64, 36), 4, 3
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    out = subprocess.check_output([str(exe), scene, str(W), str(H), str(D_), str(N), str(tmp_path / "v")], text=True, timeout=300)
    assert "display veneer ok" in out
    rd = lambda name: np.frombuffer(open("%s.%s" % (tmp_path / "v", name), "rb").read(), np.uint8).reshape(H, W, 4)
    s = _scene(pt, "cornell.txt", (W, H), depth=D_)
    with pt.Tracer(s) as T, pt.Display(W, H) as D:
        T.set_render_ahead(True)
        for it in range(1, N + 1):
            T.pathtrace(it)
        assert np.array_equal(rd("off.preview").reshape(-1, 4), np.asarray(T.pbo(N)).reshape(-1, 4))       # the parent's bytes
        den = T.denoise(N)
        assert np.array_equal(rd("off.denoised").reshape(-1, 4), T.denoised_pbo(den))
        T.pathtrace(N + 1)
        T.pathtrace(N + 2)
        D.tracer(T, N + 2)
        on = D.read()
        assert np.array_equal(rd("on.preview"), on) and not np.array_equal(on, np.asarray(T.pbo(N + 2)).reshape(H, W, 4))
        T.denoise(N + 2)
        D.tracer(T, 1, source="denoised")
        assert np.array_equal(rd("on.denoised"), D.read()) and np.array_equal(rd("on.host"), D.read())
        assert not np.array_equal(rd("on.denoised"), on)


def _png_rgb8(path):
    """an 8-bit RGB, non-interlaced PNG -> (h, w, 3) uint8 (zlib + the five row filters)"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr = 8, b"", None
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        if typ == b"IDAT":
            idat += body
        pos += 12 + n
    w, h = ihdr[:2]
    assert ihdr[2:] == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w * 3 + 1)
    dec = np.zeros((h, w * 3), np.int64)
    for y in range(h):
        f, line = rows[y, 0], rows[y, 1:].astype(np.int64)
        for i in range(w * 3):
            a = dec[y, i - 3] if i >= 3 else 0
            b = dec[y - 1, i] if y else 0
            c = dec[y - 1, i - 3] if (y and i >= 3) else 0
            if f == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            else:
                pred = (0, a, b, (a + b) >> 1)[f]
            dec[y, i] = (line[i] + pred) & 255
    return dec.astype(np.uint8).reshape(h, w, 3)


def test_headless_driver_display_flags(gpu_product, tmp_path):
    """--tonemap aces --exposure auto --srgb at 64 x 36: the PNG holds the x-mirrored codes of Display.tracer on the same render, the
    denoised PNG those of the denoised frame, and one line per file reports the exposure; without the flags the PNG is what it was"""
    pt = gpu_product
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    W, H, N = 64, 36, 4
    common = [exe, scene, "--res", str(W), str(H), "--depth", "4", "--iterations", str(N), "--denoise"]
    r = subprocess.run(common + ["--tonemap", "aces", "--exposure", "auto", "--srgb", "--out", str(tmp_path / "d")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("display ")]
    assert len(lines) == 2 and all("metered exposure" in l and "applied" in l for l in lines), r.stdout
    p = subprocess.run(common + ["--out", str(tmp_path / "p")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "display " not in p.stdout, p.stderr
    one = lambda pat: _png_rgb8(glob.glob(str(tmp_path / pat))[0])
    s = _scene(pt, "cornell.txt", (W, H))
    with pt.Tracer(s) as T, pt.Display(W, H) as D:
        T.render(1, N)
        D.tracer(T, N, tone="aces", transfer="srgb")
        assert np.array_equal(one("d.*.%dsamp.png" % N), D.read()[:, ::-1, :3])
        assert ("%.6g" % D.status()["metered"]) in lines[0]
        den = T.denoise(N)
        D.reset()
        D.tracer(T, N, source="denoised", tone="aces", transfer="srgb")
        assert np.array_equal(one("d.*.%dsamp.denoised.png" % N), D.read()[:, ::-1, :3])
        # without the flags: saveImage's rule on the same frames, as before
        old = lambda frame, div: (np.clip(frame.reshape(H, W, 3) / np.float32(div), 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)[:, ::-1]
        assert np.array_equal(one("p.*.%dsamp.png" % N), old(T.read_image(), N))
        assert np.array_equal(one("p.*.%dsamp.denoised.png" % N), old(den, 1))
        assert not np.array_equal(one("p.*.%dsamp.png" % N), one("d.*.%dsamp.png" % N))
