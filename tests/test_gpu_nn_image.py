"""GPU: the network denoiser on described images (csrc/pt_nn_image.hip, ptx_nn_denoise_images_*) and through the OIDN veneer
(csrc/oidn_api.h) on synthetic weights.  Every claim is a bit-for-bit equality with an entry point that other tests pin -- NN.host
(ptx_nn_denoise_host: tests/test_gpu_nn.py, _channels, _tiles), NNPrefilter.host (tests/test_gpu_nn_prefilter.py) -- or with the numpy
restatement of the descriptor (tests/nn_image_ref.py): the same pixels through another layout give the same bits, a half image is the
widened / rounded float image, and no byte outside a pixel's three channels changes.  No image-quality claim."""
import os
import subprocess

import numpy as np
import pytest

import nn_image_ref as R
import unet_aux_ref as X
import unet_ref as U
from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

FRAMES = [(38, 22), (33, 17), (1, 1)]
SPECIAL = [np.nan, np.inf, -np.inf, 0.0, -0.0, 70000.0, 1e9, 3.0, -3.0, 1.0, 65504.0, 65520.0]
LAYOUTS = ["packed", "x4", "pitch", "offset"]
_BLOBS = {}


def _blob(ic, table="standard", seed=1):
    key = (ic, table, seed)
    if key not in _BLOBS:
        _BLOBS[key] = U.weights_blob(U.synthetic_weights(ic, seed, channels=U.table(ic, *U.NARROW) if table == "narrow" else None))
    return _BLOBS[key]


def _gauss(w, h, seed, k=1.0, dtype=np.float32):
    """(H, W, 3) of N(0, 1) * k with NaN, +-inf, +-0 and values above 65504 among them (as many as the frame holds), in `dtype`"""
    v = (np.random.default_rng(seed).standard_normal((h, w, 3)) * k).astype(np.float32)
    flat = v.reshape(-1)
    n = min(len(SPECIAL), flat.size)
    flat[(np.arange(n) * 7) % flat.size if flat.size > 7 * n else np.arange(n)] = np.asarray(SPECIAL[:n], np.float32)
    with np.errstate(over="ignore"):
        return v.astype(dtype)


def _half(a):
    """float32 values as float16 (above 65504: inf)"""
    with np.errstate(over="ignore"):
        return a.astype(np.float16)


def _layout(pixels, layout, sentinel=-7.0):
    """(buffer, view): `pixels` (H, W, 3) placed in a buffer of its dtype filled with `sentinel`; view is the (H, W, 3) view of them.
    x4: four channels per pixel; pitch: rows of W + 5 pixels; offset: a row, two pixels and one channel in, four channels, pitched."""
    h, w = pixels.shape[:2]
    shape, at = {"packed": ((h, w, 3), np.s_[:, :, :]), "x4": ((h, w, 4), np.s_[:, :, :3]), "pitch": ((h, w + 5, 3), np.s_[:, :w, :]),
                 "offset": ((h + 1, w + 5, 4), np.s_[1:, 2:2 + w, 1:4])}[layout]
    buf = np.full(shape, sentinel, pixels.dtype)
    view = buf[at]
    view[...] = pixels
    return buf, view


def _expect(pixels, layout, dtype, sentinel=-7.0):
    """the whole buffer an output view of this layout must be afterwards: `pixels` (float32) where the channels are, the sentinel elsewhere"""
    return _layout(pixels if dtype == np.float32 else R.to_half(pixels), layout, sentinel)[0]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


MODES = [dict(), dict(srgb=1), dict(hdr=1, input_scale=0.25), dict(hdr=1)]


def _inputs(w, h, ic, seed, dtype=np.float32):
    rgb = _gauss(w, h, seed, 2.0, dtype)
    alb = _gauss(w, h, seed + 1, 1.0, dtype) if ic >= 6 else None
    nrm = _gauss(w, h, seed + 2, 1.0, dtype) if ic >= 9 else None
    return rgb, alb, nrm


# ---- 1: packed Float3 descriptors are the packed entry point ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ic", [3, 6, 9])
@pytest.mark.parametrize("w,h", FRAMES)
def test_packed_float_images_give_the_packed_calls_bits(gpu_product, w, h, ic):
    pt = gpu_product
    rgb, alb, nrm = _inputs(w, h, ic, 10 * ic + w)
    with pt.NN(w, h, _blob(ic)) as nn:
        for mode in MODES:
            for samples in (1, 3):
                want = nn.host(rgb, alb, nrm, samples=samples, **mode)
                scale = nn.scale()
                out = np.full((h, w, 3), -7.0, np.float32)
                nn.images_host(rgb, out, albedo=alb, normal=nrm, samples=samples, **mode)
                assert beq(out, want), (mode, samples, int((out.view(np.uint32) != want.view(np.uint32)).sum()))
                assert nn.scale().tobytes() == scale.tobytes(), (mode, nn.scale(), scale)
        assert w == 1 or (want.std() > 0 and scale not in (0.25, 1.0))                       # the last mode's scale was metered
        with pytest.raises(pt.PathTracerError, match="albedo " + ("is required" if ic >= 6 else "must be NULL")):
            nn.images_host(rgb, out, albedo=None if ic >= 6 else rgb, normal=nrm)
        if ic > 3:
            with pytest.raises(pt.PathTracerError, match="the albedo role is refused on weights that take %d input channels" % ic):
                nn.images_host(rgb, out, albedo=alb, normal=nrm, role="albedo")
        with pytest.raises(pt.PathTracerError, match="the output image: a row stride of"):
            nn.images_host(rgb, pt.nn_image_of(out.ctypes.data, format=1, row_stride=12 * w - 4), albedo=alb, normal=nrm)


# ---- 2: other layouts of the same pixels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS[1:])
@pytest.mark.parametrize("w,h", FRAMES)
def test_other_layouts_give_the_packed_bits_and_touch_nothing_else(gpu_product, w, h, layout):
    """colour + albedo through a float4 view with a sentinel alpha, a row pitch of W + 5 pixels, a non-zero offset; the output as such
    a view; the whole output buffer compared.  hdr with the automatic scale takes the gather for the meter."""
    pt = gpu_product
    rgb, alb, _ = _inputs(w, h, 6, 77 + w)
    with pt.NN(w, h, _blob(6)) as nn:
        for mode in MODES:
            want = nn.host(rgb, alb, **mode)
            scale = nn.scale()
            for in_layout, out_layout in ((layout, "packed"), ("packed", layout), (layout, layout)):
                cbuf, cview = _layout(rgb, in_layout, 5e4)
                abuf, aview = _layout(alb, in_layout, np.nan)
                obuf, oview = _layout(np.zeros_like(rgb), out_layout)
                before = cbuf.copy(), abuf.copy()
                nn.images_host(cview, oview, albedo=aview, **mode)
                assert _same(obuf, _expect(want, out_layout, np.float32)), (mode, in_layout, out_layout)
                assert nn.scale().tobytes() == scale.tobytes(), (mode, in_layout)
                assert _same(cbuf, before[0]) and _same(abuf, before[1])


# ---- 3: halves ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["packed", "x4", "offset"])
@pytest.mark.parametrize("w,h", FRAMES)
def test_half_images_are_the_widened_and_rounded_float_images(gpu_product, w, h, layout):
    pt = gpu_product
    rgb, alb, nrm = _inputs(w, h, 9, 300 + w, np.float16)
    wide = [a.astype(np.float32) for a in (rgb, alb, nrm)]
    with pt.NN(w, h, _blob(9)) as nn:
        for mode in MODES + [dict(hdr=1, input_scale=1e-6)]:
            want = nn.host(*wide, **mode)
            scale = nn.scale()
            views = [_layout(a, layout, 9.0)[1] for a in (rgb, alb, nrm)]
            out = np.full((h, w, 3), -7.0, np.float32)
            nn.images_host(views[0], out, albedo=views[1], normal=views[2], **mode)                # half in, float out
            assert beq(out, want) and nn.scale().tobytes() == scale.tobytes(), mode
            hbuf, hview = _layout(np.zeros((h, w, 3), np.float16), layout)
            nn.images_host(views[0], hview, albedo=views[1], normal=views[2], **mode)              # half in, half out
            assert _same(hbuf, _expect(want, layout, np.float16)), mode
            hbuf2, hview2 = _layout(np.zeros((h, w, 3), np.float16), layout)
            nn.images_host(wide[0], hview2, albedo=wide[1], normal=wide[2], **mode)                # float in, half out
            assert _same(hbuf2, hbuf), mode
        # the last mode's result does pass 65504: the clamp was exercised, and no infinity was written
        assert (want > 65504).any() and np.isfinite(want[want <= 65504]).all() and not np.isinf(hbuf.astype(np.float32)[hbuf != -7]).any()
        assert (hbuf == np.float16(65504)).any()
        with pytest.raises(pt.PathTracerError, match="mixed input formats: the albedo image"):
            nn.images_host(views[0], out, albedo=wide[1], normal=views[2])


@pytest.mark.parametrize("w,h", FRAMES)
def test_half_subnormals_survive_in_and_out(gpu_product, w, h):
    """a pass-through network without a curve (srgb = 1) hands fp16 values in [0, 1] through exactly: what went in as a half comes out
    as that half, the subnormals among them"""
    pt = gpu_product
    rng = np.random.default_rng(w)
    x = (rng.integers(0, 1024, (h, w, 3)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float16)      # 0 .. 1023 ulps: all subnormal
    x.reshape(-1)[1::2] = rng.random(x.size // 2).astype(np.float16)
    tiny = (x != 0) & (np.abs(x) < np.float16(2.0 ** -14))
    assert tiny.any()
    blob = U.weights_blob(X.passthrough_weights(3, (0, 1, 2), 1.0))
    with pt.NN(w, h, blob) as nn:
        buf, view = _layout(np.zeros((h, w, 3), np.float16), "x4")
        nn.images_host(_layout(x, "x4")[1], view, srgb=1)
        assert _same(buf, _layout(x, "x4")[0])
        out = np.zeros((h, w, 3), np.float32)
        nn.images_host(x, out, srgb=1)
        assert beq(out, x.astype(np.float32)) and beq(out, nn.host(x.astype(np.float32), srgb=1))


# ---- 4: roles ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", FRAMES)
def test_roles_are_the_prefilters_networks(gpu_product, w, h):
    pt = gpu_product
    blob = _blob(3, seed=4)
    a = _gauss(w, h, 50 + w, 0.8)
    n = _gauss(w, h, 60 + w, 0.7)
    with pt.NNPrefilter(w, h, albedo_tza=blob, normal_tza=blob) as pf, pt.NN(w, h, blob) as nn:
        cases = [("albedo", a, dict(srgb=0)), ("albedo", a, dict(srgb=1)), ("albedo", a, dict(srgb=0, input_scale=0.5)), ("normal", n, dict()),
                 ("normal", n, dict(input_scale=2.0))]
        for role, img, params in cases:
            clean_a, clean_n = pf.host(albedo=a, normal=n, **params)
            want = clean_a if role == "albedo" else clean_n
            out = np.full((h, w, 3), -7.0, np.float32)
            nn.images_host(img, out, role=role, **params)
            assert beq(out, want), (role, params, int((out.view(np.uint32) != want.view(np.uint32)).sum()))
            for layout in LAYOUTS[1:]:
                obuf, oview = _layout(np.zeros_like(img), layout)
                nn.images_host(_layout(img, layout, np.inf)[1], oview, role=role, **params)
                assert _same(obuf, _expect(want, layout, np.float32)), (role, params, layout)
            half = _half(img)
            widened = np.full((h, w, 3), -7.0, np.float32)
            nn.images_host(half.astype(np.float32), widened, role=role, **params)
            hbuf, hview = _layout(np.zeros((h, w, 3), np.float16), "x4")
            nn.images_host(_layout(half, "x4")[1], hview, role=role, **params)
            assert _same(hbuf, _expect(widened, "x4", np.float16)), (role, params)
        assert w == 1 or (clean_a.std() > 0 and clean_n.std() > 0)
        for kw, text in ((dict(role="albedo", hdr=1), "hdr != 0"), (dict(role="normal", srgb=1), "srgb != 0"), (dict(role="normal", samples=2), "samples != 1")):
            with pytest.raises(pt.PathTracerError, match=text):
                nn.images_host(a, out, **kw)


# ---- 5: in place ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", FRAMES)
def test_in_place_with_one_tile(gpu_product, w, h):
    """the output aliased exactly to the colour, then shifted by one pixel against it"""
    pt = gpu_product
    rgb, alb, _ = _inputs(w, h, 6, 500 + w)
    with pt.NN(w, h, _blob(6)) as nn:
        assert nn.tiling(tiles=False)["tiles_x"] * nn.tiling(tiles=False)["tiles_y"] == 1
        for mode in (dict(), dict(hdr=1)):
            want = nn.host(rgb, alb, **mode)
            same = rgb.copy()
            nn.images_host(same, same, albedo=alb, **mode)
            assert beq(same, want), mode
            for lead in (0, 1):                       # the colour one pixel behind the output, then one pixel ahead of it
                flat = np.full((w * h + 1) * 3, -7.0, np.float32)
                views = flat[:-3].reshape(h, w, 3), flat[3:].reshape(h, w, 3)
                color, out = views[lead], views[1 - lead]
                color[...] = rgb
                nn.images_host(color, out, albedo=alb, **mode)
                assert beq(out, want), (mode, lead)


def test_in_place_with_more_than_one_tile(gpu_product):
    """289 x 17 under 1 MiB with the narrow table: two tiles.  Out of place the tiled image call is the one-tile packed call; with the
    output in the colour buffer, then in the albedo buffer, it still is; and so with a half4 buffer as colour and output."""
    import torch
    pt = gpu_product
    w, h = 289, 17
    blob = _blob(6, "narrow")
    rgb, alb, _ = _inputs(w, h, 6, 900)
    with pt.NN(w, h, blob) as one, pt.NN(w, h, blob, max_memory_mb=1) as tiled:
        t = tiled.tiling(tiles=False)
        assert t["tiles_x"] * t["tiles_y"] > 1
        for mode in (dict(), dict(hdr=1)):
            want = one.host(rgb, alb, **mode)
            scale = one.scale()
            out = np.full((h, w, 3), -7.0, np.float32)
            tiled.images_host(rgb, out, albedo=alb, **mode)
            assert beq(out, want) and tiled.scale().tobytes() == scale.tobytes(), mode
            for target in ("colour", "albedo"):
                c, a = rgb.copy(), alb.copy()
                tiled.images_host(c, c if target == "colour" else a, albedo=a, **mode)
                assert beq(c if target == "colour" else a, want), (mode, target)
                assert beq(a if target == "colour" else c, alb if target == "colour" else rgb)
            # float4 buffers, the output over the colour: every alpha stays
            cbuf, cview = _layout(rgb, "x4", 123.0)
            tiled.images_host(cview, cview, albedo=_layout(alb, "x4")[1], **mode)
            assert _same(cbuf, _expect(want, "x4", np.float32, 123.0)), mode
            # half4: colour and output in one buffer
            hrgb, halb = _half(rgb), _half(alb)
            hwant = one.host(hrgb.astype(np.float32), halb.astype(np.float32), **mode)
            hbuf, hview = _layout(hrgb, "x4", 123.0)
            tiled.images_host(hview, hview, albedo=_layout(halb, "x4")[1], **mode)
            assert _same(hbuf, _expect(hwant, "x4", np.float16, 123.0)), mode
        assert want.std() > 0
        # the old entry point still refuses the overlap
        d = torch.from_numpy(rgb).to("cuda:0")
        da = torch.from_numpy(alb).to("cuda:0")
        with pytest.raises(pt.PathTracerError, match="may not overlap"):
            tiled.device(d.data_ptr(), d.data_ptr(), albedo_ptr=da.data_ptr())


# ---- 6: one handle, several layouts; the device form on a stream --------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", FRAMES[:2])
def test_device_form_on_a_stream_and_calls_in_a_row(gpu_product, w, h):
    import torch
    pt = gpu_product
    rgb, alb, _ = _inputs(w, h, 6, 700 + w)
    with pt.NN(w, h, _blob(6)) as nn:
        want = nn.host(rgb, alb, hdr=1)
        # two calls in a row with different layouts on one handle
        o1, v1 = _layout(np.zeros_like(rgb), "offset")
        nn.images_host(_layout(rgb, "x4")[1], v1, albedo=_layout(alb, "pitch")[1], hdr=1)
        o2, v2 = _layout(np.zeros((h, w, 3), np.float16), "pitch")
        nn.images_host(_layout(rgb, "pitch")[1], v2, albedo=_layout(alb, "offset")[1], hdr=1)
        assert _same(o1, _expect(want, "offset", np.float32)) and _same(o2, _expect(want, "pitch", np.float16))
        # the device form: float4 colour with a row pitch, packed albedo, half4 output, on a stream of torch's
        stream = torch.cuda.Stream(device="cuda:0")
        cbuf, _ = _layout(rgb, "offset", 5.0)
        obuf, _ = _layout(np.zeros((h, w, 3), np.float16), "x4")
        with torch.cuda.stream(stream):
            dc, da, do = torch.from_numpy(cbuf).to("cuda:0"), torch.from_numpy(alb).to("cuda:0"), torch.from_numpy(obuf).to("cuda:0")
            row = (w + 5) * 16
            color = pt.nn_image_of(dc.data_ptr(), format=pt.NN_FORMAT_FLOAT3, byte_offset=row + 2 * 16 + 4, pixel_stride=16, row_stride=row)
            nn.images_device(color, pt.nn_image_of(do.data_ptr(), format=pt.NN_FORMAT_HALF3, pixel_stride=8),
                             albedo=pt.nn_image_of(da.data_ptr(), format=pt.NN_FORMAT_FLOAT3), hdr=1, stream=stream.cuda_stream)
            got = do.cpu().numpy()
        stream.synchronize()
        assert _same(got, _expect(want, "x4", np.float16)) and beq(dc.cpu().numpy(), cbuf)


# ---- the veneer ------------------------------------------------------------------------------------------------------------------------------------
def test_oidn_veneer_runs_cpudenoises_sequence(gpu_product, tmp_path):
    """tests/oidn_veneer_check.cpp at 33 x 17 on synthetic blobs written as OIDN names them"""
    pt = gpu_product
    w, h = 33, 17
    pkg = os.path.join(ROOT, "mygpuraytracer_amd")
    exe = tmp_path / "oidn_veneer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", str(exe), os.path.join(ROOT, "tests", "oidn_veneer_check.cpp"),
                           "-L" + pkg, "-lmi355x_pathtracer", "-Wl,-rpath," + pkg + ",-rpath,/opt/rocm/lib"])
    wdir = tmp_path / "weights"
    wdir.mkdir()
    blobs = {"rt_ldr_alb": _blob(6), "rt_alb": _blob(3, seed=4), "rt_hdr_alb": _blob(6, seed=2)}
    for name, blob in blobs.items():
        (wdir / (name + ".tza")).write_bytes(blob)
    rgb, alb, _ = _inputs(w, h, 6, 41)
    rgb = np.abs(rgb) * np.float32(30)
    rgb.tofile(str(tmp_path / "in.color"))
    alb.tofile(str(tmp_path / "in.albedo"))
    r = subprocess.run([str(exe), str(wdir), str(w), str(h), str(tmp_path / "in"), str(tmp_path / "out")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "oidn veneer ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rd = lambda ext, shape=(h, w, 3): np.fromfile(str(tmp_path / "out") + ext, np.float32).reshape(shape)
    with pt.NN(w, h, blobs["rt_ldr_alb"]) as nn:
        want = nn.host(rgb, alb)
        assert beq(rd(".ldr"), want) and beq(rd(".moved"), want) and want.std() > 0
    with pt.NN(w - 1, h, blobs["rt_ldr_alb"]) as nn:
        assert beq(rd(".small", (h, w - 1, 3)), nn.host(rgb[:, :w - 1], alb[:, :w - 1]))
    with pt.NN(w, h, blobs["rt_alb"]) as nn:
        role = np.zeros((h, w, 3), np.float32)
        nn.images_host(alb, role, role="albedo")
        assert beq(rd(".alb"), role) and role.std() > 0
    with pt.NN(w, h, blobs["rt_hdr_alb"]) as nn:
        want = nn.host(rgb, alb, hdr=1)
        assert beq(rd(".hdr"), want) and want.std() > 0
        assert rd(".scale", (1,)).tobytes() == nn.scale().tobytes() and nn.scale() not in (0.0, 1.0)
