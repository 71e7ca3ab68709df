"""GPU: the lightmap filter (csrc/pt_nn_lightmap.hip, ptx_nn_denoise_lightmap_*) on synthetic weights.  The directional mode is held
to the normal role of ptx_nn_denoise_images_* byte for byte; the HDR mode to its float64 restatement (tests/nn_lightmap_ref.py) through
a pass-through network and through a random one, within bounds that come from the number formats and from the restatements' own
difference; layouts, halves, in place and tiles to the packed float call's bytes.  No image-quality claim."""
import numpy as np
import pytest

import nn_image_ref as R
import nn_lightmap_ref as LM
import unet_aux_ref as X
import unet_ref as U
from conftest import beq
from test_gpu_nn import _net_case, _sweep
from test_gpu_nn_image import LAYOUTS, _blob, _expect, _gauss, _half, _layout, _same

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _out(h, w, dtype=np.float32):
    return np.full((h, w, 3), -7.0, dtype)


# ---- 1: directional is the normal role ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("w,h", [(33, 17), (16, 16)])
def test_directional_is_the_normal_role_byte_for_byte(gpu_product, w, h, scale):
    """lightmap_host(directional=True) against images_host(role="normal") on the same 3-input blob: packed, float4, pitched, offset
    and half4 images, the whole output buffer compared, so the sentinels between the pixels too"""
    pt = gpu_product
    img = _gauss(w, h, 40 + w, 0.9)
    with pt.NN(w, h, _blob(3, seed=4)) as nn:
        for layout in LAYOUTS:
            for dtype in (np.float32, np.float16) if layout == "x4" else (np.float32,):
                src = img if dtype == np.float32 else _half(img)
                cbuf, cview = _layout(src, layout, 5e4)
                wbuf, wview = _layout(np.zeros((h, w, 3), dtype), layout)
                nn.images_host(cview, wview, role="normal", input_scale=scale)
                before = cbuf.copy()
                gbuf, gview = _layout(np.zeros((h, w, 3), dtype), layout)
                nn.lightmap_host(cview, gview, directional=True, input_scale=scale)
                assert _same(gbuf, wbuf), (layout, dtype)
                assert _same(cbuf, before)
                assert (np.asarray(gbuf, np.float32).reshape(-1) == -7).sum() == gbuf.size - 3 * w * h or layout == "packed"
        want, got = _out(h, w), _out(h, w)
        nn.images_host(img, want, role="normal", input_scale=scale)
        nn.lightmap_host(img, got, directional=True, input_scale=scale)
        assert beq(got, want) and want.std() > 0
        if scale == 1.0:                                                       # NaN: 1
            nn.lightmap_host(img, got, directional=True)
            assert beq(got, want) and nn.scale() == 1
        # and the float32 restatement of the ends around a pass-through network: the device's bits
    blob = U.weights_blob(X.passthrough_weights(3, (0, 1, 2), 1.0))
    with pt.NN(w, h, blob) as nn:
        got = _out(h, w)
        nn.lightmap_host(img, got, directional=True, input_scale=scale)
        assert beq(got, LM.output_f32(X.passthrough(LM.input_f32(img, True, scale)), True, scale))


# ---- 2: HDR through a pass-through network ------------------------------------------------------------------------------------------------
def _fp16_step(h):
    """the spacing of fp16 at the fp16 value h (float64 in, float64 out)"""
    h16 = np.asarray(h, np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        up = np.nextafter(h16, np.float16(np.inf)).astype(np.float64)
    return np.where(np.isfinite(up), up - h16.astype(np.float64), 0.0)


@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_hdr_against_the_restatement_through_a_pass_through_network(gpu_product, scale):
    """The network hands fp16(forward(v)) through, so the result is inverse(fp16(forward(v))) / scale.  want: the float64 inverse of
    fp16(forward64).  Within 2^-16 |want| + 2^-24 / scale (the inverse's bound of test_gpu_nn.py::test_transfer_functions); a value whose
    forward rounds to the neighbouring fp16 may use one fp16 step of the network's input carried through the float64 inverse instead,
    and at most 1 % may.  The float32 numpy restatement needs that for at most one of the 2553, which is the premise.  Where want is
    beyond FLT_MAX (inf at scale 0.25: exp(88.7) * 4) the fp32 result is +inf.  NaN, negatives and inputs below 2^-24 (v + 1 == 1: 324
    of the 2553) come out as exactly 0."""
    pt = gpu_product
    rgb = _sweep()
    h, w = rgb.shape[:2]
    assert (w, h) == (37, 23)
    blob = U.weights_blob(X.passthrough_weights(3, (0, 1, 2), 1.0))
    x16 = X.passthrough(LM.input_f64(rgb, False, scale).astype(np.float32)).astype(np.float64)      # fp16(forward64)
    want = LM.output_f64(x16, False, scale)
    step = _fp16_step(x16)
    base = 2.0 ** -16 * np.abs(want) + 2.0 ** -24 / scale
    alt = np.maximum(np.abs(LM.output_f64(x16 + step, False, scale) - want), np.abs(LM.output_f64(np.maximum(x16 - step, 0), False, scale) - want)) + base
    fits = want <= U.FLT_MAX

    def share(got, who):
        got = got.astype(np.float64)
        assert np.isposinf(got[~fits]).all(), who
        err = np.abs(got - want)[fits]
        needs = err > base[fits]
        print("%s scale %g: %d of %d beyond FLT_MAX; largest err / base %.3g; %d of %d use the fp16 step" % (
            who, scale, (~fits).sum(), want.size, (err / base[fits]).max(), needs.sum(), want.size))
        assert (err <= alt[fits]).all(), who
        return needs.sum()

    # the premise: the float32 restatement itself.  1 of 2553 at scale 1 (8077.74, whose forward lies 3e-8 from a tie of fp16) and 0 at 0.25
    assert share(LM.output_f32(X.passthrough(LM.input_f32(rgb, False, scale)), False, scale), "float32 restatement") <= 1
    with pt.NN(w, h, blob) as nn:
        got = _out(h, w)
        nn.lightmap_host(rgb, got, input_scale=scale)
        assert nn.scale() == np.float32(scale)
        assert share(got, "device") <= want.size // 100
        with np.errstate(invalid="ignore"):
            below = rgb < 2.0 ** -24                                            # the negatives among them; v + 1 == 1
            assert int(below.sum()) == 324 and int(np.isnan(rgb).sum()) == 1
            v = X._sanitise32((rgb * np.float32(scale)).astype(np.float32), 0.0, X.FLT_MAX32)
        tiny = (v + np.float32(1)).astype(np.float32) == 1
        assert tiny[below].all() and tiny[np.isnan(rgb)].all() and (x16[tiny] == 0).all()
        assert (got[x16 == 0] == 0).all() and not np.signbit(got[x16 == 0]).any() and (got[x16 > 0] > 0).all()
        # a scale of 0 cannot be given (and the meter never yields one): refused, nothing written
        keep = got.copy()
        with pytest.raises(pt.PathTracerError, match="input_scale must be NaN \\(automatic\\) or finite and > 0"):
            nn.lightmap_host(rgb, got, input_scale=0.0)
        assert beq(got, keep)


# ---- 3: HDR on a random network ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(33, 17), (86, 70)])
def test_hdr_on_a_random_network_within_the_restatements_own_difference(gpu_product, w, h):
    """test_gpu_nn.py::test_modes' bound: A = the float64 network on the float32 input transform's values, B = the float32 one; d =
    4 max|A - B| on the raw output carried through the float64 inverse (monotone), plus the inverse's own tolerance.  dec_conv0 is scaled
    to a quarter around 0.45, so the output stays in the inverse's range; d <= std / 4, so the bound cannot hide a wiring error."""
    pt = gpu_product
    scale = 0.5
    c = _net_case(3, w, h, 1)
    weights = dict(c["weights"])
    weights["dec_conv0.weight"] = (weights["dec_conv0.weight"] * 0.25).astype(np.float32)
    weights["dec_conv0.bias"] = np.full(3, 0.45, np.float32)
    rgb = (c["rgb"] * 4.0).astype(np.float32)
    # the network's input as the device forms it up to logf's last bits: the float32 restatement, rounded to fp16 by the network itself
    x = LM.input_f32(rgb, False, scale)
    netA, netB = U.unet(x, weights), U.unet(x, weights, "float32")
    # logf of the device against numpy's: an ulp of the input is far below an fp16 step, but may flip a rounding; that is B's kind of
    # difference and inside the factor 4
    d = 4 * np.abs(netA - netB).max()
    out = lambda net: LM.output_f64(net, False, scale)
    A = out(netA)
    slack = np.maximum(np.abs(out(netA + d) - A), np.abs(out(netA - d) - A)) + 2.0 ** -16 * np.abs(A) + 2.0 ** -24 / scale
    with pt.NN(w, h, U.weights_blob(weights)) as nn:
        got = _out(h, w)
        nn.lightmap_host(rgb, got, input_scale=scale)
    got = got.astype(np.float64)
    print("%dx%d: d %.3g, network output %.3g .. %.3g (std %.3g), result %.3g .. %.3g, largest |gpu - A| / slack %.3g" % (
        w, h, d, netA.min(), netA.max(), netA.std(), A.min(), A.max(), (np.abs(got - A) / slack).max()))
    assert netA.min() > 0.2 and netA.max() < 1.5 and A.max() < 1e7
    assert d <= netA.std() / 4
    assert (np.abs(got - A) <= slack).all()


# ---- 4: the automatic scale ---------------------------------------------------------------------------------------------------------------
def test_automatic_scale_is_the_display_meter(gpu_product):
    pt = gpu_product
    w, h = 86, 70
    c = _net_case(3, w, h, 1)
    rgb = (c["rgb"] * 7.5).astype(np.float32)
    rgb[3, 4] = np.nan
    with pt.NN(w, h, c["blob"]) as nn, pt.Display(w, h) as D:
        auto = _out(h, w)
        nn.lightmap_host(rgb, auto)
        scale = nn.scale()
        D.host(rgb, samples=1, key=0.18)
        metered = np.float32(D.status()["metered"])
        assert scale.tobytes() == metered.tobytes() and scale != 1
        given = _out(h, w)
        nn.lightmap_host(rgb, given, input_scale=float(scale))
        assert beq(auto, given) and np.isfinite(auto).all() and auto.std() > 0
        # a layout that is not packed is gathered for the meter: the same scale, the same bytes
        for layout in LAYOUTS[1:]:
            obuf, oview = _layout(np.zeros_like(rgb), layout)
            nn.lightmap_host(_layout(rgb, layout, 5e4)[1], oview)
            assert nn.scale().tobytes() == scale.tobytes() and _same(obuf, _expect(auto, layout, np.float32)), layout
        hrgb = _half(rgb)
        nn.lightmap_host(hrgb, given)
        hs = nn.scale()
        D.host(hrgb.astype(np.float32), samples=1, key=0.18)
        assert hs.tobytes() == np.float32(D.status()["metered"]).tobytes()


# ---- 5: layouts, halves, in place, tiles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(33, 17)])
def test_hdr_layouts_halves_and_in_place_give_the_packed_bytes(gpu_product, w, h):
    pt = gpu_product
    rgb = np.abs(_gauss(w, h, 9, 2.0))
    with pt.NN(w, h, _blob(3, "narrow", 2)) as nn:
        for scale in (NAN, 0.25):
            want = _out(h, w)
            nn.lightmap_host(rgb, want, input_scale=scale)
            for in_layout, out_layout in [(l, l) for l in LAYOUTS[1:]] + [("packed", "offset"), ("x4", "packed")]:
                cbuf, cview = _layout(rgb, in_layout, 5e4)
                obuf, oview = _layout(np.zeros_like(rgb), out_layout)
                before = cbuf.copy()
                nn.lightmap_host(cview, oview, input_scale=scale)
                assert _same(obuf, _expect(want, out_layout, np.float32)) and _same(cbuf, before), (scale, in_layout, out_layout)
            # half in: the widened image's result; half out: its rounding
            hrgb = _half(rgb)
            hwant = _out(h, w)
            nn.lightmap_host(hrgb.astype(np.float32), hwant, input_scale=scale)
            for layout in ("packed", "x4", "offset"):
                hbuf, hview = _layout(np.zeros((h, w, 3), np.float16), layout)
                nn.lightmap_host(_layout(hrgb, layout, 9.0)[1], hview, input_scale=scale)
                assert _same(hbuf, _expect(hwant, layout, np.float16)), (scale, layout)
            # the output over the colour, exactly and one pixel apart
            same = rgb.copy()
            nn.lightmap_host(same, same, input_scale=scale)
            assert beq(same, want)
            for lead in (0, 1):
                flat = np.full((w * h + 1) * 3, -7.0, np.float32)
                views = flat[:-3].reshape(h, w, 3), flat[3:].reshape(h, w, 3)
                color, out = views[lead], views[1 - lead]
                color[...] = rgb
                nn.lightmap_host(color, out, input_scale=scale)
                assert beq(out, want), (scale, lead)
        assert want.std() > 0 and np.isfinite(want[np.isfinite(rgb)]).all()


def test_two_tiles_out_of_place_and_in_place_are_the_one_tile_run(gpu_product):
    """289 x 17 under 1 MiB with the narrow table: two tiles; in place they go through the temporary and the copy-out"""
    import torch
    pt = gpu_product
    w, h = 289, 17
    blob = _blob(3, "narrow", 2)
    rgb = np.abs(_gauss(w, h, 901, 2.0))
    with pt.NN(w, h, blob) as one, pt.NN(w, h, blob, max_memory_mb=1) as tiled:
        t = tiled.tiling(tiles=False)
        assert t["tiles_x"] * t["tiles_y"] == 2
        for directional, scale in ((False, NAN), (False, 0.25), (True, NAN), (True, 0.37)):
            want = _out(h, w)
            one.lightmap_host(rgb, want, directional=directional, input_scale=scale)
            s = one.scale()
            out = _out(h, w)
            tiled.lightmap_host(rgb, out, directional=directional, input_scale=scale)
            assert beq(out, want) and tiled.scale().tobytes() == s.tobytes(), (directional, scale)
            c = rgb.copy()
            tiled.lightmap_host(c, c, directional=directional, input_scale=scale)
            assert beq(c, want), (directional, scale)
            cbuf, cview = _layout(rgb, "x4", 123.0)
            tiled.lightmap_host(cview, cview, directional=directional, input_scale=scale)
            assert _same(cbuf, _expect(want, "x4", np.float32, 123.0)), (directional, scale)
            hrgb = _half(rgb)
            hwant = _out(h, w)
            one.lightmap_host(hrgb.astype(np.float32), hwant, directional=directional, input_scale=scale)
            hbuf, hview = _layout(hrgb, "x4", 123.0)
            tiled.lightmap_host(hview, hview, directional=directional, input_scale=scale)
            assert _same(hbuf, _expect(hwant, "x4", np.float16, 123.0)), (directional, scale)
        assert want.std() > 0
        # the device form, in place, on a stream of torch's
        stream = torch.cuda.Stream(device="cuda:0")
        want = _out(h, w)
        one.lightmap_host(rgb, want, input_scale=0.25)
        with torch.cuda.stream(stream):
            d = torch.from_numpy(rgb).to("cuda:0")
            img = pt.nn_image_of(d.data_ptr(), format=pt.NN_FORMAT_FLOAT3)
            tiled.lightmap_device(img, img, input_scale=0.25, stream=stream.cuda_stream)
            got = d.cpu().numpy()
        stream.synchronize()
        assert beq(got, want)


# ---- 6: the smallest frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_the_smallest_frames_run_touch_their_own_bytes_and_repeat(gpu_product, w, h):
    pt = gpu_product
    rgb = np.abs(_gauss(w, h, 3 + w + 2 * h, 1.0))
    rgb[~np.isfinite(rgb)] = 0.5
    with pt.NN(w, h, _blob(3, "narrow", 2)) as nn:
        for directional in (False, True):
            for scale in (NAN, 0.5):
                runs = []
                for _ in range(2):
                    obuf, oview = _layout(np.zeros_like(rgb), "offset")
                    nn.lightmap_host(_layout(rgb, "offset", 5e4)[1], oview, directional=directional, input_scale=scale)
                    runs.append(obuf)
                assert _same(runs[0], runs[1]) and _same(runs[0], _expect(oview, "offset", np.float32)), (directional, scale)
                assert np.isfinite(oview).all() and (oview != -7).all()


def test_refusals_with_a_handle(gpu_product):
    pt = gpu_product
    w, h = 16, 16
    img = np.zeros((h, w, 3), np.float32)
    for ic in (6, 9):
        with pt.NN(w, h, _blob(ic)) as nn:
            with pytest.raises(pt.PathTracerError, match="the weights take %d input channels: a lightmap network takes the colour alone" % ic):
                nn.lightmap_host(img, img)
    with pt.NN(w, h, _blob(3)) as nn:
        with pytest.raises(pt.PathTracerError, match="directional must be 0"):
            nn.lightmap_host(img, img, directional=2)
        with pytest.raises(pt.PathTracerError, match="the output image: a row stride of"):
            nn.lightmap_host(img, pt.nn_image_of(img.ctypes.data, format=1, row_stride=12 * w - 4))
