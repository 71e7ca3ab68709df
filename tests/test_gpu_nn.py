"""GPU: the network denoiser (ptx_nn_*, csrc/pt_nn.hip) against its restatement (tests/unet_ref.py), on synthetic weights only: nothing
here is about image quality.  One layer bit for bit on exact data and against a derived bound on random data, for every (Cin, Cout)
pair of the standard network in its plain, two-source and pooled forms; the transfer functions; the whole network against the float64
restatement with the float32 restatement as the yardstick; the modes; the plumbing through the tracer.

The convolution's spatial tile is TILE x TILE = 16 x 16 output pixels (four waves of four rows); 38 x 22 crosses it in both directions
and leaves a remainder of 6 in each."""
import os

import numpy as np
import pytest

import unet_ref as U
from conftest import ROOT, beq
from nncases import exact_case as _exact_case, random_case

pytestmark = pytest.mark.gpu

TILE = 16
ICS = (3, 6, 9)
# every (cin, cout) of the standard network with ic = 3, 6, 9, as one-source layers (dec_conv1a's 64 + ic among them)
PLAIN = sorted({(sum(cin) if isinstance(cin, tuple) else cin, cout) for ic in ICS for _, cin, cout in U.standard_channels(ic)})
# the four dec_conv*a: (upsampled cin0, skip cin1, cout)
TWO = sorted({cin + (cout,) for ic in ICS for _, cin, cout in U.standard_channels(ic) if isinstance(cin, tuple)})
# enc_conv1 .. 4, which write only their pooled output
POOLED = [(U.EC1, U.EC1), (U.EC1, U.EC2), (U.EC2, U.EC3), (U.EC3, U.EC4)]


@pytest.mark.parametrize("cin,cout", PLAIN)
def test_one_layer_exact_plain(gpu_product, cin, cout):
    for k, (w, h) in enumerate(((38, 22), (1, 1), (TILE, TILE))):
        _exact_case(gpu_product, w, h, cin, 0, cout, False, 1000 * cin + cout + k)


@pytest.mark.parametrize("cin0,cin1,cout", TWO)
def test_one_layer_exact_two_sources(gpu_product, cin0, cin1, cout):
    for k, (w, h) in enumerate(((38, 22), (2, 2), (TILE, TILE))):
        _exact_case(gpu_product, w, h, cin0, cin1, cout, False, 7000 * cin0 + 10 * cin1 + cout + k)


@pytest.mark.parametrize("cin,cout", POOLED)
def test_one_layer_exact_pooled(gpu_product, cin, cout):
    for k, (w, h) in enumerate(((38, 22), (2, 2), (TILE, TILE))):
        _exact_case(gpu_product, w, h, cin, 0, cout, True, 3000 * cin + cout + k)


@pytest.mark.parametrize("cin0,cin1,cout", [(c, 0, o) for c, o in PLAIN] + TWO)
def test_one_layer_random_within_the_summation_bound(gpu_product, cin0, cin1, cout):
    """Inputs from {0} and [2^-10, 2) (no fp16 subnormals), He-scaled weights, both fp16 values.  s = the float64 result on them;
    E = 2 K 2^-24 (|b| + sum |w| |x|), K = 9 Cin: twice the standard summation bound, the matrix core's order and rounding being its own;
    every output is within E + 2^-11 (|relu(s)| + E) + 2^-25 of relu(s): the sum's error, then one rounding to fp16."""
    random_case(gpu_product, cin0, cin1, cout)


def _sweep():
    """log-spaced values with 0, the branch points and their fp32 neighbours, 65504, NaN, negatives and values above 1, as an (H, W, 3) frame"""
    f = np.float32
    special = [0.0, U.PU_Y0, U.PU_Y1, U.SRGB_Y0, U.PU_X0, U.PU_X1, U.SRGB_X0, 1.0, 65504.0, np.nan, -0.5, -1e30, 1.5, 2.0, 1e30, np.inf]
    special += [float(np.nextafter(f(v), f(np.inf))) for v in special[1:7]] + [float(np.nextafter(f(v), f(-np.inf))) for v in special[1:7]]
    v = np.concatenate([np.asarray(special, np.float32), (10.0 ** np.linspace(-9, 5, 3 * 37 * 23 - len(special))).astype(np.float32)])
    return v.reshape(23, 37, 3)


@pytest.mark.parametrize("hdr,srgb", [(1, 0), (0, 0), (0, 1)])
def test_transfer_functions(gpu_product, hdr, srgb):
    """forward within 2^-18 relative of the float64 restatement on the same fp32 inputs (powf and logf are good to a few ulp; the
    value is rounded to fp16, 2^-11, next), inverse within 2^-16 relative + 2^-24 absolute (exp's argument reaches about 11, so its own
    rounding is amplified to about 2^-19.5); NaN, negative colour and albedo above 1 come out exactly"""
    pt = gpu_product
    rgb = _sweep()
    alb, nrm = rgb.copy(), (rgb - 1).astype(np.float32)
    for scale in (1.0, 0.37):
        got = pt.kat_nn_transfer(rgb, alb, nrm, hdr=hdr, srgb=srgb, scale=scale).astype(np.float64)
        want = U.input_transform(rgb, alb, nrm, hdr, srgb, scale)
        err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        print("forward hdr %d srgb %d scale %g: max relative error 2^%.1f" % (hdr, srgb, scale, np.log2(max(err[want != 0].max(), 1e-30))))
        assert (np.abs(got - want) <= 2.0 ** -18 * np.abs(want)).all()
        bad = np.isnan(rgb) | (rgb <= 0)
        assert (got[..., :3][bad] == 0).all() and (got[..., 3:6][bad] == 0).all()                # sanitised: exactly 0
        assert (got[..., 3:6][rgb >= 1] == 1).all() and (got[..., 6:][nrm >= 1] == 1).all() and (got[..., 6:][nrm <= -1] == 0).all()
        net = np.where(np.isinf(rgb), np.float32(1.25), rgb) if hdr else rgb                     # (PU^-1 of a huge value is inf - inf territory)
        net = np.where(net > 1.3, np.float32(1.3), net) if hdr else net                          # the network's range: PU(65504) / PU(65504) = 1
        goti = pt.kat_nn_transfer(net, hdr=hdr, srgb=srgb, scale=scale, inverse=True).astype(np.float64)
        wanti = U.output_transform(net, hdr, srgb, scale)
        fin = np.isfinite(wanti) & (wanti < 3e38)
        assert (np.abs(goti - wanti)[fin] <= 2.0 ** -16 * np.abs(wanti[fin]) + 2.0 ** -24).all()
        assert (goti[np.isnan(net) | (net <= 0)] == 0).all()
    assert (pt.kat_nn_transfer(net, hdr=hdr, srgb=srgb, scale=0.0, inverse=True) == 0).all()      # scale 0: times 0


_NET = {}


def _net_case(ic, w, h, seed):
    """one synthetic network and frame with both restatements' raw outputs (before the output transform), computed once"""
    key = (ic, w, h, seed)
    if key not in _NET:
        rng = np.random.default_rng(seed)
        weights = U.synthetic_weights(ic, seed)
        rgb = rng.random((h, w, 3), dtype=np.float32)
        alb = rng.random((h, w, 3), dtype=np.float32) if ic >= 6 else None
        nrm = (rng.random((h, w, 3), dtype=np.float32) * 2 - 1) if ic >= 9 else None
        _NET[key] = dict(weights=weights, blob=U.weights_blob(weights), rgb=rgb, alb=alb, nrm=nrm)
    return _NET[key]


# seeds for which the condition 4 max|A - B| <= rms(A) / 4 holds on the CPU (asserted below)
@pytest.mark.parametrize("ic,seed", [(3, 1), (6, 2), (9, 1)])
@pytest.mark.parametrize("w,h", [(16, 16), (33, 17), (86, 70)])
def test_whole_network_against_the_float64_restatement(gpu_product, ic, seed, w, h):
    """linear mode (srgb = 1, scale 1) through nn_denoise_buffers.  A = the float64 restatement, B = the float32 one: they differ by the
    summation order alone, hence by a few flipped fp16 roundings, and the device's order is a third of the same kind:
    max|gpu - A| <= 4 max|A - B| and the same for the RMS.  4 max|A - B| <= rms(A) / 4, so the bound cannot hide a wiring error (concat
    order, dec_conv1a's padded blocks, pool and upsample indexing, the right / bottom padding), which costs O(rms(A))."""
    pt = gpu_product
    c = _net_case(ic, w, h, seed)
    A = U.denoise(c["rgb"], c["weights"], c["alb"], c["nrm"], srgb=1)
    B = U.denoise(c["rgb"], c["weights"], c["alb"], c["nrm"], srgb=1, dtype_name="float32")
    got = pt.nn_denoise_buffers(c["blob"], c["rgb"], c["alb"], c["nrm"], srgb=1).astype(np.float64)
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    print("ic %d %dx%d: max|A-B| %.3g rms|A-B| %.3g rms(A) %.3g; max|gpu-A| %.3g rms|gpu-A| %.3g" % (
        ic, w, h, np.abs(A - B).max(), rms(A - B), rms(A), np.abs(got - A).max(), rms(got - A)))
    assert 4 * np.abs(A - B).max() <= rms(A) / 4
    assert np.abs(got - A).max() <= 4 * np.abs(A - B).max()
    assert rms(got - A) <= 4 * rms(A - B)


@pytest.mark.parametrize("hdr,srgb,scale", [(1, 0, 0.5), (0, 0, 1.0)])
def test_modes(gpu_product, hdr, srgb, scale):
    """output = inverse(net(forward(.))): the network's input is what the input kernel itself computed (ptx_kat_nn_transfer, held to the
    restatement by test_transfer_functions), so that no fp16 rounding of the input is flipped by the transfer's last bits; d = 4 max|A - B|
    on the network's raw output is carried through the float64 inverse, which is monotone, plus the inverse's own tolerance"""
    pt = gpu_product
    ic, w, h = 6, 33, 17
    c = _net_case(ic, w, h, 2)
    # dec_conv0 scaled to a quarter around 0.45, so that the network's output lies in about [0.35, 1]: the range the inverse transfers
    # are made for (PU^-1 of a synthetic network's raw output, several units wide, would be exp of dozens)
    weights = dict(c["weights"])
    weights["dec_conv0.weight"] = (weights["dec_conv0.weight"] * 0.25).astype(np.float32)
    weights["dec_conv0.bias"] = np.full(3, 0.45, np.float32)
    blob = U.weights_blob(weights)
    rgb = (c["rgb"] * (4.0 if hdr else 1.2)).astype(np.float32)
    x = pt.kat_nn_transfer(rgb, c["alb"], None, hdr=hdr, srgb=srgb, scale=scale)[..., :ic]
    netA, netB = U.unet(x, weights), U.unet(x, weights, "float32")
    d = 4 * np.abs(netA - netB).max()
    out = lambda net: U.output_transform(net, hdr, srgb, scale)
    A = out(netA)
    slack = np.maximum(np.abs(out(netA + d) - A), np.abs(out(netA - d) - A)) + 2.0 ** -16 * np.abs(A) + 2.0 ** -24 / scale
    got = pt.nn_denoise_buffers(blob, rgb, c["alb"], None, hdr=hdr, srgb=srgb, input_scale=scale).astype(np.float64)
    print("hdr %d srgb %d: d %.3g, network output %.3g .. %.3g (std %.3g), result %.3g .. %.3g, largest |gpu - A| / slack %.3g" % (
        hdr, srgb, d, netA.min(), netA.max(), netA.std(), A.min(), A.max(), (np.abs(got - A) / slack).max()))
    assert netA.min() > 0.2 and netA.max() < 1.5 and A.max() < 1e6          # (the case itself: the range meant above)
    assert (np.abs(got - A) <= slack).all()
    assert d <= netA.std() / 4                                # the bound cannot hide a wiring error, which costs O(std)


def test_automatic_scale_is_the_display_meter(gpu_product):
    """hdr with input_scale NaN: the scale the input kernel used is Display's `metered` of the same frame at key 0.18, bit for bit; the
    result is that of the same scale given explicitly; without hdr the automatic scale is 1"""
    pt = gpu_product
    ic, w, h = 3, 86, 70
    c = _net_case(ic, w, h, 1)
    rgb = (c["rgb"] * 7.5).astype(np.float32)
    rgb[3, 4] = np.nan
    with pt.NN(w, h, c["blob"]) as nn, pt.Display(w, h) as D:
        with pytest.raises(pt.PathTracerError, match="no denoise"):
            nn.scale()
        auto = nn.host(rgb, samples=2, hdr=1)
        scale = nn.scale()
        D.host(rgb, samples=2, key=0.18)
        metered = np.float32(D.status()["metered"])
        assert scale.tobytes() == metered.tobytes() and scale != 1
        assert beq(auto, nn.host(rgb, samples=2, hdr=1, input_scale=float(scale)))
        nn.host(rgb)
        assert nn.scale() == 1


def _scene(pt, name, res, depth=4):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s


@pytest.mark.parametrize("ic,bounces", [(9, 0), (9, 2), (6, 0), (3, 0)])
def test_tracer_denoise_nn_is_nn_denoise_buffers_on_its_own_frames(gpu_product, ic, bounces):
    pt = gpu_product
    W, H, spp = 64, 48, 3
    c = _net_case(ic, W, H, 1)
    s = _scene(pt, "cornellGlass.txt" if bounces else "cornell.txt", (W, H), depth=6)
    with pt.NN(W, H, c["blob"]) as nn, pt.Tracer(s) as T, pt.Tracer(s) as other:
        if bounces:
            T.set_guide_bounces(bounces)
        T.render(1, spp)
        other.render(1, spp)
        got = T.denoise_nn(nn, spp)
        g = T.gbuffer()
        mean = (T.read_image().reshape(H, W, 3) / np.float32(spp)).astype(np.float32)
        want = pt.nn_denoise_buffers(c["blob"], mean, g["albedo"] if ic >= 6 else None, g["normal"] if ic >= 9 else None)
        assert beq(got, want.reshape(got.shape)) and got.any()
        assert beq(T.denoise_nn(nn, spp), got)                                   # the same bits on every run
        assert T.device_denoised_ptr()
        # the frame, the statistics and a following iteration are those of a tracer that never saw the network
        assert beq(T.read_image(), other.read_image()) and T.stats()["rays_per_bounce"] == other.stats()["rays_per_bounce"]
        T.render(spp + 1, 1)
        other.render(spp + 1, 1)
        assert beq(T.read_image(), other.read_image())


def test_a_handle_serves_two_tracers_and_streams(gpu_product):
    import torch
    pt = gpu_product
    W, H = 64, 48
    c = _net_case(6, W, H, 1)
    s = _scene(pt, "cornell.txt", (W, H))
    st = torch.cuda.Stream()
    with pt.NN(W, H, c["blob"]) as nn, pt.Tracer(s) as T1, pt.Tracer(s, stream_ptr=st.cuda_stream) as T2:
        T1.render(1, 2)
        T2.render(1, 2)
        a = T1.denoise_nn(nn, 2, read=False)
        b = T2.denoise_nn(nn, 2)
        assert a is None and beq(T1.read_denoised(), b)
        info = nn.info()
        assert info["input_channels"] == 6 and [(n, o) for n, _, o in info["layers"]] == [(n, o) for n, _, o in U.standard_channels(6)]
        assert info["padded_width"] == 64 and info["padded_height"] == 48 and info["scratch_bytes"] > 0
        assert info["macs"] == sum(9 * (sum(ci) if isinstance(ci, tuple) else ci) * co * (W >> lv) * (H >> lv)
                                   for (_, ci, co), lv in zip(U.standard_channels(6), (0, 0, 1, 2, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 0)))


def test_refusals(gpu_product):
    import torch
    pt = gpu_product
    W, H = 37, 23
    c3, c6, c9 = (_net_case(ic, W, H, 1) for ic in ICS)
    s = _scene(pt, "cornell.txt", (W, H))
    with pytest.raises(pt.PathTracerError, match="bad frame size"):
        pt.NN(7681, 4320, c3["blob"])
    with pytest.raises(pt.PathTracerError, match="bad frame size"):
        pt.NN(0, 4, c3["blob"])
    with pytest.raises(pt.PathTracerError, match="device ordinal"):
        pt.NN(W, H, c3["blob"], device=64)
    with pytest.raises(pt.PathTracerError, match="weight blob"):
        pt.NN(W, H, c3["blob"][:100])
    with pt.NN(W, H, c6["blob"]) as nn, pt.NN(W + 1, H, c6["blob"]) as other, pt.NN(W, H, c3["blob"]) as nn3, pt.NN(W, H, c9["blob"]) as nn9:
        with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as T:
            T.render(1, 1)
            with pytest.raises(pt.PathTracerError, match="row tile"):
                T.denoise_nn(nn, 1)
        with pt.Tracer(s) as T:
            T.render(1, 1)
            with pytest.raises(pt.PathTracerError, match="size 38 x 23 differs"):
                T.denoise_nn(other, 1)
            with pytest.raises(pt.PathTracerError, match="spp"):
                T.denoise_nn(nn, 0)
            for bad, what in ((dict(hdr=2), "hdr"), (dict(srgb=-1), "srgb"), (dict(input_scale=-1.0), "input_scale"), (dict(input_scale=float("inf")), "input_scale")):
                with pytest.raises(pt.PathTracerError, match=what):
                    T.denoise_nn(nn, 1, **bad)
            with pytest.raises(pt.PathTracerError, match="no ptx_denoise"):
                T.read_denoised()
        if torch.cuda.device_count() > 1:
            with pt.NN(W, H, c6["blob"], device=1) as far, pt.Tracer(s) as T:
                with pytest.raises(pt.PathTracerError, match="created on device 1"):
                    T.denoise_nn(far, 1)
        d = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
        p = d.data_ptr()
        with pytest.raises(pt.PathTracerError, match="albedo is required"):
            nn.device(p, p)
        with pytest.raises(pt.PathTracerError, match="normals must be NULL"):
            nn.device(p, p, albedo_ptr=p, normal_ptr=p)
        with pytest.raises(pt.PathTracerError, match="albedo must be NULL"):
            nn3.device(p, p, albedo_ptr=p)
        with pytest.raises(pt.PathTracerError, match="normals are required"):
            nn9.device(p, p, albedo_ptr=p)
        with pytest.raises(pt.PathTracerError, match="samples"):
            nn3.device(p, p, samples=0)
        with pytest.raises(pt.PathTracerError, match="null"):
            nn3.device(0, p)
        with pytest.raises(pt.PathTracerError, match="no denoise"):
            nn3.scale()                                                           # nothing of all that was enqueued
