"""GPU: the network denoiser's prefiltered guides (csrc/pt_nn_aux.hip, ptx_nn_prefilter_*, ptx_denoise_nn_prefiltered; OIDN's cleanAux)
on synthetic weights.  No expected image comes from the feature itself: the two kernels and the pass-through networks are held bit for
bit to the float32 numpy restatement (tests/unet_aux_ref.py), the albedo network to the tested LDR colour path of the network denoiser,
the normal network on random weights to the float64 restatement by the project's rule, and the cache to a fresh handle's results."""
import ctypes
import os

import numpy as np
import pytest

import unet_aux_ref as X
import unet_ref as U
from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

SPECIAL = [np.nan, np.inf, -np.inf, 3.0, -3.0, 1.0, -1.0, 0.0, -0.0]


def _with_specials(v):
    flat = v.reshape(-1)
    k = min(len(SPECIAL), flat.size)
    flat[:k] = np.asarray(SPECIAL[:k], np.float32)
    return v


def _gauss(w, h, seed):
    """(H, W, 3) float32 of N(0, 1) values with NaN, +-inf, +-3, +-1, 0 and -0 among them (as many as the frame holds)"""
    return _with_specials(np.random.default_rng(seed).standard_normal((h, w, 3)).astype(np.float32))


def _normals(w, h, seed, specials=True):
    n = np.random.default_rng(seed).standard_normal((h, w, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    return _with_specials(n) if specials else n


def _blob3(seed, counts=None):
    return U.weights_blob(U.synthetic_weights(3, seed, channels=U.table(3, *counts) if counts else None))


# ---- 1: the two kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_transforms_bit_for_bit(gpu_product, scale):
    """every step is one IEEE fp32 operation under -ffp-contract=off: the float32 numpy restatement's bits.  The albedo kind's sRGB
    curve has a powf: there the reference is the network denoiser's own colour path (hdr 0, samples 1), which tests/test_gpu_nn.py holds
    to its bounds."""
    pt = gpu_product
    v = _gauss(38, 22, 5)
    for kind, srgb in ((X.NORMAL, 0), (X.ALBEDO, 1)):
        fwd = pt.kat_nn_transfer_aux(v, kind, srgb=srgb, scale=scale)
        assert beq(fwd, X.aux_input_f32(v, kind, srgb, scale)), (kind, int((fwd.view(np.uint32) != X.aux_input_f32(v, kind, srgb, scale).view(np.uint32)).sum()))
        inv = pt.kat_nn_transfer_aux(v, kind, srgb=srgb, scale=scale, inverse=True)
        assert beq(inv, X.aux_output_f32(v, kind, srgb, scale)), (kind, int((inv.view(np.uint32) != X.aux_output_f32(v, kind, srgb, scale).view(np.uint32)).sum()))
    assert beq(pt.kat_nn_transfer_aux(v, X.ALBEDO, srgb=0, scale=scale), pt.kat_nn_transfer(v, hdr=0, srgb=0, scale=scale)[..., :3])
    assert beq(pt.kat_nn_transfer_aux(v, X.ALBEDO, srgb=0, scale=scale, inverse=True), pt.kat_nn_transfer(v, hdr=0, srgb=0, scale=scale, inverse=True))
    assert (pt.kat_nn_transfer_aux(v, X.NORMAL, scale=0.0, inverse=True) == 0).all()                # scale 0: times 0
    with pytest.raises(pt.PathTracerError, match="no transfer curve"):
        pt.kat_nn_transfer_aux(v, X.NORMAL, srgb=1)
    with pytest.raises(pt.PathTracerError, match="kind"):
        pt.kat_nn_transfer_aux(v, 3)


# ---- 2: the albedo network is the LDR colour filter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(38, 22), (1, 1)])
def test_albedo_filtering_is_the_ldr_colour_filter(gpu_product, w, h):
    import torch
    pt = gpu_product
    blob = _blob3(1)
    a = _with_specials((np.random.default_rng(3).random((h, w, 3)) * 1.2).astype(np.float32))
    with pt.NNPrefilter(w, h, albedo_tza=blob) as pf, pt.NN(w, h, blob) as nn:
        for srgb in (0, 1):
            got = pf.host(albedo=a, srgb=srgb)
            assert beq(got, nn.host(a, samples=1, hdr=0, srgb=srgb)) and (w == 1 or got.any())
            assert beq(pf.read(), got)
            # the same values at a stride of four floats (the G-buffer's records) give the same bits
            a4 = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
            a4[..., :3] = torch.from_numpy(a).to("cuda:0")
            pf.device(albedo_ptr=a4.data_ptr(), albedo_stride=4, srgb=srgb)
            assert beq(pf.read(), got)
        assert pf.info()["runs"] == 4 and pf.info()["normal"] is None and pf.info()["albedo"]["input_channels"] == 3
        with pytest.raises(pt.PathTracerError, match="normal image must be NULL"):
            pf.host(albedo=a, normal=a)
        with pytest.raises(pt.PathTracerError, match="albedo image is required"):
            pf.host()


# ---- 3: the normal network end to end, exact -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [1.0, 0.5])
@pytest.mark.parametrize("w,h", [(16, 16), (33, 17), (1, 1)])
def test_normal_filtering_through_a_pass_through_network_is_exact(gpu_product, w, h, g):
    """clean = clamp(fp16(g * fp16(clamp(n) * 0.5 + 0.5)) * 2 - 1), bit for bit; with g = 1 it is the normal to the fp16 rounding of a
    value in [0, 1] (at most 2^-12) doubled: 2^-11"""
    pt = gpu_product
    n = _normals(w, h, 11)
    blob = U.weights_blob(X.passthrough_weights(3, (0, 1, 2), g))
    with pt.NNPrefilter(w, h, normal_tza=blob) as pf:
        clean = pf.host(normal=n)
    want = X.aux_output_f32(X.passthrough(X.aux_input_f32(n, X.NORMAL), g), X.NORMAL)
    assert beq(clean, want), int((clean.view(np.uint32) != want.view(np.uint32)).sum())
    if g == 1.0:
        ok = ~np.isnan(n)
        err = np.abs(clean.astype(np.float64) - np.clip(n.astype(np.float64), -1, 1))[ok].max()
        print("%dx%d: max|clean - clamp(n)| %.4g" % (w, h, err))
        assert err <= 2.0 ** -11 and (clean[~ok] == 0).all()


# ---- 4: the normal network on random weights ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("w,h", [(38, 22), (33, 17)])
@pytest.mark.parametrize("counts", [None, U.NARROW], ids=["standard", "narrow"])
def test_normal_filtering_on_random_weights(gpu_product, counts, w, h, seed):
    """A = the float64 restatement of the whole auxiliary filter, B = the float32 one: max|gpu - A| <= 4 max|A - B| and the same for the
    RMS.  The case counts only while that bound is small against the image (4 max|A - B| <= std(A) / 4) and at least 0.4 of A lies
    strictly inside (-1, 1), where the output's clamp cannot hide an error."""
    pt = gpu_product
    weights = U.synthetic_weights(3, seed, channels=U.table(3, *counts) if counts else None)
    n = _normals(w, h, 100 + seed, specials=False)
    A = X.aux_denoise(n, X.NORMAL, weights)
    B = X.aux_denoise(n, X.NORMAL, weights, dtype_name="float32")
    with pt.NNPrefilter(w, h, normal_tza=U.weights_blob(weights)) as pf:
        got = pf.host(normal=n).astype(np.float64)
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    inside = float(np.mean(np.abs(A) < 1))
    print("%s %dx%d seed %d: max|A-B| %.3g rms|A-B| %.3g std(A) %.3g inside %.2f; max|gpu-A| %.3g rms|gpu-A| %.3g" % (
        "narrow" if counts else "standard", w, h, seed, np.abs(A - B).max(), rms(A - B), A.std(), inside, np.abs(got - A).max(), rms(got - A)))
    assert 4 * np.abs(A - B).max() <= A.std() / 4 and inside >= 0.4
    assert np.abs(got - A).max() <= 4 * np.abs(A - B).max()
    assert rms(got - A) <= 4 * rms(A - B)


# ---- 5: tiles and the shared scratch ------------------------------------------------------------------------------------------------------------
def test_tiles_and_the_one_scratch(gpu_product):
    pt = gpu_product
    W, H = 289, 17
    alb_blob, nrm_blob = _blob3(1), _blob3(2, U.NARROW)                     # two plans of different sizes in the one scratch
    a = np.random.default_rng(8).random((H, W, 3), dtype=np.float32)
    n = _normals(W, H, 9, specials=False)
    with pt.NNPrefilter(W, H, alb_blob, nrm_blob, max_memory_mb=1) as pf, pt.NNPrefilter(W, H, alb_blob, nrm_blob) as one:
        info, info1 = pf.info(), one.info()
        for key, blob in (("albedo", alb_blob), ("normal", nrm_blob)):
            plan = pt.debug_nn_tiling(blob, W, H, 1, tiles=False)
            assert (plan["tiles_x"], plan["tiles_y"]) == (2, 1)
            assert (info[key]["padded_width"], info[key]["padded_height"]) == (plan["tile_width"], plan["tile_height"]) == (288, 32)
            assert info[key]["scratch_bytes"] == plan["scratch_bytes"] and info[key]["macs"] == plan["macs"]
            assert (info1[key]["padded_width"], info1[key]["padded_height"]) == (304, 32)            # the whole frame, one tile
        for i in (info, info1):
            assert i["scratch_bytes"] == max(i["albedo"]["scratch_bytes"], i["normal"]["scratch_bytes"])
            assert i["albedo"]["scratch_bytes"] != i["normal"]["scratch_bytes"]
        want = one.host(a, n)
        first = pf.host(a, n)
        second = pf.host(a, n)
        for k in range(2):
            assert beq(first[k], want[k]) and beq(second[k], want[k]) and want[k].any()
        assert pf.info()["runs"] == 2
    # each network alone, with a scratch of its own size, gives the same: nothing is carried over between the two
    with pt.NNPrefilter(W, H, albedo_tza=alb_blob, max_memory_mb=1) as pa, pt.NNPrefilter(W, H, normal_tza=nrm_blob, max_memory_mb=1) as pn:
        assert beq(pa.host(albedo=a), want[0]) and beq(pn.host(normal=n), want[1])


# ---- 6 .. 8: the tracer ------------------------------------------------------------------------------------------------------------------------
W, H, SPP = 64, 48, 3


def _scene(pt, name="cornellGlass.txt"):
    """the scene with runCuda's camera, and the orbit state that camera came from"""
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=(W, H), depth=6)
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))
    return s, o


def _pass3(g):
    return U.weights_blob(X.passthrough_weights(3, (0, 1, 2), g))


def _pass9(pick):
    return U.weights_blob(X.passthrough_weights(9, pick, 1.0))


def _routed(guide, kind):
    """what a 9-input pass-through main network (g = 1, srgb = 1) gives for the guide it was fed: the guide through k_nn_input's guide
    path, the fp16 rounding, and the linear output transform"""
    x = X.aux_input_f32(guide, kind, srgb=1 if kind == X.ALBEDO else 0)       # albedo: NaN -> 0, clamp [0, 1]; normal: ..., * 0.5 + 0.5
    return X.aux_output_f32(X.passthrough(x, 1.0), X.ALBEDO, srgb=1)


def _clean(guide, kind, g, scale=1.0):
    """a pass-through prefilter network (srgb = 1 for the albedo) on a guide image, fp16 rounding points written out"""
    srgb = 1 if kind == X.ALBEDO else 0
    return X.aux_output_f32(X.passthrough(X.aux_input_f32(guide, kind, srgb, scale), g), kind, srgb, scale)


def test_the_main_network_gets_the_cleaned_guides(gpu_product):
    pt = gpu_product
    s, _ = _scene(pt)
    with pt.Tracer(s) as T, pt.NNPrefilter(W, H, _pass3(0.5), _pass3(0.5)) as pf:
        T.set_guide_bounces(2)
        T.render(1, SPP)
        g = T.gbuffer()
        for pick, kind, guide in (((3, 4, 5), X.ALBEDO, g["albedo"]), ((6, 7, 8), X.NORMAL, g["normal"])):
            with pt.NN(W, H, _pass9(pick)) as nn:
                got = T.denoise_nn(nn, SPP, prefilter=pf, prefilter_params=dict(srgb=1), srgb=1)
                raw = T.denoise_nn(nn, SPP, srgb=1)
            want, want_raw = _routed(_clean(guide, kind, 0.5), kind), _routed(guide, kind)
            assert beq(got, want), (pick, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            assert beq(raw, want_raw)                                            # (the scheme reads the plain call's guides too)
            assert (got != raw).mean() > 0.25 and got.any()
        assert pf.info()["runs"] == 1                                            # both main networks from one prefilter run


def test_tracer_prefiltered_is_the_networks_on_the_tracers_own_frames(gpu_product):
    pt = gpu_product
    s, _ = _scene(pt)
    alb_blob, nrm_blob = _blob3(1), _blob3(2, U.NARROW)
    main = U.weights_blob(U.synthetic_weights(9, 1))
    with pt.Tracer(s) as T, pt.Tracer(s) as other, pt.NN(W, H, main) as nn, pt.NNPrefilter(W, H, alb_blob, nrm_blob) as pf, \
            pt.NNPrefilter(W, H, alb_blob, nrm_blob) as fresh:
        for t in (T, other):
            t.set_guide_bounces(2)
            t.render(1, SPP)
        got = T.denoise_nn(nn, SPP, prefilter=pf)
        g = T.gbuffer()
        ca, cn = pf.read()
        fa, fn = fresh.host(g["albedo"], g["normal"])
        assert beq(ca, fa) and beq(cn, fn) and ca.any() and cn.any()
        mean = (T.read_image().reshape(H, W, 3) / np.float32(SPP)).astype(np.float32)
        assert beq(got, nn.host(mean, ca, cn)) and got.any()
        assert not beq(got, T.denoise_nn(nn, SPP))                               # (the raw guides give another frame)
        assert T.device_denoised_ptr()
        # the frame, the statistics and a following iteration are those of a tracer that never saw the call
        assert beq(T.read_image(), other.read_image()) and T.stats()["rays_per_bounce"] == other.stats()["rays_per_bounce"]
        T.render(SPP + 1, 1)
        other.render(SPP + 1, 1)
        assert beq(T.read_image(), other.read_image())


def test_the_clean_guides_are_cached_per_gbuffer(gpu_product):
    pt = gpu_product
    s, o = _scene(pt)
    alb_blob, nrm_blob = _blob3(1), _blob3(2, U.NARROW)
    main = U.weights_blob(U.synthetic_weights(9, 1))

    def fresh_result(t, **pp):
        with pt.NNPrefilter(W, H, alb_blob, nrm_blob) as fresh:
            return t.denoise_nn(nn, SPP, prefilter=fresh, prefilter_params=pp)

    with pt.Tracer(s) as T, pt.Tracer(s) as T2, pt.NN(W, H, main) as nn, pt.NNPrefilter(W, H, alb_blob, nrm_blob) as pf:
        runs = lambda: pf.info()["runs"]
        for t in (T, T2):
            t.set_guide_bounces(2)
            t.render(1, SPP)
        first = T.denoise_nn(nn, SPP, prefilter=pf)
        assert runs() == 1
        assert beq(T.denoise_nn(nn, SPP, prefilter=pf), first) and runs() == 1 and beq(first, fresh_result(T))
        s.orbit_events(o, [("left", 40.0, 10.0)])                                # a new camera
        T.set_camera(s)
        moved = T.denoise_nn(nn, SPP, prefilter=pf)
        assert runs() == 2 and beq(moved, fresh_result(T)) and not beq(moved, first)
        T.set_guide_bounces(1)
        assert beq(T.denoise_nn(nn, SPP, prefilter=pf), fresh_result(T)) and runs() == 3
        scaled = T.denoise_nn(nn, SPP, prefilter=pf, prefilter_params=dict(input_scale=0.5))
        assert runs() == 4 and beq(scaled, fresh_result(T, input_scale=0.5))
        assert beq(T.denoise_nn(nn, SPP, prefilter=pf, prefilter_params=dict(input_scale=0.5)), scaled) and runs() == 4
        assert beq(T2.denoise_nn(nn, SPP, prefilter=pf, prefilter_params=dict(input_scale=0.5)), fresh_result(T2, input_scale=0.5)) and runs() == 5
        pf.invalidate()
        assert beq(T2.denoise_nn(nn, SPP, prefilter=pf, prefilter_params=dict(input_scale=0.5)), fresh_result(T2, input_scale=0.5)) and runs() == 6
        # a run of the handle's own forgets the G-buffer as well
        g = T2.gbuffer()
        pf.host(g["albedo"], g["normal"])
        assert runs() == 7
        T2.denoise_nn(nn, SPP, prefilter=pf, prefilter_params=dict(input_scale=0.5))
        assert runs() == 8


def test_mixed_and_refused(gpu_product):
    import torch
    pt = gpu_product
    s, _ = _scene(pt)
    main3, main6 = (U.weights_blob(U.synthetic_weights(ic, 1)) for ic in (3, 6))
    with pt.Tracer(s) as T, pt.NNPrefilter(W, H, normal_tza=_pass3(0.5)) as pn:
        T.set_guide_bounces(2)
        T.render(1, SPP)
        g = T.gbuffer()
        # a handle with the normal network alone: a 9-input main network gets the raw albedo and the clean normal
        for pick, want in (((3, 4, 5), _routed(g["albedo"], X.ALBEDO)), ((6, 7, 8), _routed(_clean(g["normal"], X.NORMAL, 0.5), X.NORMAL))):
            with pt.NN(W, H, _pass9(pick)) as nn:
                assert beq(T.denoise_nn(nn, SPP, prefilter=pn, srgb=1), want), pick
        with pt.NN(W, H, main6) as nn6, pt.NN(W, H, main3) as nn3, pt.NNPrefilter(W, H, albedo_tza=_pass3(0.5)) as pa, \
                pt.NNPrefilter(W + 1, H, albedo_tza=_pass3(0.5)) as other:
            with pytest.raises(pt.PathTracerError, match="no albedo network"):
                T.denoise_nn(nn6, SPP, prefilter=pn)
            with pytest.raises(pt.PathTracerError, match="3 input channels"):
                T.denoise_nn(nn3, SPP, prefilter=pa)
            with pytest.raises(pt.PathTracerError, match="prefilter handle's size 65 x 48 differs"):
                T.denoise_nn(nn6, SPP, prefilter=other)
            with pytest.raises(pt.PathTracerError, match="hdr"):
                T.denoise_nn(nn6, SPP, prefilter=pa, prefilter_params=dict(hdr=1))
            with pytest.raises(pt.PathTracerError, match="srgb"):
                T.denoise_nn(nn6, SPP, prefilter=pa, prefilter_params=dict(srgb=2))
            with pytest.raises(pt.PathTracerError, match="spp"):
                T.denoise_nn(nn6, 0, prefilter=pa)
            with pytest.raises(pt.PathTracerError, match="prefilter_params without a prefilter"):
                T.denoise_nn(nn6, SPP, prefilter_params=dict(srgb=1))
            # a 6-input main network with the albedo network: the clean albedo, and no use of a normal network
            got = T.denoise_nn(nn6, SPP, prefilter=pa, prefilter_params=dict(srgb=1))
            mean = (T.read_image().reshape(H, W, 3) / np.float32(SPP)).astype(np.float32)
            assert beq(got, nn6.host(mean, _clean(g["albedo"], X.ALBEDO, 0.5))) and beq(pa.read(), _clean(g["albedo"], X.ALBEDO, 0.5))
            with pt.Tracer(s, tile_rows=8, tile_rank=0, tile_world=2) as tiled:
                tiled.render(1, 1)
                with pytest.raises(pt.PathTracerError, match="row tile"):
                    tiled.denoise_nn(nn6, 1, prefilter=pa)
            if torch.cuda.device_count() > 1:
                with pt.NNPrefilter(W, H, albedo_tza=_pass3(0.5), device=1) as far:
                    with pytest.raises(pt.PathTracerError, match="created on device 1"):
                        T.denoise_nn(nn6, SPP, prefilter=far)
    with pytest.raises(pt.PathTracerError, match="no weights"):
        pt.NNPrefilter(W, H)
    with pytest.raises(pt.PathTracerError, match="input channels"):
        pt.NNPrefilter(W, H, albedo_tza=main6)
    with pytest.raises(pt.PathTracerError, match="bad frame size"):
        pt.NNPrefilter(7681, 4320, albedo_tza=main3)
