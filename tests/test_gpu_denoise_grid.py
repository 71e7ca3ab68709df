"""GPU: the denoiser kernels (pt_denoise.hip) against their float64 restatements over the parameter grid of tests/denoisecases.py --
spatial_radius 1 .. 3, prefilter 0 / 1, passes up to 10 (steps up to 512), every edge-stopping constant away from its default, shapes on
the 64 x 4 workgroup's edges, hit masks on its early exits -- at the suites' TOL = 1e-4 in their metric |gpu - ref| / (|ref| + 1e-3).
tests/test_denoise_grid_cpu.py has shown every case well conditioned (float32 arithmetic alone stays within TOL / 4), so a case that fails
here is a wrong kernel or a wrong restatement.  Per case also: miss pixels keep the input's bits, their variance is 0, an all-miss frame
comes back bit for bit, a second call returns the same bits.  Then, on a rendered frame, v0 at every radius and the tracer-level call
with parameters away from the defaults.

Worst device error per family on an MI355X (153 cases, each run twice; the whole file takes 3.2 s):

    plain 3.8e-6     given variance 1.8e-5     spatial estimate 2.2e-5     v0 of the rendered frame 7.8e-7 (radius 1: 4.9e-7, 2: 6.9e-7)

No case disagreed, so neither pt_denoise.hip nor a restatement changed.  Value-only mutants of pt_denoise.hip, the cases of this file
each failed (none of them failed a test of the denoise / variance / temporal suites that were there before): spatial_radius passed as 3,
22 cases and the rendered frame's radius 1 and 2; the step capped at 16, 35; prefilter read as 1, 20; epsilon replaced by 1e-4, 14;
kx formed from 5 phi_normal (the same value at the defaults), 26."""
import os

import numpy as np
import pytest

import denoisecases as D
from conftest import ROOT, beq
from variance_ref import atrous_variance, demodulated, spatial_variance

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _err(gpu, ref):
    ref = np.asarray(ref, np.float64)
    e = np.abs(np.asarray(gpu, np.float64) - ref) / (np.abs(ref) + 1e-3)
    return float(e.max()) if e.size else 0.0


def _device(pt, c, args, ids, var):
    if c.family == "plain":
        return pt.denoise_buffers(*args, **c.params), None
    return pt.denoise_buffers_variance(*args, ids=ids, variance=var, **c.params)


@pytest.mark.parametrize("family", ["plain", "given", "spatial"])
def test_grid_matches_the_restatement(gpu_product, family):
    pt = gpu_product
    cases = D.of_family(family)
    worst, failed = (0.0, None), []
    for c in cases:
        args, ids, var, rc, rv = D.reference(c)
        rgb, hit = args[0], args[4]
        got, gv = _device(pt, c, args, ids, var)
        again, av = _device(pt, c, args, ids, var)
        ec, ev = _err(got, rc), (_err(gv, rv) if gv is not None else 0.0)
        worst = max(worst, (max(ec, ev), c.id))
        why = []
        if not (ec <= TOL and ev <= TOL):
            why.append("colour %.3g, variance %.3g" % (ec, ev))
        if not beq(got[~hit], rgb[~hit]):
            why.append("a miss pixel's colour moved")
        if gv is not None and gv[~hit].any():
            why.append("variance on a miss pixel")
        if not hit.any() and not beq(got, rgb):
            why.append("the all-miss frame changed")
        if not (beq(got, again) and (gv is None or beq(gv, av))):
            why.append("the second call differs")
        if why:
            failed.append((c.id, why))
            print("FAILED %s: %s" % (c.id, "; ".join(why)))
    print("%s: %d cases, %d failed, worst error %.3g (%s)" % (family, len(cases), len(failed), worst[0], worst[1]))
    assert not failed, "%d of %d cases: %s" % (len(failed), len(cases), failed[:6])


def _scene(pt, name, res, depth=8):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s


@pytest.fixture(scope="module")
def rendered(gpu_product):
    """cornellObj.txt at 160x90, 2 spp: the tracer (left open for the module), its G-buffer and image / spp"""
    pt = gpu_product
    W, H, spp = 160, 90, 2
    with pt.Tracer(_scene(pt, "cornellObj.txt", (W, H))) as T:
        T.render(1, spp)
        g = T.gbuffer()
        rgb = (T.read_image() / np.float32(spp)).astype(np.float32).reshape(H, W, 3)
        yield T, g, rgb, spp


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_v0_of_a_rendered_frame_at_every_radius(gpu_product, rendered, radius):
    pt = gpu_product
    T, g, rgb, spp = rendered
    dp, vp = pt.default_denoise_params(), pt.default_variance_params()
    geo = dict(phi_normal=dp.phi_normal, phi_position=dp.phi_position)
    frame = T.denoise_variance(spp, spatial_radius=radius)
    var = T.variance()
    hit = g["hit"]
    col, f = demodulated(rgb, g["albedo"], hit)
    ids = np.stack([g["material"], g["geom"]], -1)
    v0 = spatial_variance(col, g["normal"], g["position"], hit, ids, radius, **geo)
    # the filter on what the device fed it: its own v0
    want, want_v = atrous_variance(col, var["input"], g["normal"], g["position"], hit, dp.passes, vp.phi_luminance, vp.epsilon,
                                   vp.prefilter, **geo)
    e_in, e_out, e_v = _err(var["input"], v0), _err(frame, want * f), _err(var["output"], want_v)
    print("radius %d: v0 %.3g, denoised %.3g, filtered variance %.3g" % (radius, e_in, e_out, e_v))
    assert hit.sum() > hit.size // 4 and (v0[hit] > 0).any()
    assert e_in <= TOL and e_out <= TOL and e_v <= TOL, (radius, e_in, e_out, e_v)
    assert not var["input"][~hit].any() and not var["output"][~hit].any()
    if radius != 3:                                      # the radius reaches the kernel: another one gives another estimate
        other = spatial_variance(col, g["normal"], g["position"], hit, ids, 3, **geo)
        assert _err(var["input"], other) > 100 * TOL


def test_tracer_path_with_other_parameters_is_the_buffers_filter(gpu_product, rendered):
    pt = gpu_product
    T, g, rgb, spp = rendered
    prm = dict(passes=8, phi_color=0.25, phi_normal=10, phi_position=0.01)
    got = T.denoise(spp, **prm)
    assert beq(got, pt.denoise_buffers(rgb, g["albedo"], g["normal"], g["position"], g["hit"], **prm))
    assert not beq(got, T.denoise(spp))
