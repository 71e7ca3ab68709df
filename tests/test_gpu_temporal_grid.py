"""GPU: the three reprojection kernels (pt_temporal.hip: k_temporal_reproject, k_reproject_variance, k_reproject_measured) through
ptx_kat_reproject -- which stages host arrays and calls pt_temporal_camera and pt_temporal_enqueue, the production path -- against their
float64 restatements over the grid of tests/temporalcases.py: max_history 0 .. 16 on hist counts up to 40, specular_history 0 / 1,
normal_cos -1 .. 1, plane_tolerance 0 .. 0.5, spp 1 .. 7, hist states with and without V, 2 .. 9 batches; frames from 1 x 1 to 6 x 257 on
the 64 x 4 workgroup's edges; hit masks applied to either side alone; hist cameras that pan, dolly, roll, stretch one axis, are not
orthogonal, look the other way or are singular; NaN and inf in the guides.  At the suites' TOL = 1e-4 in their metric
|gpu - ref| / (|ref| + 1e-3), the pixels `near` names left out.  tests/test_temporal_grid_cpu.py has shown every case well conditioned
(float32 arithmetic alone stays within TOL / 4) and within 2 % of `near`, so a case that fails here is a wrong kernel or a wrong
restatement.  Per case also, bit for bit: pixels that inherit nothing have mix = rgb / spp, n = spp and (h, n_h) = 0; the cameras without
a projection and max_history = 0 inherit nothing anywhere; the state's normals, positions and ids are the inputs; the three variants
agree on (h, n_h), mix, D and n; a second call returns the same bits; specular pixels inherit only with specular_history.  Then the
tracer path with parameters away from the defaults, fed back through the entry point.

Worst device error per variant on an MI355X (100 cases per variant, each run twice: 600 calls that allocate and free their buffers; the
whole file takes 1.2 s):

    plain 7.0e-6     variance 2.1e-5     measured 7.0e-6     (the float32 probe on the CPU reads the same three figures)

No case disagreed and the tracer path came back bit for bit, so neither pt_temporal.hip nor a restatement changed.  Value-only
mutants of pt_temporal.hip (in bounds by construction, never committed), the cases of this file each failed per variant plain /
variance / measured, the other tests of this file it failed, and the tests of the temporal, variance and temporal-measured suites that
were there before (42 tests) it failed:

    the fminf(.., max_history) dropped      64 / 64 / 64, the tracer path      7 old (the max_history = 0 orbit, the 16-spp measured views)
    specular_history read as 0              10 / 10 / 10, the specular test    none
    normal_cos replaced by 0.9               5 /  5 /  5                        none
    plane_tolerance replaced by 0.01         8 /  8 /  8, the specular test    none
    fu and 1 - fu swapped                   64 / 64 / 64                        8 old (every comparison with the restatement)
    the id test compares the material only  59 / 59 / 59, the specular test    none
    e dropped in variant 1                   0 / 64 /  0                        2 old (the variance orbit, the pooled estimator)
    mb2's row stride pairs * 2 replaced by w 0 /  0 / 34                        3 old (97 x 61 only: the one odd width)
"""
import ctypes
import os

import numpy as np
import pytest

import temporalcases as TC
from conftest import ROOT, beq
from temporal_ref import camera_dict, specular_flags

pytestmark = pytest.mark.gpu

TOL = 1e-4
NAMES = {0: "plain", 1: "variance", 2: "measured"}


def _err(gpu, ref):
    ref = np.asarray(ref, np.float64)
    e = np.abs(np.asarray(gpu, np.float64) - ref) / (np.abs(ref) + 1e-3)
    return float(e.max()) if e.size else 0.0


_DEVICE = {}


def _device(pt, c, variant):
    """the device's answer to a case, computed twice on the first request (the second for the determinism check) and kept"""
    key = (c.id, variant)
    if key not in _DEVICE:
        args, kw = TC.api_arguments(c, TC.reference(c), variant)
        _DEVICE[key] = (pt.reproject_buffers(*args, **kw), pt.reproject_buffers(*args, **kw))
    return _DEVICE[key]


def _check(c, r, variant, got, again):
    """(largest error, the reasons the case fails)"""
    cur, hit, keep, spp = r["cur"], r["cur"]["hit"], ~r["near"], c.params["spp"]
    hn, mix, dd, xn = got["hn"], got["mix"], got["dd"], got["xn"]
    errs = dict(h=_err(hn[..., :3][keep], r["h"][keep]), nh=_err(hn[..., 3][keep], r["nh"][keep]), mix=_err(mix[keep], r["mix"][keep]),
                D=_err(dd[..., :3][keep], r["D"][keep]), n=_err(xn[..., 3][keep], r["n"][keep]))
    why = []
    V = dd[..., 3]
    if variant == 0:
        if V.any():
            why.append("a V in the plain kernel's state")
    else:
        want = r["V1"] if variant == 1 else r["V2"]
        has = keep & np.isfinite(want)
        errs["V"] = _err(V[has], want[has])
        if not (V[keep & ~np.isfinite(want)] == -1).all():
            why.append("V is not -1 where the spatial estimate is due")
        if V[~hit].any():
            why.append("V on a miss pixel")
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    if bad:
        why.append(", ".join("%s %.3g" % kv for kv in bad.items()))
    none = keep & (~hit | (r["nh"] == 0))
    if not beq(mix[none], r["c32"][none]):
        why.append("mix is not rgb / spp where nothing is inherited")
    if not (xn[..., 3][none] == spp).all():
        why.append("n is not spp where nothing is inherited")
    if hn[none].any():
        why.append("(h, n_h) is not 0 where nothing is inherited")
    if (c.camera in TC.NOTHING or c.params["max_history"] == 0) and (hn.any() or not beq(mix, r["c32"])):
        why.append("something is inherited")
    if r["poisoned"].any() and (hn[r["poisoned"]].any() or not beq(mix[r["poisoned"]], r["c32"][r["poisoned"]])):
        why.append("a poisoned pixel inherits")
    if not c.params["specular_history"] and hn[cur["material"] == 2].any():
        why.append("a specular pixel inherits")
    nh4 = np.concatenate([cur["normal"], hit[..., None].astype(np.float32)], -1)
    if not (beq(got["nh"], nh4) and beq(xn[..., :3], cur["position"]) and beq(got["ids"], np.stack([cur["material"], cur["geom"]], -1))):
        why.append("the state's normals, positions or ids are not the inputs")
    if not all(beq(got[k], again[k]) for k in got):
        why.append("the second call differs")
    return max(errs.values()), why


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_grid_matches_the_restatement(gpu_product, variant):
    pt = gpu_product
    cases = TC.of_variant(variant)
    worst, failed = (0.0, ""), []
    for c in cases:
        r = TC.reference(c)
        got, again = _device(pt, c, variant)
        e, why = _check(c, r, variant, got, again)
        worst = max(worst, (e, c.id))
        if why:
            failed.append((c.id, why))
            print("FAILED %s: %s" % (c.id, "; ".join(why)))
    print("%s: %d cases, %d failed, worst error %.3g (%s)" % (NAMES[variant], len(cases), len(failed), worst[0], worst[1]))
    assert not failed, "%d of %d cases: %s" % (len(failed), len(cases), failed[:6])


def test_the_variants_agree_bit_for_bit(gpu_product):
    """"taps, n_h, h and mix are the other kernels', bit for bit" (pt_temporal.hip): and so are the state's D and n"""
    pt = gpu_product
    failed = []
    for c in TC.CASES:
        a, b, m = (_device(pt, c, v)[0] for v in (0, 1, 2))
        for name, other in (("variance", b), ("measured", m)):
            same = (beq(a["hn"], other["hn"]) and beq(a["mix"], other["mix"]) and beq(a["dd"][..., :3], other["dd"][..., :3])
                    and beq(a["xn"], other["xn"]) and beq(a["nh"], other["nh"]) and beq(a["ids"], other["ids"]))
            if not same:
                failed.append((c.id, name))
    assert not failed, failed[:8]


def test_specular_pixels_inherit_where_the_restatement_says(gpu_product):
    pt = gpu_product
    n = 0
    for c in TC.CASES:
        if c.params["specular_history"] and c.camera in TC.CAMERAS and c.params["max_history"] > 0:
            r = TC.reference(c)
            spec = r["cur"]["hit"] & (r["cur"]["material"] == 2) & ~r["near"]
            for v in (0, 1, 2):
                got = _device(pt, c, v)[0]["hn"][..., 3]
                assert np.array_equal(got[spec] > 0, r["nh"][spec] > 0), (c.id, v)
            n += int((r["nh"][spec] > 0).sum())
    assert n > 100


def _scene(pt, name, res, depth=8):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    o = s.orbit_init()
    s.lib.ptx_orbit_apply(s.h, ctypes.byref(o))          # = apply_runcuda_camera, keeping the orbit state
    return s, o


def test_tracer_path_with_other_parameters_is_the_entry_point(gpu_product):
    """two views of cornellObj.txt at 97 x 61 through Tracer.denoise_temporal with parameters away from the defaults; the entry point, fed
    the tracer's own G-buffer and image and the first view's state rebuilt on the host, returns ptx_temporal_read's bits: the state's
    D = mix / max(albedo, 1e-3) is one IEEE division and n = spp + n_h one addition, which numpy's float32 performs as the device does"""
    pt = gpu_product
    W, H, spp0, spp = 97, 61, 4, 2                       # the first view's four samples are more than max_history
    prm = dict(max_history=3, specular_history=1, normal_cos=0.5, plane_tolerance=0.1)
    s, o = _scene(pt, "cornellObj.txt", (W, H))
    spec = specular_flags(s.dump()["materials"])
    ids = lambda g: np.stack([g["material"], g["geom"]], -1)
    with pt.Temporal(0, W, H) as tm, pt.Tracer(s) as T:
        T.render(1, spp0)
        T.denoise_temporal(tm, spp0, read=False, **prm)
        g0, r0, cam0 = T.gbuffer(), tm.read(), camera_dict(s.camera)
        assert not r0["count"].any()
        a = np.maximum(g0["albedo"].astype(np.float32), np.float32(1e-3))
        hist = dict(hit=g0["hit"], normal=g0["normal"], position=g0["position"], ids=ids(g0), V=None,
                    n=np.full((H, W), spp0, np.float32), D=np.where(g0["hit"][..., None], r0["mix"] / a, r0["mix"]).astype(np.float32))
        s.orbit_events(o, [("left", 8.0, 1.0)])
        T.set_camera(s)
        T.reset_image()
        T.render(1, spp)
        T.denoise_temporal(tm, spp, read=False, **prm)
        g1, r1 = T.gbuffer(), tm.read()
        rgb = T.read_image().reshape(H, W, 3)
        got = pt.reproject_buffers(rgb, g1["albedo"], g1["normal"], g1["position"], ids(g1), g1["hit"], spec, hist=hist, hist_camera=cam0,
                                   spp=spp, variant=0, **prm)
        assert (r1["count"] > 0).sum() > W * H // 4 and (r1["count"] == 3).any()
        assert beq(got["hn"][..., :3], r1["history"]) and beq(got["hn"][..., 3], r1["count"]) and beq(got["mix"], r1["mix"])
        other = pt.reproject_buffers(rgb, g1["albedo"], g1["normal"], g1["position"], ids(g1), g1["hit"], spec, hist=hist, hist_camera=cam0,
                                     spp=spp, variant=0)
        assert not beq(other["mix"], r1["mix"])
