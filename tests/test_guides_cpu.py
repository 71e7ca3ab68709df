"""CPU: the sampled guides' definition (tests/guides_ref.py) driven by the oracle's own camera rays and intersections, and the C ABI's
new symbols.  The GPU side of the same restatement is tests/test_gpu_guides.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, beq
from guides_ref import oracle_samples, sampled_guides, untextured_albedo


@pytest.fixture()
def O(oracle_lib):
    oracle_lib.set_libm(1)
    yield oracle_lib
    oracle_lib.set_libm(0)


def _oracle(pt, O, name, res, aa, dof, depth=8):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    s.apply_runcuda_camera()
    d = s.dump()
    O.create(d, d["textures"])
    O.set_options(aa=aa, dof=dof)
    O.pt_init()
    return d


def test_one_centre_sample_is_the_centre_gbuffer_bit_for_bit(product, O):
    W, H = 64, 48
    d = _oracle(product, O, "cornell.txt", (W, H), 0, 0)
    g = sampled_guides(oracle_samples(O, d, 1, 1))
    O.pt_generate(1)
    op = O.paths()
    oi = O.compute_intersections(op)
    hit = oi["t"] > 0
    assert hit.sum() > W * H // 4
    assert np.array_equal(g["hit"], hit) and beq(g["coverage"], hit.astype(np.float32))
    assert beq(g["t"][hit], oi["t"][hit]) and beq(g["normal"][hit], oi["normal"][hit])
    assert beq(g["material"][hit], oi["materialId"][hit]) and beq(g["geom"][hit], oi["geomId"][hit])
    assert beq(g["position"][hit], (op["origin"] + oi["t"][:, None] * op["direction"]).astype(np.float32)[hit])
    for k in ("position", "normal", "albedo", "t", "material", "geom"):
        assert not g[k][~hit].any(), k
    # the albedo: the apps variant's AOV of iteration 1 (the first hit does not depend on the depth when nothing jitters)
    O.set_apps_variant(1)
    O.set_depth(1)
    O.pt_init()
    O.iterate(1)
    assert beq(g["albedo"], O.albedo())
    O.set_apps_variant(0)


def test_the_restated_albedo_is_the_aov_of_a_jittered_iteration(product, O):
    # write_albedo from the dumped materials against the oracle's own AOV, whose camera ray carries the jitter and the lens
    d = _oracle(product, O, "cornell.txt", (48, 48), 1, 1)
    g = sampled_guides(oracle_samples(O, d, 1, 1))
    O.set_apps_variant(1)
    O.pt_init()
    O.iterate(1)
    aov = O.albedo()
    O.set_apps_variant(0)
    assert g["hit"].any() and beq(g["albedo"], aov)


def test_antialiased_samples_on_one_flat_face_keep_its_unit_normal(product, O):
    d = _oracle(product, O, "cornell.txt", (64, 64), 1, 0)
    for K in (4, 5):
        samples = list(oracle_samples(O, d, 1, K))
        g = sampled_guides(samples)
        n0 = samples[0]["normal"]
        flat = (g["hits"] == K) & ~g["mixed"]
        for s in samples:                                # every sample's normal is the first's, bit for bit: one flat face
            flat &= (s["normal"].view(np.uint32) == n0.view(np.uint32)).all(axis=1)
        assert flat.sum() > 64 * 64 // 2
        assert beq(g["coverage"][flat], np.ones(flat.sum(), np.float32))
        assert np.abs(np.linalg.norm(g["normal"][flat].astype(np.float64), axis=1) - 1.0).max() < 1e-6
        if K == 4:                                       # n + n + n + n and / 4 are exact
            assert beq(g["normal"][flat], n0[flat])
        else:                                            # four roundings of the sum and one of the division, 2^-24 each
            assert np.abs(g["normal"][flat].astype(np.float64) - n0[flat]).max() <= 5 * 2.0 ** -24
        edge = g["mixed"] & g["hit"]                      # ... and a pixel across two faces has a shorter one
        assert edge.any()
        assert (np.linalg.norm(g["normal"][edge].astype(np.float64), axis=1) < 1.0 + 1e-6).all()


def test_depth_of_field_gives_partial_coverage_and_a_coverage_weighted_albedo(product, O):
    K = 8
    d = _oracle(product, O, "cornell.txt", (64, 64), 0, 1)
    samples = list(oracle_samples(O, d, 1, K))
    g = sampled_guides(samples)
    part = (g["coverage"] > 0) & (g["coverage"] < 1)
    assert part.sum() >= 8, int(part.sum())
    assert beq(g["coverage"], (g["hits"] / np.float32(K)).astype(np.float32))
    # where every sample that hit has the first one's material albedo, the albedo is coverage x that albedo: K - 1 roundings in the sum,
    # one in each division and one in the product, 2^-24 relative each
    a0 = untextured_albedo(d, g["material"], g["geom"], g["hit"])
    same = part.copy()
    for s in samples:
        h = s["t"] > 0
        same &= ~h | (s["albedo"] == a0).all(axis=1)
    assert same.sum() >= 4, int(same.sum())
    want = g["coverage"][same, None].astype(np.float64) * a0[same]
    assert np.abs(g["albedo"][same] - want).max() <= (K + 2) * 2.0 ** -24 * np.abs(want).max()
    assert (g["albedo"][same].max(axis=1) < a0[same].max(axis=1)).all()


def test_the_c_abi_has_the_three_entry_points_and_stays_version_5(product):
    header = open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()
    for decl in (r"int ptx_set_guide_samples\(ptx_tracer \*t, int iter_first, int count\);",
                 r"int ptx_get_guide_samples\(const ptx_tracer \*t, int \*iter_first, int \*count\);",
                 r"int ptx_read_guide_coverage\(ptx_tracer \*t, float \*coverage1\);"):
        assert re.search(decl, header), decl
    assert re.search(r"#define PTX_ABI_VERSION 5\b", header)
    L = product.load_library()
    assert L.ptx_abi_version() == 5
    for name in ("ptx_set_guide_samples", "ptx_get_guide_samples", "ptx_read_guide_coverage"):
        assert getattr(L, name).restype is C.c_int, name
    # a NULL tracer is refused before any device is touched, with the entry point's name
    assert L.ptx_set_guide_samples(None, 1, 1) == 1 and b"ptx_set_guide_samples" in L.ptx_last_error()
    assert L.ptx_get_guide_samples(None, None, None) == 1 and b"ptx_get_guide_samples" in L.ptx_last_error()
    assert L.ptx_read_guide_coverage(None, None) == 1 and b"ptx_read_guide_coverage" in L.ptx_last_error()
    for method in ("set_guide_samples", "guide_samples", "guide_coverage"):
        assert callable(getattr(product.Tracer, method)), method


def test_headless_help_names_guide_samples_and_its_refusals(product):
    import subprocess
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mygpuraytracer_amd", "csrc"), "headless"])
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--guide-samples K" in r.stdout
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    for args, what in ((["--guide-samples", "4"], "--guide-samples needs --denoise or --adaptive-denoise"),
                       (["--denoise", "--guide-samples", "0"], "--guide-samples needs K >= 1"),
                       (["--denoise", "--temporal", "--guide-samples", "4"], "--guide-samples does not combine with --temporal")):
        bad = subprocess.run([exe, scene] + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and what in bad.stderr, (args, bad.stderr)
