"""CPU: the followed guides' restatement (tests/guide_bounces_ref.py) against geometry it can know -- a face-on mirror images the wall
behind the camera isometrically, a ray through a glass sphere's centre leaves undeviated, two facing mirrors alternate, a mirror that
reflects out of the box keeps its own record -- the share of pixels the GPU grid would have to leave out (none), the C ABI's new
symbols, the driver's option and the C++ veneer's switch.  The GPU side of the same restatement is tests/test_gpu_guide_bounces.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, beq
from cpulibs import PATH_DTYPE
from guide_bounces_ref import SCENE_BASE, effective_bounces, follow, followed, followed_samples, mesh_mirror, write_scene
from guides_ref import oracle_samples, sampled_guides

W, H = 97, 61


@pytest.fixture()
def O(oracle_lib):
    oracle_lib.set_libm(1)
    yield oracle_lib
    oracle_lib.set_libm(0)


def _oracle(pt, O, tmp_path, name, res=(W, H), depth=8, aa=0, dof=0):
    path, names = write_scene(tmp_path, name, res, depth)
    s = pt.Scene(path, base_dir=SCENE_BASE)
    s.apply_runcuda_camera()
    d = s.dump()
    if name == "e":
        mesh_mirror(d, names)
    O.create(d, d["textures"])
    O.set_options(aa=aa, dof=dof)
    O.pt_init()
    return d, names


def _centre_chains(O, d, bounces):
    O.pt_generate(1)
    return follow(O, d, O.paths(), effective_bounces(d, bounces))


def test_a_face_on_mirror_shows_the_wall_behind_the_camera(product, O, tmp_path):
    d, names = _oracle(product, O, tmp_path, "a")
    first = _centre_chains(O, d, 0)
    r = _centre_chains(O, d, 1)
    fol = first["hit"] & followed(d, first["material"], first["geom"])
    assert fol.sum() > W * H // 20 and np.array_equal(fol, first["geom"] == names["mirror"])
    assert np.array_equal(r["continuations"] == 1, fol)
    # every followed pixel's record lies on the wall behind the camera (its inner face: z = 5 - .005), and names it
    assert (r["geom"][fol] == names["front"]).all() and (r["material"][fol] == d["geom_ints"][names["front"]][1]).all()
    assert np.abs(r["point"][fol, 2] - 4.995).max() < 1e-4
    assert np.abs(r["normal"][fol] - np.float32([0, 0, -1])).max() < 1e-6
    # t = the two segments' lengths summed, in that order, in fp32
    assert beq(r["t"][fol], (first["t"][fol] + r["seg_t"][fol]).astype(np.float32))
    cam = d["cam_floats"][0:3].astype(np.float64)
    mirror_point = first["point"][fol].astype(np.float64)
    geometric = np.linalg.norm(mirror_point - cam, axis=1) + np.linalg.norm(r["point"][fol] - mirror_point, axis=1)
    assert np.abs(r["t"][fol] - geometric).max() < 0.011      # (the continued ray starts .01 off the mirror)
    # a plane mirror is an isometry: the images of two wall points are as far apart as the points' own mirror images, i.e. the
    # recorded points reflected in the mirror's plane z = -1.75 lie on the camera rays, prolonged
    # (the restart .01 off the mirror moves a point by at most .01 tan(angle of incidence) < .005)
    p = r["point"][fol].astype(np.float64)
    dirs = first["direction"][fol].astype(np.float64)
    image = cam + dirs * ((2 * -1.75 - 4.995 - cam[2]) / dirs[:, 2])[:, None]      # where the camera rays meet the wall's mirror image
    assert np.abs(image[:, :2] - p[:, :2]).max() < 5e-3
    i, j = 0, fol.sum() - 1
    assert np.linalg.norm(p[i] - p[j]) > 3 and abs(np.linalg.norm(p[i] - p[j]) - np.linalg.norm(image[i] - image[j])) < 1e-2
    # the albedo is T x the wall's colour, T = the mirror's specular colour (exponent 0: pow(x, 0) = 1)
    assert beq(r["T"][fol], np.tile(np.float32([.98, .98, .98]), (fol.sum(), 1)))
    # the pixels that are not followed keep their record bit for bit
    for k in ("point", "t", "normal", "material", "geom", "T", "hit"):
        assert beq(r[k][~fol], first[k][~fol]), k


def test_b_a_ray_through_the_glass_spheres_centre_leaves_undeviated(product, O, tmp_path):
    d, names = _oracle(product, O, tmp_path, "b")
    p = np.zeros(1, PATH_DTYPE)
    p["origin"], p["direction"], p["color"], p["remainingBounces"] = (0, 5, 10.5), (0, 0, -1), 1, 8
    r = follow(O, d, p, 7)
    assert r["continuations"][0] == 2 and r["geom"][0] == names["wall_green"]
    assert np.abs(r["direction"][0] - np.float32([0, 0, -1])).max() < 1e-6
    assert np.abs(r["point"][0] - np.float32([0, 5, -4.995])).max() < 1e-4
    assert abs(float(r["t"][0]) - (10.5 + 4.995)) < 0.03          # (two restarts of .01, each along the ray)
    assert beq(r["T"][0], (np.float32([.85, .85, .98]) * np.float32([.85, .85, .98])).astype(np.float32))
    one = follow(O, d, p, 1)                                     # the budget runs out inside: the record is the sphere's far side
    assert one["continuations"][0] == 1 and one["geom"][0] == names["glass"] and abs(float(one["point"][0, 2]) - 1.5) < 1e-3
    # the whole frame: the sphere's pixels see the two-colour wall (or the box) through it, the seam included
    chains = _centre_chains(O, d, 8)
    first = _centre_chains(O, d, 0)
    glass = first["geom"] == names["glass"]
    assert glass.sum() > W * H // 20
    seen = set(np.unique(chains["geom"][glass & chains["hit"]]).tolist())
    assert {names["wall_red"], names["wall_green"]} <= seen
    assert np.isfinite(chains["normal"]).all() and np.isfinite(chains["point"]).all()


def test_c_two_facing_mirrors_alternate(product, O, tmp_path):
    d, names = _oracle(product, O, tmp_path, "c")
    centre = (H // 2) * W + W // 2
    seen = [int(_centre_chains(O, d, b)["geom"][centre]) for b in (0, 1, 2, 3)]
    assert seen == [names["mirror_far"], names["mirror_near"], names["mirror_far"], names["mirror_near"]]
    r = _centre_chains(O, d, 8)                                  # depth 8: seven continuations, the budget ends the chain on a mirror
    assert r["continuations"][centre] == 7 and r["geom"][centre] == names["mirror_near"]
    assert r["continuations"].max() == 7
    t = [float(_centre_chains(O, d, b)["t"][centre]) for b in (0, 1, 2)]
    assert t[0] < t[1] < t[2]


def test_d_a_continued_ray_that_misses_leaves_the_mirrors_record(product, O, tmp_path):
    d, names = _oracle(product, O, tmp_path, "d")
    first = _centre_chains(O, d, 0)
    r = _centre_chains(O, d, 8)
    mirror = first["geom"] == names["mirror"]
    assert mirror.sum() > W * H // 50
    assert (r["continuations"][mirror] == 1).all()               # followed once, out of the open side
    for k in ("point", "t", "normal", "material", "geom", "T", "hit"):
        assert beq(r[k], first[k]), k


def test_e_emitters_and_meshes_are_not_followed(product, O, tmp_path):
    d, names = _oracle(product, O, tmp_path, "e")
    first = _centre_chains(O, d, 0)
    r = _centre_chains(O, d, 8)
    for role in ("emitter", "mesh"):
        on = first["geom"] == names[role]
        assert on.sum() > 30, role
        assert (r["continuations"][on] == 0).all() and beq(r["point"][on], first["point"][on]), role
    m = d["materials"]
    assert m[d["geom_ints"][names["mesh"]][1], 7] > 0 and m[d["geom_ints"][names["emitter"]][1], 7] > 0      # (both are mirrors)
    on = first["geom"] == names["mirror"]
    assert on.sum() > 30 and (r["continuations"][on] >= 1).all()


def test_f_the_throughput_is_the_reflective_branchs_factor(product, O, tmp_path):
    d, names = _oracle(product, O, tmp_path, "f")
    first = _centre_chains(O, d, 0)
    r = _centre_chains(O, d, 1)
    fol = first["geom"] == names["mirror"]
    # face-on: dot(-d, reflect(d, n)) = 2 cos^2 - 1 with cos = -d.z; T = speccolor * (.75 * that^4), within a few ulps of the fp64 value
    c = -first["direction"][fol, 2].astype(np.float64)
    want = np.float32([.9, .6, .3]).astype(np.float64)[None, :] * (0.75 * (2 * c * c - 1) ** 4)[:, None]
    assert fol.sum() > 100 and np.abs(r["T"][fol] / want - 1).max() < 1e-5
    assert len(np.unique(r["T"][fol, 0])) > 50                   # (it varies over the mirror: an exponent at work)


def test_the_grid_leaves_no_pixel_out(product, O, tmp_path):
    """every case of the GPU grid (tests/test_gpu_guide_bounces.py): the restatement's records are finite, so nothing is excluded"""
    for name in "abcdefg":
        d, names = _oracle(product, O, tmp_path, name)
        g = sampled_guides(followed_samples(O, d, 1, 1, 8))
        for k in ("normal", "position", "t", "albedo"):
            assert np.isfinite(g[k]).all(), (name, k)
        if name == "g":
            g0 = sampled_guides(oracle_samples(O, d, 1, 1))
            for k in g0:
                assert beq(g[k], g0[k]), k
    for name in "ab":
        d, names = _oracle(product, O, tmp_path, name, aa=1, dof=1)
        g = sampled_guides(followed_samples(O, d, 2, 3, 8))
        for k in ("normal", "position", "t", "albedo"):
            assert np.isfinite(g[k]).all(), (name, k)


def test_bounces_zero_is_the_sampled_guides_restatement(product, O, tmp_path):
    d, names = _oracle(product, O, tmp_path, "b", aa=1, dof=1)
    g0 = sampled_guides(oracle_samples(O, d, 2, 3))
    g = sampled_guides(followed_samples(O, d, 2, 3, 0))
    for k in g0:
        assert beq(g[k], g0[k]), k
    g8 = sampled_guides(followed_samples(O, d, 2, 3, 8))
    keep = ~(g0["hit"] & followed(d, g0["material"], g0["geom"])) & ~g0["mixed"]
    glass = g0["geom"] == names["glass"]
    assert keep.any() and not beq(g8["position"][glass & g0["hit"]], g0["position"][glass & g0["hit"]])


def test_the_c_abi_has_the_two_entry_points(product):
    header = open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()
    for decl in (r"int ptx_set_guide_bounces\(ptx_tracer \*t, int bounces\);",
                 r"int ptx_get_guide_bounces\(const ptx_tracer \*t, int \*bounces\);"):
        assert re.search(decl, header), decl
    L = product.load_library()
    for name in ("ptx_set_guide_bounces", "ptx_get_guide_bounces"):
        assert getattr(L, name).restype is C.c_int, name
    # a NULL tracer is refused before any device is touched, with the entry point's name
    assert L.ptx_set_guide_bounces(None, 1) == 1 and b"ptx_set_guide_bounces" in L.ptx_last_error()
    assert L.ptx_get_guide_bounces(None, None) == 1 and b"ptx_get_guide_bounces" in L.ptx_last_error()
    for method in ("set_guide_bounces", "guide_bounces"):
        assert callable(getattr(product.Tracer, method)), method


def test_headless_help_names_guide_bounces_and_its_refusals(product):
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mygpuraytracer_amd", "csrc"), "headless"])
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--guide-bounces B" in r.stdout
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    for args, what in ((["--guide-bounces", "4"], "--guide-bounces needs --denoise or --adaptive-denoise"),
                       (["--denoise", "--guide-bounces", "0"], "--guide-bounces needs 1 <= B <= 64"),
                       (["--denoise", "--guide-bounces", "65"], "--guide-bounces needs 1 <= B <= 64"),
                       (["--denoise", "--temporal", "--guide-bounces", "4"], "--guide-bounces does not combine with --temporal")):
        bad = subprocess.run([exe, scene] + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and what in bad.stderr, (args, bad.stderr)


def test_cpp_veneer_guide_bounces_switch(product, tmp_path):
    """tests/guide_bounces_veneer_check.cpp: host only -- the switch, its default and the C ABI's refusals through the veneer's header"""
    exe = tmp_path / "guide_bounces_veneer_check"
    lib = os.path.join(ROOT, "mygpuraytracer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "guide_bounces_veneer_check.cpp"), "-L" + lib, "-lmi355x_pathtracer",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib + ",-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([str(exe)], text=True, timeout=60)
    assert "guide bounces veneer ok" in out
