"""CPU: the network denoiser's image descriptors (csrc/pt_nn_image.h, "images" in include/mi355x_pathtracer.h) and the OIDN veneer
(csrc/oidn_api.h) without a device: the library's verdict on a descriptor against the restated rules (tests/nn_image_ref.py), one case
per rule with the message naming it; the refusals of ptx_nn_denoise_images_host that come before any device call; the same in a
process with no device visible; the descriptor arithmetic and the veneer's weight table under the sanitizers as a stand-alone program
(tests/nn_image_check.cpp); the reference's CPUdenoise() compiled as written against the veneer; the veneer where there is no device."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import nn_image_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
PKG = os.path.join(ROOT, "mygpuraytracer_amd")
W, H = 7, 5


def _raises(pt, match, fn, *a, **kw):
    with pytest.raises(pt.PathTracerError, match=match):
        fn(*a, **kw)


def check_descriptors(pt):
    """accepted: packed float and half, float4 and half4 views, a row pitch, an offset; refused: each rule, named"""
    f4, h4 = np.zeros((H, W + 3, 4), np.float32), np.zeros((H, W + 3, 4), np.float16)
    for a in (np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float16), f4[:, :W, :3], h4[:, :W, :3], f4[:, 2:2 + W, 1:], h4[1:, 3:, 1:]):
        w, h = a.shape[1], a.shape[0]
        pt.debug_nn_image_problem(w, h, a)
        pt.debug_nn_image_problem(w, h, a, is_output=True)
    base = f4.ctypes.data
    img = lambda fmt=1, off=0, ps=0, rs=0: pt.nn_image_of(base, format=fmt, byte_offset=off, pixel_stride=ps, row_stride=rs)
    pt.debug_nn_image_problem(W, H, img())                                   # the defaults: 12 and W * 12
    pt.debug_nn_image_problem(W, H, img(2, off=6, ps=8, rs=8 * (W + 2)))
    bad = pt.NNImage(ctypes.c_void_p(base), 3, 0, 0, 0)
    _raises(pt, "the input image: unknown format 3", pt.debug_nn_image_problem, W, H, bad)
    _raises(pt, "the output image: a pixel stride of 8 bytes is below the pixel's size of 12", pt.debug_nn_image_problem, W, H, img(ps=8), True)
    _raises(pt, "a pixel stride of 4 bytes is below the pixel's size of 6", pt.debug_nn_image_problem, W, H, img(2, ps=4))
    _raises(pt, "a row stride of 108 bytes is below width \\* pixel stride = 112", pt.debug_nn_image_problem, W, H, img(ps=16, rs=108))
    _raises(pt, "a row stride of 120 bytes is not a multiple of the pixel stride of 16", pt.debug_nn_image_problem, W, H, img(ps=16, rs=120))
    _raises(pt, "ptr \\+ byte_offset is not a multiple of the channel size of 4 bytes \\(the device needs aligned channels\\)",
            pt.debug_nn_image_problem, W, H, img(off=2))
    _raises(pt, "the pixel stride is not a multiple of the channel size of 4", pt.debug_nn_image_problem, W, H, img(ps=14, rs=14 * W))
    _raises(pt, "the pixel stride is not a multiple of the channel size of 2", pt.debug_nn_image_problem, W, H, img(2, ps=7, rs=7 * W))
    _raises(pt, "ptr \\+ byte_offset is not a multiple of the channel size of 2", pt.debug_nn_image_problem, W, H, img(2, off=1))
    _raises(pt, "no image", pt.debug_nn_image_problem, W, H, pt.NNImage(None, 1, 0, 0, 0))
    _raises(pt, "bad frame size", pt.debug_nn_image_problem, 0, H, img())
    # (a row stride that is a multiple of the pixel stride and of nothing else cannot exist: the pixel stride is checked first)


def check_random_descriptors(pt, count=3000):
    """the library refuses exactly what the restated rules refuse, and for the restated reason"""
    rng = np.random.default_rng(5)
    lib = pt.load_library()
    seen = {}
    for _ in range(count):
        w, h = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        fmt = int(rng.choice([1, 2, 2, 1, 3, 0]))
        size = R.SIZE.get(fmt, 4)
        jitter = lambda: int(rng.choice([0, 0, 0, 1, size // 2]))
        ps = int(rng.choice([0, 2 * size, 3 * size, 4 * size, 5 * size])) + jitter()
        rs = int(rng.choice([0, w * (ps or 3 * size), (w + 3) * (ps or 3 * size), max(0, (w - 1) * (ps or 3 * size)), w * (ps or 3 * size) + size])) + jitter()
        desc = (4096 + jitter(), fmt, int(rng.integers(0, 9)) * size + jitter(), ps, rs)
        want = R.problem(desc, w, h)
        rc = lib.ptx_debug_nn_image_problem(w, h, ctypes.byref(pt.NNImage(*desc)), 0)
        msg = lib.ptx_last_error().decode()
        assert (rc == 0) == (want is None) and (want is None or (rc == 1 and want in msg)), (desc, w, h, want, rc, msg)
        seen[want] = seen.get(want, 0) + 1
    assert set(seen) == set(R.RULES) | {None} and min(seen.values()) >= count // 150, seen


def check_refusals(pt):
    """ptx_nn_denoise_images_host without a handle: the params, the role's rules and the formats are refused first, each by name"""
    a32, a16 = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float16)
    lib = pt.load_library()

    def call(color=a32, albedo=None, normal=None, output=a32, samples=1.0, role=0, **params):
        p = pt.default_nn_params(**params)
        descs = [None if a is None else (a if isinstance(a, pt.NNImage) else pt.nn_image_of(a)) for a in (color, albedo, normal, output)]
        refs = [None if d is None else ctypes.byref(d) for d in descs]
        rc = lib.ptx_nn_denoise_images_host(None, *refs, float(samples), int(role), ctypes.byref(p))
        return rc, lib.ptx_last_error().decode()

    for kw, text in ((dict(role=3), "role must be"), (dict(role=-1), "role must be"), (dict(hdr=2), "hdr must be 0 or 1"), (dict(samples=0.0), "samples"),
                     (dict(role=1, hdr=1), "the albedo role is refused with hdr != 0"), (dict(role=2, hdr=1), "the normal role is refused with hdr != 0"),
                     (dict(role=1, samples=2.0), "the albedo role is refused with samples != 1"), (dict(role=2, srgb=1), "the normal role is refused with srgb != 0"),
                     (dict(role=1, input_scale=0.0), "the albedo role needs an input_scale"),
                     (dict(albedo=a16), "mixed input formats: the albedo image"), (dict(color=a16, albedo=a16, normal=a32), "mixed input formats: the normal image"),
                     (dict(output=pt.NNImage(ctypes.c_void_p(a32.ctypes.data), 7, 0, 0, 0)), "the output image: unknown format 7"),
                     (dict(), "null handle"), (dict(color=a16, albedo=a16, output=a32), "null handle"), (dict(role=1, srgb=1), "null handle")):
        rc, msg = call(**kw)
        assert rc == 1 and text in msg and msg.startswith("ptx_nn_denoise_images_host: "), (kw, rc, msg)


def test_symbols_structs_and_the_header(product):
    from mygpuraytracer_amd import api
    lib = product.load_library()
    header = open(os.path.join(ROOT, "include", "mi355x_pathtracer.h")).read()
    assert "#define PTX_ABI_VERSION 5\n" in header and lib.ptx_abi_version() == api.ABI_VERSION == 5      # additive: the ABI stays
    for name in ("ptx_sizeof_nn_image", "ptx_nn_denoise_images_device", "ptx_nn_denoise_images_host", "ptx_debug_nn_image_problem"):
        assert hasattr(lib, name) and name + "(" in header, name
    assert lib.ptx_sizeof_nn_image() == ctypes.sizeof(api.NNImage) == 40
    assert lib.ptx_sizeof_nn_params() == 12                                                       # ptx_nn_params has no new field
    for line in ("#define PTX_NN_FORMAT_FLOAT3 1\n", "#define PTX_NN_FORMAT_HALF3 2\n", "#define PTX_NN_ROLE_COLOR 0\n", "#define PTX_NN_ROLE_ALBEDO 1\n",
                 "#define PTX_NN_ROLE_NORMAL 2\n", "} ptx_nn_image;", "the device needs aligned channels", "outside max_memory_mb"):
        assert line in header, line
    assert (api.NN_FORMAT_FLOAT3, api.NN_FORMAT_HALF3, api.NN_ROLES) == (1, 2, {"color": 0, "albedo": 1, "normal": 2})
    # nn_image_of takes the offset and the strides from the view itself
    buf = np.zeros((H, W + 5, 4), np.float16)
    v = buf[1:, 2:2 + W, 1:]
    d = api.nn_image_of(v)
    assert (d.ptr - buf.ctypes.data, d.format, d.byte_offset, d.pixel_stride, d.row_stride) == ((W + 5) * 8 + 2 * 8 + 2, 2, 0, 8, (W + 5) * 8)
    for bad in (np.zeros((H, W, 2), np.float32), np.zeros((H, W, 3), np.float64), np.zeros((H, W), np.float32), np.zeros((H, W, 6), np.float32)[..., ::2],
                np.zeros((H, W, 3), np.float32)[::-1]):
        with pytest.raises(product.PathTracerError):
            api.nn_image_of(bad)


def test_descriptors_accepted_and_refused_rule_by_rule(product):
    check_descriptors(product)


def test_random_descriptors_against_the_restated_rules(product):
    check_random_descriptors(product)


def test_the_refusals_that_come_before_any_device_call(product):
    check_refusals(product)


def test_none_of_it_touches_a_device(product):
    """the same checks in a process where no device is visible"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    code = ("import mygpuraytracer_amd as pt, test_nn_image_cpu as T\n"
            "assert pt.load_library().ptx_device_count() == 0\n"
            "T.check_descriptors(pt); T.check_random_descriptors(pt, 600); T.check_refusals(pt)\n"
            "print('no device: ok')\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "no device: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_the_descriptor_arithmetic_is_clean_under_the_sanitizers(tmp_path):
    """tests/nn_image_check.cpp with its own main, -fsanitize=address,undefined, run as a program"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "nn_image_check"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "nn_image_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "nn_image_check: 0 failures in " in r.stdout and int(r.stdout.split(" in ")[1].split()[0]) > 50000, r.stdout[-2000:]


def _link_args():
    return ["-L" + PKG, "-lmi355x_pathtracer", "-Wl,-rpath," + PKG + ",-rpath,/opt/rocm/lib"]


def test_the_veneer_without_a_device(product, tmp_path):
    """tests/oidn_nodevice_check.cpp: the device's commit leaves an error that getError returns and then clears, the error function is
    called once, a null filter's calls are InvalidArgument"""
    exe = tmp_path / "oidn_nodevice_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", str(exe), os.path.join(ROOT, "tests", "oidn_nodevice_check.cpp")] + _link_args())
    r = subprocess.run([str(exe)], env=dict(os.environ, HIP_VISIBLE_DEVICES=""), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "oidn nodevice ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


REF_MAIN = "/root/reference/apps/src/main.cpp"
REF_GLM = "/root/reference/external/include"


@pytest.mark.skipif(not (os.path.exists(REF_MAIN) and os.path.isdir(REF_GLM)), reason="needs the reference's main.cpp and vendored glm (dev container only)")
def test_veneer_compiles_main_cpp_cpudenoise(product, tmp_path):
    """The reference's errorCallback and isCancelled (apps/src/main.cpp:92-98) and CPUdenoise() (:167-219) are read from its file at
    test time (text, never stored here), wrapped with the globals they use and a Timer of the wrapper's own, and compiled and linked
    against oidn_api.h with the reference's vendored glm on the include path.  Compile and link is the assertion."""
    lines = open(REF_MAIN).read().splitlines()
    blk = lambda a, b: "\n".join(lines[a - 1:b])
    assert "void CPUdenoise()" in lines[166] and "errorCallback" in lines[91]
    src = tmp_path / "main_cpudenoise.cpp"
    src.write_text('''#include <chrono>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>
#include <glm/glm.hpp>
#include "oidn_api.h"
using namespace oidn;
struct Timer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void reset() { t0 = std::chrono::steady_clock::now(); }
    double query() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
struct RenderState { std::vector<glm::vec3> image, albedo, output; };
RenderState *renderState;
int iteration;
int width;
int height;
std::vector<glm::vec3> inputColor;
%s
%s
int main(int argc, char **argv) {
    static RenderState state;
    renderState = &state; width = 4; height = 3; iteration = 2;
    state.image.assign(12, glm::vec3(1.f)); state.albedo.assign(12, glm::vec3(0.5f)); state.output.assign(12, glm::vec3(0.f));
    if (argc > 1) oidn::setWeightsDirectory(argv[1]);      // the one line a port adds
    try { CPUdenoise(); } catch (const std::exception &e) { std::cout << "refused: " << e.what() << std::endl; return 3; }
    return 0;
}
''' % (blk(92, 98), blk(167, 219)))
    exe = tmp_path / "main_cpudenoise"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + CSRC, "-I" + REF_GLM, "-o", str(exe), str(src)] + _link_args())
    assert os.path.exists(exe)


def test_the_unit_is_built_under_the_network_units_flags():
    line = [l for l in subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/pt_nn_image.o"], text=True).splitlines() if " -c pt_nn_image.hip " in l]
    assert len(line) == 1 and " -O3 " in line[0] and "-ffp-contract=off" in line[0] and line[0].index("-O3") > line[0].index("-Os")
    unit = open(os.path.join(CSRC, "pt_nn_image.hip")).read()
    assert '#include "pt_nn_transfer.h"' in unit and "pt_nn_run_tiles(n, st, stages)" in unit
    for word in ("__shared__", "atomic"):
        assert word not in unit.split("#include <hip/hip_runtime.h>")[1], word
