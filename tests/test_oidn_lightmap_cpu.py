"""CPU: the veneer's newer half without a device (csrc/oidn_api.h: buffers, the progress monitor's setter, Format's numbers, images of
size 0, the device's parameters, the RTLightmap filter on request).  tests/oidn_nodevice_lightmap_check.cpp is compiled once without
and once with -DOIDN_FILTER_RTLIGHTMAP and run where no device is visible; then a program is linked from both kinds of translation
unit, each way round, in which each unit gets the device it asked for.  The two compatibility headers are ours and one step long."""
import os
import subprocess

import pytest

import unet_ref as U
from conftest import ROOT

PKG = os.path.join(ROOT, "mygpuraytracer_amd")
CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(ROOT, "tests", "oidn_nodevice_lightmap_check.cpp")
LINK = ["-L" + PKG, "-lmi355x_pathtracer", "-Wl,-rpath," + PKG + ",-rpath,/opt/rocm/lib"]
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror"]


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    path = tmp_path_factory.mktemp("weights") / "net3.tza"
    path.write_bytes(U.weights_blob(U.synthetic_weights(3, 1, channels=U.table(3, *U.NARROW))))
    return str(path)


def _run(exe, weights):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    env.pop("MI355X_OIDN_WEIGHTS", None)
    r = subprocess.run([str(exe), weights], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


@pytest.mark.parametrize("asked", [False, True])
def test_the_lightmap_filter_is_offered_to_a_unit_that_asks(product, tmp_path, weights, asked):
    exe = tmp_path / "check"
    subprocess.check_call(CXX + (["-DOIDN_FILTER_RTLIGHTMAP"] if asked else []) + ["-o", str(exe), SRC] + LINK)
    assert "oidn nodevice lightmap ok (%s)" % ("asked" if asked else "not asked") in _run(exe, weights)


@pytest.mark.parametrize("main_asks", [False, True])
def test_both_kinds_of_translation_unit_in_one_program(product, tmp_path, weights, main_asks):
    """no two definitions of one name: the asking unit's newDevice lives in an inline namespace of its own"""
    flag = ["-DOIDN_FILTER_RTLIGHTMAP"]
    main_o, second_o, exe = tmp_path / "main.o", tmp_path / "second.o", tmp_path / "both"
    subprocess.check_call(CXX + (flag if main_asks else []) + ["-DWITH_SECOND_UNIT", "-c", "-o", str(main_o), SRC])
    subprocess.check_call(CXX + ([] if main_asks else flag) + ["-DSECOND_UNIT", "-c", "-o", str(second_o), SRC])
    subprocess.check_call(["g++", "-o", str(exe), str(main_o), str(second_o)] + LINK)
    assert "oidn nodevice lightmap ok" in _run(exe, weights)
    names = subprocess.check_output(["nm", "-C", str(main_o), str(second_o)], text=True)
    # the asking unit reaches the library through detail::newDevice (its own newDevice is inline), the other through the exported one
    assert " U oidn::detail::newDevice(oidn::DeviceType, bool)" in names and " U oidn::newDevice(oidn::DeviceType)" in names


def test_the_compatibility_headers_are_ours():
    for rel in ("OpenImageDenoise/oidn.hpp", "include/OpenImageDenoise/oidn.hpp"):
        text = open(os.path.join(CSRC, "oidn_compat", rel)).read()
        assert "oidn_api.h" in text or "OpenImageDenoise/oidn.hpp" in text
        assert len(text.splitlines()) <= 8 and "Intel" not in text and "Apache" not in text
    first = open(os.path.join(CSRC, "oidn_compat", "OpenImageDenoise", "oidn.hpp")).read()
    for macro in ("OIDN_NAMESPACE_BEGIN", "OIDN_NAMESPACE_END", "OIDN_NAMESPACE_USING"):
        assert "#define " + macro in first
    header = open(os.path.join(CSRC, "oidn_api.h")).read()
    assert "Not offered: the C API." in header and "Not offered: BufferRef" not in header
