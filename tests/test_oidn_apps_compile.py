"""CPU: OIDN's own three programs -- apps/oidnTest.cpp, apps/oidnDenoise.cpp, apps/oidnBenchmark.cpp, with apps/utils/image_io.cpp and
common/platform.cpp that they link to -- compile as written against the veneer (csrc/oidn_api.h through csrc/oidn_compat) and link
against the product library.  They are compiled from the reference tree in place, with both filter macros defined as OIDN's CMake
defines them for its consumers; every object and program goes into tmp_path, and nothing of the reference's text is stored here.
Compile and link is the assertion: without a GPU they cannot run.  Skipped where the reference tree is absent."""
import os
import subprocess

import pytest

from conftest import ROOT

REF = "/root/reference"
PKG = os.path.join(ROOT, "mygpuraytracer_amd")
COMPAT = os.path.join(PKG, "csrc", "oidn_compat")
APPS = ["apps/oidnTest.cpp", "apps/oidnDenoise.cpp", "apps/oidnBenchmark.cpp"]
HELPERS = ["apps/utils/image_io.cpp", "common/platform.cpp"]

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(REF, f)) for f in APPS + HELPERS),
                                reason="needs the reference's apps/oidn*.cpp, apps/utils and common (dev container only)")


def _compile(rel, out_dir):
    obj = out_dir / (os.path.basename(rel)[:-4] + ".o")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DOIDN_FILTER_RT", "-DOIDN_FILTER_RTLIGHTMAP", "-I" + COMPAT, "-I" + REF,
                           "-c", os.path.join(REF, rel), "-o", str(obj)])
    return str(obj)


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    out = tmp_path_factory.mktemp("oidn_helpers")
    return [_compile(rel, out) for rel in HELPERS]


@pytest.mark.parametrize("app", APPS)
def test_the_program_compiles_and_links_against_the_library(product, tmp_path, helpers, app):
    obj = _compile(app, tmp_path)
    exe = tmp_path / os.path.basename(app)[:-4]
    subprocess.check_call(["g++", "-o", str(exe), obj] + helpers + ["-L" + PKG, "-lmi355x_pathtracer", "-Wl,-rpath," + PKG + ",-rpath,/opt/rocm/lib", "-lpthread"])
    assert os.path.exists(exe)
    # the program was compiled against our header, not the reference's: its device comes from the asking unit's inline newDevice
    names = subprocess.check_output(["nm", "-C", "--undefined-only", obj], text=True)
    assert "oidn::detail::newDevice(oidn::DeviceType, bool)" in names and "oidnNewDevice" not in names
