"""CPU: the spill and occupancy guards of tests/test_build_resources.py and tests/test_build_resources_last.py on the code objects of
arithmetic levels 1 and 2 (`make resource-usage-arith1|2`, `make resource-usage-last-arith1|2`: the same recipes under the level's
flags), with the same floors.  The other levels are launched with level 0's grids -- eight workgroups per CU for the specialised later
bounce, seven waves for the camera bounce -- so a contraction or a hardware seed that costs one of those kernels a register past its
bound spills at that level alone, and no test of results would notice.  (The per-stage test kernels carry 36 bytes of scratch at every
level, level 0 included; they are not part of the guard.)"""
import os
import shutil

import pytest

import resource_usage
from test_build_resources import _bounce

LEVELS = (1, 2)


@pytest.fixture(scope="module", params=LEVELS)
def level(request):
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    return request.param


@pytest.fixture(scope="module")
def usage(level):
    return resource_usage.resource_usage("resource-usage-arith%d" % level)


@pytest.fixture(scope="module")
def usage_last(level):
    return resource_usage.resource_usage("resource-usage-last-arith%d" % level)


def test_no_kernel_of_the_path_spills(usage):
    names = [k for k in usage if "k_bounce" in k or "k_mesh" in k or "k_finish" in k]
    assert len(names) == 12 + 2 + 2, sorted(names)               # 12 k_bounce variants, two instances each of k_mesh and k_finish
    for k in names:
        assert usage[k]["scratch"] == 0, (k, usage[k])


def test_specialised_bounce_kernels_fit_their_waves(usage):
    later, first = _bounce(usage, 0, 0, 1), _bounce(usage, 1, 0, 1)
    assert later["waves"] >= 8 and later["vgprs"] <= 64, later
    assert first["waves"] >= 7 and first["vgprs"] <= 72, first


def test_occupancy_headroom_does_not_regress(usage):
    for first in (0, 1):
        for fast in (0, 1):
            m1, m2 = _bounce(usage, first, 1, fast), _bounce(usage, first, 2, fast)
            assert m1["waves"] >= 6 and m1["vgprs"] <= 80, (first, fast, m1)
            assert m2["waves"] >= 7 and m2["vgprs"] <= 40, (first, fast, m2)
        g = _bounce(usage, first, 0, 0)
        assert g["waves"] >= 4 and g["vgprs"] <= 128, g
    for k, mesh in usage.items():
        if "k_mesh" in k:
            assert mesh["waves"] >= 6 and mesh["vgprs"] <= 84, (k, mesh)


def test_the_level_holds_the_kernels_level_0_holds(usage):
    # the same list as level 0's unit (tests/test_build_resources.py): a kernel compiled out at one level would be a missing table entry
    level0 = resource_usage.kernels_by_file(resource_usage.remarks("resource-usage"))["pt_kernels.hip"]
    assert len(usage) == len(level0), (sorted(usage), sorted(level0))


def test_light_only_last_bounce(usage, usage_last):
    want = ["k_bounceILb0ELi3ELb%dEE" % fast for fast in (0, 1)]
    for tag in want:
        assert len([k for k in usage_last if tag in k]) == 1, (tag, sorted(usage_last))
    assert len(usage_last) == len(want), sorted(usage_last)
    fast = [v for k, v in usage_last.items() if "k_bounceILb0ELi3ELb1E" in k][0]
    general = [v for k, v in usage_last.items() if "k_bounceILb0ELi3ELb0E" in k][0]
    assert fast["scratch"] == 0 and general["scratch"] == 0, (fast, general)
    assert fast["waves"] >= 8 and fast["vgprs"] <= 64, fast
    assert general["waves"] >= 4 and general["vgprs"] <= 128, general
    assert not [k for k in usage if "k_bounceILb0ELi3" in k], sorted(usage)
