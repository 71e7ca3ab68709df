"""CPU: what the compiler made of the light-only last bounce (`make resource-usage-last` = -Rpass-analysis=kernel-resource-usage on
pt_kernels_last.hip at the exact level).  The unit is pt_kernels.hip's source compiled for ONE mode of the k_bounce
template: it must hold exactly the two kernels of that mode -- anything else would be a dead copy of a kernel the level's main code
object already has -- and pt_kernels.hip must not hold them.  The specialised one is launched with the later bounces' grid, eight
workgroups per CU = eight waves per SIMD: 64 registers, no scratch."""
import os
import shutil

import pytest

import resource_usage


@pytest.fixture(scope="module")
def remarks():
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    return resource_usage.remarks("resource-usage-last")


def test_the_unit_holds_the_two_kernels_of_the_mode_and_nothing_else(remarks):
    usage = resource_usage.parse_usage(remarks)
    want = ["k_bounceILb0ELi3ELb%dEE" % fast for fast in (0, 1)]
    for tag in want:
        assert len([k for k in usage if "_GLOBAL__N_18" + tag in k]) == 1, (tag, sorted(usage))
    assert len(usage) == len(want), sorted(usage)


def test_neither_kernel_spills_and_the_specialised_one_fits_eight_waves(remarks):
    usage = resource_usage.parse_usage(remarks)
    fast = [v for k, v in usage.items() if "k_bounceILb0ELi3ELb1E" in k][0]
    general = [v for k, v in usage.items() if "k_bounceILb0ELi3ELb0E" in k][0]
    assert fast["scratch"] == 0 and general["scratch"] == 0, (fast, general)
    assert fast["waves"] >= 8 and fast["vgprs"] <= 64, fast
    assert general["waves"] >= 4 and general["vgprs"] <= 128, general      # (4 waves by its launch bounds, like the general k_bounce)


def test_the_main_unit_does_not_instantiate_the_mode():
    usage = resource_usage.resource_usage("resource-usage")
    assert not [k for k in usage if "k_bounceILb0ELi3" in k], sorted(usage)
