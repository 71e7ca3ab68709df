"""CPU: what the compiler made of the display transform's kernels (`make resource-usage-display` = -Rpass-analysis=kernel-resource-usage
on pt_display.hip).  The unit holds exactly k_display_blocks, k_display_meter and the four instances of k_display_map
(vector / per-pixel form, with / without the float frame); none of them has scratch, and pt_engine.hip holds none of them."""
import os
import shutil

import pytest

import resource_usage

MAP_INSTANCES = ["k_display_mapILb%dELb%dEE" % (vec, keep) for vec in (0, 1) for keep in (0, 1)]
KERNELS = ["k_display_blocks", "k_display_meter"] + MAP_INSTANCES


@pytest.fixture(scope="module")
def usage():
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    return resource_usage.resource_usage("resource-usage-display")


def test_the_unit_holds_the_three_display_kernels_and_nothing_else(usage):
    assert list(resource_usage.kernels_named(usage, KERNELS)) == KERNELS
    assert len(usage) == len(KERNELS), sorted(usage)


def test_no_display_kernel_has_scratch(usage):
    for name, k in resource_usage.kernels_named(usage, KERNELS).items():
        assert k["scratch"] == 0, (name, k)
        print(name, k)
    found = resource_usage.kernels_named(usage, KERNELS)
    assert all(found[n]["lds"] == 0 for n in MAP_INSTANCES)          # the map is one pass over memory
    assert found["k_display_blocks"]["lds"] == 16                     # one float per wave
    assert found["k_display_meter"]["lds"] == 1024 * (8 + 4)          # a double and a count per thread


def test_the_engine_unit_does_not_hold_them():
    usage = resource_usage.resource_usage("resource-usage")
    assert not [n for n in usage if "k_display" in n], sorted(usage)
