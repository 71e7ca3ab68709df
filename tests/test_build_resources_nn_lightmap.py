"""CPU: what the compiler made of the lightmap filter's kernels (`make resource-usage-nn-lightmap` = -Rpass-analysis=kernel-resource-usage
on pt_nn_lightmap.hip).  The unit holds exactly k_nn_lightmap_input and k_nn_lightmap_output -- the convolutions between
them are pt_nn.hip's, the gather and the copy-out pt_nn_image.hip's, launched from there -- and neither has scratch or LDS: one pass
over memory each.  Resource figures only."""
import os
import shutil

import pytest

import resource_usage

KERNELS = ["k_nn_lightmap_input", "k_nn_lightmap_output"]


def _find(usage, name):
    """the one kernel of the unit's anonymous namespace with this name"""
    tag = "_GLOBAL__N_1%d%sE" % (len(name), name)
    hits = [k for k in usage if tag in k]
    assert len(hits) == 1, (name, hits, sorted(usage))
    return usage[hits[0]]


@pytest.fixture(scope="module")
def usage():
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    return resource_usage.resource_usage("resource-usage-nn-lightmap")


def test_the_unit_holds_the_two_lightmap_kernels_and_nothing_else(usage):
    for name in KERNELS:
        _find(usage, name)
    assert len(usage) == len(KERNELS), sorted(usage)


def test_no_lightmap_kernel_has_scratch_or_lds(usage):
    for name in KERNELS:
        k = _find(usage, name)
        print(name, k)
        assert k["scratch"] == 0 and k["lds"] == 0, (name, k)
