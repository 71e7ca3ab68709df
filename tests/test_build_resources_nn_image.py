"""CPU: what the compiler made of the image entry points' kernels (`make resource-usage-nn-image` = -Rpass-analysis=kernel-resource-usage
on pt_nn_image.hip).  The unit holds exactly k_nn_image_input, k_nn_image_output, k_nn_image_gather and k_nn_image_copy
-- the convolutions between the first two are pt_nn.hip's, launched from there -- and none has scratch or LDS: one pass over memory
each.  Resource figures only."""
import os
import shutil

import pytest

import resource_usage

KERNELS = ["k_nn_image_input", "k_nn_image_output", "k_nn_image_gather", "k_nn_image_copy"]


def _find(usage, name):
    """the one kernel of the unit's anonymous namespace with this name"""
    tag = "_GLOBAL__N_1%d%sE" % (len(name), name)
    hits = [k for k in usage if tag in k]
    assert len(hits) == 1, (name, hits, sorted(usage))
    return usage[hits[0]]


@pytest.fixture(scope="module")
def usage():
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    return resource_usage.resource_usage("resource-usage-nn-image")


def test_the_unit_holds_the_four_image_kernels_and_nothing_else(usage):
    for name in KERNELS:
        _find(usage, name)
    assert len(usage) == len(KERNELS), sorted(usage)


def test_no_image_kernel_has_scratch_or_lds(usage):
    for name in KERNELS:
        k = _find(usage, name)
        print(name, k)
        assert k["scratch"] == 0 and k["lds"] == 0, (name, k)
