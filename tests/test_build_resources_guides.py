"""CPU: what the compiler made of the sampled guides' kernel (`make resource-usage-guides` = -Rpass-analysis=kernel-resource-usage on
pt_guides.hip).  The unit holds exactly k_guides: pt_engine.hip keeps the kernels tests/test_build_resources.py lists.
The K loop keeps thirteen accumulators in registers next to a whole intersectScene: no scratch, and the register count must leave the
occupancy its launch bounds state (a workgroup of 64 x 4 pixels, at least 4 waves per SIMD, i.e. at most 128 registers)."""
import os
import shutil

import pytest

import resource_usage


@pytest.fixture(scope="module")
def usage():
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    return resource_usage.resource_usage("resource-usage-guides")


def test_the_unit_holds_k_guides_and_nothing_else(usage):
    assert list(resource_usage.kernels_named(usage, ["k_guides"])) == ["k_guides"]
    assert len(usage) == 1, sorted(usage)


def test_k_guides_does_not_spill_and_fits_its_launch_bounds(usage):
    k = resource_usage.kernels_named(usage, ["k_guides"])["k_guides"]
    assert k["scratch"] == 0 and k["lds"] == 0, k
    src = open(os.path.join(resource_usage.ROOT, "mygpuraytracer_amd", "csrc", "pt_guides.hip")).read()
    assert "__launch_bounds__(PT_BX * PT_BY, 4)" in src      # the floor this test holds the compiler's result to
    assert k["waves"] >= 4 and k["vgprs"] <= 128, k


def test_the_engine_unit_does_not_hold_it():
    usage = resource_usage.resource_usage("resource-usage")
    assert not [n for n in usage if "k_guides" in n], sorted(usage)
