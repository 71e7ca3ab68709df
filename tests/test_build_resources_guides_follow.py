"""CPU: what the compiler made of the followed guides' kernel (`make resource-usage-guides-follow` = -Rpass-analysis=kernel-resource-usage
on pt_guides_follow.hip, DESIGN.md 10 "Guides through mirrors and glass").  The unit holds exactly k_guides_follow; pt_engine.hip and
pt_guides.hip keep their kernels.  The chain state (throughput, record, point, t) sits in registers next to k_guides' thirteen
accumulators and a whole intersectScene: no scratch, no LDS, and the register count must leave the occupancy the launch bounds state
(a workgroup of 64 x 4 pixels, at least 4 waves per SIMD, i.e. at most 128 registers).  The figures are printed."""
import os
import re
import shutil

import pytest

import resource_usage


@pytest.fixture(scope="module")
def usage():
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    return resource_usage.resource_usage("resource-usage-guides-follow")


def test_the_unit_holds_k_guides_follow_and_nothing_else(usage):
    assert list(resource_usage.kernels_named(usage, ["k_guides_follow"])) == ["k_guides_follow"]
    assert len(usage) == 1, sorted(usage)


def test_k_guides_follow_does_not_spill_and_fits_its_launch_bounds(usage):
    k = resource_usage.kernels_named(usage, ["k_guides_follow"])["k_guides_follow"]
    src = open(os.path.join(resource_usage.ROOT, "mygpuraytracer_amd", "csrc", "pt_guides_follow.hip")).read()
    stated = re.search(r"__launch_bounds__\(PT_BX \* PT_BY, (\d+)\) void k_guides_follow\(", src)
    assert stated, "k_guides_follow states no waves per SIMD"
    waves = int(stated.group(1))
    print("k_guides_follow: %d VGPRs, %d bytes of scratch per lane, %d bytes of LDS, %d waves per SIMD (stated: %d)" %
          (k["vgprs"], k["scratch"], k["lds"], k["waves"], waves))
    assert k["scratch"] == 0 and k["lds"] == 0, k
    assert waves == 4                                   # the floor this test holds the compiler's result to: k_guides' own
    assert k["waves"] >= waves and k["vgprs"] <= 512 // waves, k


def test_the_other_guide_units_do_not_hold_it():
    for target in ("resource-usage", "resource-usage-guides"):
        usage = resource_usage.resource_usage(target)
        assert not [n for n in usage if "k_guides_follow" in n], (target, sorted(usage))
