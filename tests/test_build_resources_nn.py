"""CPU: what the compiler made of the network denoiser's kernels (`make resource-usage-nn` = -Rpass-analysis=kernel-resource-usage on
pt_nn.hip).  The unit holds exactly k_nn_input, k_nn_output and the eight instances of k_nn_conv (1 .. 8 blocks of 16
output channels per workgroup); none of them has scratch, and pt_engine.hip and pt_display.hip hold none of them.  Resource figures
only."""
import os
import shutil

import pytest

import resource_usage

CONV = ["k_nn_convILi%dEE" % n for n in range(1, 9)]
PLAIN = ["k_nn_input", "k_nn_output"]


def _find(usage, name):
    """the one kernel of the unit's anonymous namespace with this name (an instance: <name>ILi<n>EE)"""
    base = name.split("ILi")[0]
    tag = "_GLOBAL__N_1%d%s" % (len(base), name if "ILi" in name else name + "E")
    hits = [k for k in usage if tag in k]
    assert len(hits) == 1, (name, hits, sorted(usage))
    return usage[hits[0]]


@pytest.fixture(scope="module")
def usage():
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    return resource_usage.resource_usage("resource-usage-nn")


def test_the_unit_holds_the_three_nn_kernels_and_nothing_else(usage):
    for name in PLAIN + CONV:
        _find(usage, name)
    assert len(usage) == len(PLAIN) + len(CONV), sorted(usage)


def test_no_nn_kernel_has_scratch(usage):
    for name in PLAIN + CONV:
        k = _find(usage, name)
        print(name, k)
        assert k["scratch"] == 0, (name, k)
    for name in PLAIN:
        assert _find(usage, name)["lds"] == 0                        # one pass over memory each
    for name in CONV:
        assert _find(usage, name)["lds"] == 18 * 18 * 32 * 2          # the 18 x 18 halo tile of one 32-channel chunk, fp16
    # the accumulators are 4 rows x NCO blocks x 4 registers: all of them fit, with room for two workgroups per SIMD's worth of waves
    assert _find(usage, CONV[-1])["vgprs"] <= 256


def test_the_engine_and_display_units_do_not_hold_them():
    for target in ("resource-usage", "resource-usage-display"):
        usage = resource_usage.resource_usage(target)
        assert not [n for n in usage if "k_nn_" in n], (target, sorted(usage))
