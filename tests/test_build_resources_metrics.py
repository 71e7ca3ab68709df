"""CPU: what the compiler made of the image metrics' kernels (`make resource-usage-metrics` = -Rpass-analysis=kernel-resource-usage on
pt_metrics.hip).  The unit holds k_metrics_prep, k_metrics_grad, k_metrics_pool, k_metrics_finish and the three instances
of k_metrics_ssim; none has scratch, and every kernel's static LDS is within 64 KiB."""
import os
import shutil

import pytest

import resource_usage

SSIM_INSTANCES = ["k_metrics_ssimILb%dELb%dEE" % (cs, full) for cs, full in ((0, 1), (1, 0), (1, 1))]
KERNELS = ["k_metrics_prep", "k_metrics_grad", "k_metrics_pool", "k_metrics_finish"] + SSIM_INSTANCES


@pytest.fixture(scope="module")
def usage():
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    return resource_usage.resource_usage("resource-usage-metrics")


def test_the_unit_holds_the_metrics_kernels_and_nothing_else(usage):
    assert sorted(resource_usage.kernels_named(usage, KERNELS)) == sorted(KERNELS)
    assert len(usage) == len(KERNELS), sorted(usage)


def test_no_metrics_kernel_has_scratch_and_lds_is_within_64_kib(usage):
    found = resource_usage.kernels_named(usage, KERNELS)
    for name, k in found.items():
        print(name, k)
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
    # the SSIM tile: two 26 x 42 aprons, five 26 x 32 filtered planes, two doubles per wave
    assert all(found[n]["lds"] == 4 * (2 * 26 * 42 + 5 * 26 * 32) + 2 * 4 * 8 for n in SSIM_INSTANCES)
    assert found["k_metrics_pool"]["lds"] == 0
