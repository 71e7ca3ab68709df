"""CPU: what the compiler made of the kernels (hipcc cross-compiles gfx950 without a GPU; `make resource-usage` =
-Rpass-analysis=kernel-resource-usage on pt_kernels.hip at the exact level and on pt_engine.hip).  The specialised bounce kernels are launched as eight (later bounces) and
twenty (camera bounce) workgroups per CU and compiled for eight / seven waves per SIMD: a change that pushes them over
64 / 72 registers would not fail any parity test, it would spill -- this test is where that shows.  (Round 5 tried the camera kernel
at eight waves: it fits 64 registers only with two values in scratch, and this test is why that build was not taken.)"""
import os
import shutil

import pytest

import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def remarks():
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if not hipcc:
        # (the image of this project always has it: a skip here means the environment is not the one the library is built in)
        pytest.skip("no hipcc on PATH or under /opt/rocm/bin: nothing to compile the kernels with -- register / occupancy guards NOT checked")
    return resource_usage.remarks("resource-usage")


@pytest.fixture(scope="module")
def usage(remarks):
    return resource_usage.parse_usage(remarks)


def _bounce(usage, first, mode, fast):
    tag = "k_bounceILb%dELi%dELb%dE" % (first, mode, fast)
    hits = [v for k, v in usage.items() if tag in k]
    assert len(hits) == 1, (tag, list(usage))
    return hits[0]


def test_no_kernel_of_the_path_spills(usage):
    names = [k for k in usage if "k_bounce" in k or "k_mesh" in k or "k_gather" in k]
    assert len(names) >= 14                      # 12 k_bounce variants + k_mesh + k_gather (k_move is gone: round 3)
    for k in names:
        assert usage[k]["scratch"] == 0, (k, usage[k])


def test_specialised_bounce_kernels_fit_their_waves(usage):
    # what the launch configuration relies on: enqueue_batch launches the specialised later-bounce kernel as 8 workgroups per CU = 8 waves
    # per SIMD (64 registers; the LDS side of it: 16 record rows and a 32-run window, pt_kernels.h), the camera-ray variant at 7 ...
    later, first = _bounce(usage, 0, 0, 1), _bounce(usage, 1, 0, 1)
    assert later["waves"] >= 8 and later["vgprs"] <= 64, later
    assert first["waves"] >= 7 and first["vgprs"] <= 72, first


def test_occupancy_headroom_does_not_regress(usage):
    # ... and the occupancy the kernels HAVE beyond their launch bounds (launch bounds only force a floor: a change that costs pass 2
    # two waves or k_mesh one would pass every parity test and the check above).  Floors = what DESIGN.md 5 quotes, one step below
    # the values of the round-4 build (unsplit FAST 57 / 8 waves and 65 / 7 for the camera rays, MODE 1 65-74 / 6-7, MODE 2 25-29 / 8, k_mesh 79-80 / 6).
    for first in (0, 1):
        for fast in (0, 1):
            m1, m2 = _bounce(usage, first, 1, fast), _bounce(usage, first, 2, fast)
            assert m1["waves"] >= 6 and m1["vgprs"] <= 80, (first, fast, m1)
            assert m2["waves"] >= 7 and m2["vgprs"] <= 40, (first, fast, m2)
        g = _bounce(usage, first, 0, 0)                  # the general kernel: 4 waves by its launch bounds, 128 registers
        assert g["waves"] >= 4 and g["vgprs"] <= 128, g
    for k, mesh in usage.items():
        if "k_mesh" in k:
            assert mesh["waves"] >= 6 and mesh["vgprs"] <= 84, (k, mesh)


# the kernels that are the same at every arithmetic level: the host unit's, compiled once
LEVEL_INDEPENDENT = ("k_capture_prefix", "k_capture", "k_replay_emission", "k_seed_totals", "k_gather", "k_stats", "k_pbo", "k_kat_fast_exact",
                     "k_gbuffer", "k_hold")
# the per-stage test kernels that go through the launcher table (KernelSet); k_kat_tile has two instances
TABLE_KAT = ("k_kat_geom", "k_kat_intersect", "k_kat_obj_tri", "k_kat_jittered", "k_kat_shade", "k_kat_generate", "k_kat_libm")


def _has(kernels, name, args="E"):
    """the kernels among `kernels` (mangled) named `name` in the library's anonymous namespace, as the Itanium mangling spells it: <length><name>, then
    the template arguments (I..E) and the E that closes the nested name -- so k_capture is not also k_capture_prefix"""
    # (k_hold is defined inside the extern "C" block: its symbol is the plain name)
    return [k for k in kernels if "_GLOBAL__N_1%d%s%s" % (len(name), name, args) in k or k == name]


def test_kernels_live_in_the_unit_their_level_dependence_says(remarks):
    # pt_engine.hip (compiled once, exact level) holds exactly the level-independent kernels; pt_kernels.hip (one code object per level)
    # holds none of them and exactly the kernels whose arithmetic depends on the level: a kernel added to the wrong file silently becomes
    # level-dependent, or is shipped in dead copies
    by_file = resource_usage.kernels_by_file(remarks)
    assert set(by_file) == {"pt_engine.hip", "pt_kernels.hip"}, sorted(by_file)
    engine, kernels = by_file["pt_engine.hip"], by_file["pt_kernels.hip"]
    for name in LEVEL_INDEPENDENT:
        assert len(_has(engine, name)) == 1, (name, sorted(engine))
        assert not _has(kernels, name), (name, sorted(kernels))
    assert len(engine) == len(LEVEL_INDEPENDENT), sorted(engine)
    expected = [("k_bounce", "ILb%dELi%dELb%dEE" % (first, mode, fast)) for first in (0, 1) for mode in (0, 1, 2) for fast in (0, 1)]
    expected += [(name, "ILb%dEE" % b) for name in ("k_mesh", "k_finish", "k_kat_tile") for b in (0, 1)]
    expected += [(name, "E") for name in TABLE_KAT]
    for name, args in expected:
        assert len(_has(kernels, name, args)) == 1, (name, args, sorted(kernels))
    assert len(kernels) == len(expected), sorted(kernels)
