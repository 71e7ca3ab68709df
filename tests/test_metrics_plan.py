"""CPU: the image metrics' host-only arithmetic (csrc/pt_metrics.h: scale sizes, buffer sizes, job layout, constants) in a stand-alone
program (tests/metrics_plan_check.cpp) built with -fsanitize=address,undefined, as tests/test_launch_plan.py builds its own."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def test_metrics_plan_under_the_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc: the library itself could not have been built"
    exe = tmp_path / "metrics_plan_check"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Wno-unused-function", "-I" + CSRC, "-x", "hip"] + SANITIZE +
                          [os.path.join(ROOT, "tests", "metrics_plan_check.cpp"), "-fsanitize=address,undefined", "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "metrics_plan_check: 0 failures" in r.stdout, r.stdout[-2000:]
