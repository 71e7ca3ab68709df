"""CPU: the plan of the local index (csrc/pt_plan.hip, plan_local_index) under AddressSanitizer and UndefinedBehaviorSanitizer, the way
tests/test_launch_plan.py runs the launch plans: the unit's host pass linked with a stand-alone program (tests/loop_index_check.cpp), no
GPU.  N2 a power of two >= the slots, the bound of an entry equal to the allocation, the bytes-per-path rule, and the fallback to the
tail's index exactly where the predicate says."""
import os
import shlex
import shutil
import subprocess

from test_launch_plan import CSRC, ROOT, SANITIZE


def test_the_plan_of_the_local_index_under_the_sanitizers(tmp_path):
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    lines = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/pt_plan.o"], text=True).splitlines()
    cmds = [shlex.split(l) for l in lines if " -c pt_plan.hip " in l]
    assert len(cmds) == 1, lines
    compile_ = cmds[0][:cmds[0].index("-c")] + ["--cuda-host-only", "-g", "-I" + CSRC] + SANITIZE
    unit, prog, exe = tmp_path / "pt_plan.o", tmp_path / "loop_index_check.o", tmp_path / "loop_index_check"
    subprocess.check_call(compile_ + ["-c", os.path.join(CSRC, "pt_plan.hip"), "-o", str(unit)])
    subprocess.check_call(compile_ + ["-x", "hip", "-c", os.path.join(ROOT, "tests", "loop_index_check.cpp"), "-o", str(prog)])
    subprocess.check_call([compile_[0], "-fsanitize=address,undefined", str(prog), str(unit), "-o", str(exe)])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PTX_DEBUG_")}
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "loop_index_check: 0 failures" in r.stdout, r.stdout[-2000:]
