"""CPU: the owner of HIP events and streams (Owned, csrc/pt_handle.h) under AddressSanitizer and UndefinedBehaviorSanitizer.  The owner
is generic in the handle and in its destroy call, so a stand-alone program (tests/hip_owned_check.cpp) instantiates it with a destroyer
that only counts and makes no HIP call: an empty owner destroys nothing, a made one exactly once, a borrowed one never, the elements
of an array and of a std::vector that grows once each, the members of a struct in the reverse of their declaration.  Compiled with
the flags the library's own host objects get (asked of the Makefile)."""
import os
import shlex
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def test_owned_handles_are_destroyed_once_and_in_order_under_the_sanitizers(tmp_path):
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    # the command the Makefile builds a host unit with, without its "-c pt_plan.hip -o build/pt_plan.o"
    lines = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/pt_plan.o"], text=True).splitlines()
    cmds = [shlex.split(l) for l in lines if " -c pt_plan.hip " in l]
    assert len(cmds) == 1, lines
    compile_ = cmds[0][:cmds[0].index("-c")] + ["--cuda-host-only", "-g", "-I" + CSRC] + SANITIZE
    prog, exe = tmp_path / "hip_owned_check.o", tmp_path / "hip_owned_check"
    subprocess.check_call(compile_ + ["-x", "hip", "-c", os.path.join(ROOT, "tests", "hip_owned_check.cpp"), "-o", str(prog)])
    subprocess.check_call([compile_[0], "-fsanitize=address,undefined", str(prog), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "hip_owned_check: 0 failures" in r.stdout, r.stdout[-2000:]
