"""CPU: pt_device.h's pt_unit_rsqrt_bits -- 1 / sqrt(s) of an operand next to 1 as an integer mapping of its bits, the second normalize of a
unit vector (getPointOnRay) -- compiled for the host from the same header by a stand-alone program (tests/unit_rsqrt_check.cpp) with
-fsanitize=address,undefined and the library's own flags.  The program compares the mapping with 1.0f / sqrtf(s) on every operand of the
window, counts them (2 W + 1), and repeats the window's derivation with a fixed seed: the largest distance of dot(v, v) from 1 over
10^8 normalized random directions and the adversarial ones must be PT_UNIT_DMAX, the window twice that."""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def test_the_mapping_equals_the_two_roundings_on_the_whole_window(tmp_path):
    # the flags of the library's exact units (make -n: nothing is built), host pass only
    lines = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/pt_scene.o"], text=True).splitlines()
    cmds = [shlex.split(l) for l in lines if " -c pt_scene.hip " in l]
    assert len(cmds) == 1, lines
    assert "-ffp-contract=off" in cmds[0]
    compile_ = cmds[0][:cmds[0].index("-c")] + ["--cuda-host-only", "-g", "-I" + CSRC] + SANITIZE
    prog, exe = tmp_path / "unit_rsqrt_check.o", tmp_path / "unit_rsqrt_check"
    subprocess.check_call(compile_ + ["-x", "hip", "-c", os.path.join(ROOT, "tests", "unit_rsqrt_check.cpp"), "-o", str(prog)])
    subprocess.check_call([compile_[0], "-fsanitize=address,undefined", str(prog), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "unit_rsqrt_check: 0 failures" in r.stdout, r.stdout[-2000:]
    m = re.search(r"window: (\d+) operands checked, 0 differ", r.stdout)
    w = re.search(r"PT_UNIT_DMAX (\d+), PT_UNIT_W (\d+)", r.stdout)
    assert m and w, r.stdout
    assert int(m.group(1)) == 2 * int(w.group(2)) + 1 and int(w.group(2)) == 2 * int(w.group(1))
    assert re.search(r"(\d+) ulps over 100000000 random directions", r.stdout), r.stdout
