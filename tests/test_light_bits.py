"""CPU: which geoms can end a path with radiance (ptx_create's light_bits, handed out device-free by ptx_debug_light_bits).
The last bounce of a launch set follows only the rays that reach one of these geoms' boxes: a bit missing here is light missing from the
frame.  Checked on the committed scenes against the rule itself (the geom's material has emittance > 0, classifyPath's test), and -- with
the host-only preparation, pt_prepare_scene -- in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/light_bits_check.cpp), compiled with the flags the library's own object gets."""
import os
import shlex
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
# the lights of the committed scenes, by geom index (scenes/*.txt: OBJECT 0 is the ceiling light of every Cornell room)
SCENES = {"cornell.txt": 0x1, "cornellGlass.txt": 0x1, "cornellObj.txt": 0x1, "cornellSpaceship.txt": 0x1, "cornellSpaceship20k.txt": 0x1, "sphere.txt": None}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_light_bits_of_the_committed_scenes(product, name):
    s = product.Scene(os.path.join(ROOT, "scenes", name))
    d = s.dump()
    mats, gm = np.asarray(d["materials"], np.float32).reshape(-1, 11), np.asarray(d["geom_ints"])[:, 1]
    want = 0
    for g, m in enumerate(gm[:32]):
        if mats[m][10] > 0:
            want |= 1 << g
    got = product.api.debug_light_bits(mats, gm)
    assert got == want
    if SCENES[name] is not None:
        assert got == SCENES[name]


def test_light_bits_edges(product):
    mats = np.zeros((2, 11), np.float32)
    mats[0, 10] = 3.0
    assert product.api.debug_light_bits(mats, [0, 1, 2, -1, 0]) == 0x11              # material indices outside the table set no bit
    assert product.api.debug_light_bits(mats, [1] * 31 + [0, 0]) == 1 << 31           # geom 32 has no bit
    assert product.api.debug_light_bits(mats, np.zeros(0, np.int32)) == 0
    mats[0, 10] = -1.0
    assert product.api.debug_light_bits(mats, [0, 0]) == 0                            # the test is emittance > 0


def test_light_bits_are_clean_under_the_sanitizers(tmp_path):
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    # the command the Makefile builds build/pt_scene.o with, without its "-c pt_scene.hip -o build/pt_scene.o"
    lines = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/pt_scene.o"], text=True).splitlines()
    cmds = [shlex.split(l) for l in lines if " -c pt_scene.hip " in l]
    assert len(cmds) == 1, lines
    compile_ = cmds[0][:cmds[0].index("-c")] + ["--cuda-host-only", "-g", "-I" + CSRC] + SANITIZE
    unit, prog, exe = tmp_path / "pt_scene.o", tmp_path / "light_bits_check.o", tmp_path / "light_bits_check"
    subprocess.check_call(compile_ + ["-c", os.path.join(CSRC, "pt_scene.hip"), "-o", str(unit)])
    subprocess.check_call(compile_ + ["-x", "hip", "-c", os.path.join(ROOT, "tests", "light_bits_check.cpp"), "-o", str(prog)])
    subprocess.check_call([compile_[0], "-fsanitize=address,undefined", str(prog), str(unit), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "light_bits_check: 0 failures" in r.stdout, r.stdout[-2000:]
