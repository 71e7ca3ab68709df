"""CPU: scene preparation (csrc/pt_scene.hip, pt_prepare_scene) under AddressSanitizer and UndefinedBehaviorSanitizer.  The unit holds no
kernel and calls no hip* function, so its host pass links with a stand-alone program (tests/scene_prep_check.cpp) and runs without a
GPU: scenes built in code -- the small-mesh path, a mesh with a BVH, and the edges (nothing, 33 geoms, an OBJ geom without faces, a
two-channel texture, the LDS limit stepped down to the refusal, each PTX_DEBUG_* switch of the phase) -- with the table lengths, the
staged blob against its six parts, the record masks' runs, the stack bound and the boxes asserted in the program.  Compiled with the
flags the library's own object gets (asked of the Makefile), since the tabulated normals depend on them."""
import os
import shlex
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def test_scene_preparation_is_clean_under_the_sanitizers(tmp_path):
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    # the command the Makefile builds build/pt_scene.o with, without its "-c pt_scene.hip -o build/pt_scene.o"
    lines = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/pt_scene.o"], text=True).splitlines()
    cmds = [shlex.split(l) for l in lines if " -c pt_scene.hip " in l]
    assert len(cmds) == 1, lines
    compile_ = cmds[0][:cmds[0].index("-c")] + ["--cuda-host-only", "-g", "-I" + CSRC] + SANITIZE
    unit, prog, exe = tmp_path / "pt_scene.o", tmp_path / "scene_prep_check.o", tmp_path / "scene_prep_check"
    subprocess.check_call(compile_ + ["-c", os.path.join(CSRC, "pt_scene.hip"), "-o", str(unit)])
    subprocess.check_call(compile_ + ["-x", "hip", "-c", os.path.join(ROOT, "tests", "scene_prep_check.cpp"), "-o", str(prog)])
    subprocess.check_call([compile_[0], "-fsanitize=address,undefined", str(prog), str(unit), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "scene_prep_check: 0 failures" in r.stdout, r.stdout[-2000:]
