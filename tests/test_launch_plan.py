"""CPU: the launch plans and the debug switches (csrc/pt_plan.hip) under AddressSanitizer and UndefinedBehaviorSanitizer.  The unit holds
no kernel and calls no hip* function, so its host pass links with a stand-alone program (tests/launch_plan_check.cpp) and runs without
a GPU: a table of plans and run cuts recorded before the plans moved there -- frames do not depend on a grid, so nothing else would
notice a slip -- and read_debug_switches with nothing set, everything set, every clamp at its edge and a short PTX_DEBUG_LANE_PRIO list.
Compiled with the flags the library's own object gets (asked of the Makefile).  And the engine reads the environment in one place."""
import os
import re
import shlex
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def test_launch_plans_and_switches_are_the_recorded_ones_under_the_sanitizers(tmp_path):
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "no hipcc: the library itself could not have been built"
    # the command the Makefile builds build/pt_plan.o with, without its "-c pt_plan.hip -o build/pt_plan.o"
    lines = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/pt_plan.o"], text=True).splitlines()
    cmds = [shlex.split(l) for l in lines if " -c pt_plan.hip " in l]
    assert len(cmds) == 1, lines
    compile_ = cmds[0][:cmds[0].index("-c")] + ["--cuda-host-only", "-g", "-I" + CSRC] + SANITIZE
    unit, prog, exe = tmp_path / "pt_plan.o", tmp_path / "launch_plan_check.o", tmp_path / "launch_plan_check"
    subprocess.check_call(compile_ + ["-c", os.path.join(CSRC, "pt_plan.hip"), "-o", str(unit)])
    subprocess.check_call(compile_ + ["-x", "hip", "-c", os.path.join(ROOT, "tests", "launch_plan_check.cpp"), "-o", str(prog)])
    subprocess.check_call([compile_[0], "-fsanitize=address,undefined", str(prog), str(unit), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "launch_plan_check: 0 failures" in r.stdout, r.stdout[-2000:]


def _function_body(text, signature):
    """the text of the function that starts with `signature`, up to the closing brace in the first column"""
    start = text.index(signature)
    return text[start:text.index("\n}\n", start) + 3]


def test_the_engine_reads_the_environment_in_one_place():
    """getenv occurs in pt_plan.hip inside read_debug_switches alone, and in pt_engine.hip only at the PTX_DEBUG_PREQUEUE_US read of
    ptx_render_strided, which says why it stays a per-call read; no other unit of the engine reads a PTX_DEBUG_* variable but
    pt_multi.cpp's PTX_DEBUG_NO_PEER."""
    plan = open(os.path.join(CSRC, "pt_plan.hip")).read()
    body = _function_body(plan, "DebugSwitches read_debug_switches() {")
    assert plan.count("getenv") == body.count("getenv") > 0
    engine = open(os.path.join(CSRC, "pt_engine.hip")).read().splitlines()
    hits = [i for i, l in enumerate(engine) if "getenv" in l]
    assert len(hits) == 1, [engine[i] for i in hits]
    assert 'getenv("PTX_DEBUG_PREQUEUE_US")' in engine[hits[0]]
    assert "tools/gpu_prequeue.py" in engine[hits[0] - 1] and engine[hits[0] - 1].lstrip().startswith("//")
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".cpp", ".h")) and name not in ("pt_plan.hip", "pt_engine.hip"):
            reads = re.findall(r'getenv\("(PTX_DEBUG_\w+)"\)', open(os.path.join(CSRC, name)).read())
            assert reads == (["PTX_DEBUG_NO_PEER"] if name == "pt_multi.cpp" else []), (name, reads)
