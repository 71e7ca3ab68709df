"""CPU: the bookkeeping of the network denoiser's progress monitor (csrc/pt_nn_progress.h, host only) under the sanitizers as a
stand-alone program (tests/nn_progress_check.cpp): the unit counts for 1, 2 and 28 tiles with and without the copy-out, a report
sequence that starts at 0, rises strictly and ends at exactly 1, an enqueue that leads the reports by at most one tile, and a cancel
at every report index, after which nothing is reported and the same state runs a whole call."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "mygpuraytracer_amd", "csrc")


def test_the_header_makes_no_hip_call():
    text = open(os.path.join(CSRC, "pt_nn_progress.h")).read()
    code = "\n".join(l.split("//")[0] for l in text.splitlines())
    assert "hip" not in code and "#include <hip" not in text


def test_the_bookkeeping_is_right_and_clean_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "nn_progress_check"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "nn_progress_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert "nn_progress_check: 0 failures in " in r.stdout and int(r.stdout.split(" in ")[1].split()[0]) > 20000, r.stdout[-2000:]
