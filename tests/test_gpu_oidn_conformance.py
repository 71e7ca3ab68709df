"""GPU: OIDN's conformance cases restated against the veneer (tests/oidn_conformance_check.cpp), run once on a weight directory of
synthetic blobs: the narrow table with dec_conv0 scaled to a quarter around 0.45, so that hdr outputs stay finite.  The two RTLightmap
runs are held to the Python call's bytes."""
import os
import subprocess

import numpy as np
import pytest

import unet_ref as U
from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

NAMES = {"rt_hdr": 3, "rt_ldr": 3, "rt_hdr_alb": 6, "rt_ldr_alb": 6, "rt_hdr_alb_nrm": 9, "rt_ldr_alb_nrm": 9, "rtlightmap_hdr": 3, "rtlightmap_dir": 3}


def _blob(ic, seed):
    weights = U.synthetic_weights(ic, seed, channels=U.table(ic, *U.NARROW))
    weights["dec_conv0.weight"] = (weights["dec_conv0.weight"] * 0.25).astype(np.float32)
    weights["dec_conv0.bias"] = np.full(3, 0.45, np.float32)
    return U.weights_blob(weights)


def test_the_conformance_cases_and_the_lightmap_filters_bytes(gpu_product, tmp_path):
    pt = gpu_product
    pkg = os.path.join(ROOT, "mygpuraytracer_amd")
    exe = tmp_path / "oidn_conformance_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-DOIDN_FILTER_RTLIGHTMAP", "-o", str(exe), os.path.join(ROOT, "tests", "oidn_conformance_check.cpp"),
                           "-L" + pkg, "-lmi355x_pathtracer", "-Wl,-rpath," + pkg + ",-rpath,/opt/rocm/lib"])
    wdir = tmp_path / "weights"
    wdir.mkdir()
    blobs = {name: _blob(ic, 1 + k) for k, (name, ic) in enumerate(NAMES.items())}
    for name, blob in blobs.items():
        (wdir / (name + ".tza")).write_bytes(blob)
    w, h = 33, 17
    rgb = (np.random.default_rng(8).random((h, w, 3), dtype=np.float32) * 3 - 0.5).astype(np.float32)
    rgb[2, 3] = (np.nan, np.inf, -np.inf)
    prefix = str(tmp_path / "run")
    rgb.tofile(prefix + ".lightmap_in")
    r = subprocess.run([str(exe), str(wdir), prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "oidn conformance ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-4000:])
    for name, directional in (("rtlightmap_hdr", False), ("rtlightmap_dir", True)):
        got = np.fromfile(prefix + (".lightmap_dir" if directional else ".lightmap_hdr"), np.float32).reshape(h, w, 3)
        want = np.full((h, w, 3), -7.0, np.float32)
        with pt.NN(w, h, blobs[name], max_memory_mb=3000) as nn:
            nn.lightmap_host(rgb, want, directional=directional, input_scale=0.5)
        assert beq(got, want) and want.std() > 0 and np.isfinite(want).all(), name
