"""bench.py's command line: the plain run (headline figure only), --full, --dump-outputs.

CPU: the options exist, bad step counts are refused, the output writer's dtypes and size limit.
GPU: a plain run prints the headline line and nothing beyond it, --steps sets the timed steps, and --dump-outputs writes the same
arrays on every run -- the frame a fresh tracer gives for the same iterations, bit for bit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
sys.path.insert(0, ROOT)


def test_bench_help_names_full_and_dump_outputs():
    out = subprocess.run([sys.executable, BENCH, "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_bad_step_counts(args):
    out = subprocess.run([sys.executable, BENCH] + args, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps" in out.stderr


def test_write_outputs_dtypes_and_limit(tmp_path, monkeypatch):
    import bench
    img = np.arange(24, dtype=np.float32).reshape(2, 4, 3)
    counts = np.array([8, 5, 2], np.int64)
    paths = bench.write_outputs(str(tmp_path / "o"), dict(image=img, rays_per_bounce=counts))
    assert sorted(os.path.basename(p) for p in paths) == ["image.npy", "rays_per_bounce.npy"]
    a, b = np.load(tmp_path / "o" / "image.npy"), np.load(tmp_path / "o" / "rays_per_bounce.npy")
    assert a.dtype == np.float32 and np.array_equal(a, img)
    assert b.dtype == np.float64 and b.tolist() == [8.0, 5.0, 2.0]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", img.nbytes + counts.nbytes - 1)
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / "p"), dict(image=img, rays_per_bounce=counts))
    assert not (tmp_path / "p").exists()


def _plain_run(outdir, steps, warmup):
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(outdir)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(gpu_product, tmp_path):
    import bench
    pt = gpu_product
    steps, warmup = 3, 2
    W, H = bench.RES
    lines = [_plain_run(tmp_path / ("run%d" % k), steps, warmup) for k in (1, 2)]
    for line in lines:
        assert line["metric"] == "Mrays/s" and line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["steps"] == steps and line["warmup"] == warmup and line["n_gpus"] == 1
        assert line["ms_per_step"] > 0 and line["value"] > 0
        assert abs(line["config"]["timed_region_ms"] - line["ms_per_step"] * steps) < 1e-6 * line["config"]["timed_region_ms"] + 1e-9
        for leg in ("roofline", "cpu_baseline", "long_run", "c5", "arith_levels", "dropin_per_call", "stream_compaction"):
            assert leg not in line, leg
    imgs = [np.load(tmp_path / ("run%d" % k) / "image.npy") for k in (1, 2)]
    rpbs = [np.load(tmp_path / ("run%d" % k) / "rays_per_bounce.npy") for k in (1, 2)]
    assert imgs[0].dtype == np.float32 and imgs[0].shape == (H, W, 3)
    assert rpbs[0].dtype == np.float64 and rpbs[0].shape == (bench.DEPTH,)
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32)) and np.array_equal(rpbs[0], rpbs[1])
    assert rpbs[0][0] == W * H and (np.diff(rpbs[0]) <= 0).all()          # the last step: one primary ray per pixel, fewer each bounce
    # the timed iterations (warmup + 1 .. warmup + steps) traced by a fresh tracer into a fresh frame: the same bits
    s = pt.Scene(os.path.join(ROOT, "scenes", bench.SCENE), res=bench.RES, depth=bench.DEPTH)
    s.apply_runcuda_camera()
    with pt.Tracer(s, device=0) as T:
        T.render(warmup + 1, steps)
        T.synchronize()
        img = T.read_image()
        assert T.stats()["rays_per_bounce"] == rpbs[0].astype(np.int64).tolist()
    assert np.array_equal(img.reshape(H, W, 3).view(np.uint32), imgs[0].view(np.uint32))
