"""GPU: the life of a tracer's streams and events, of the timed regions of the sc_* host entry points and of the veneer's timer.
A tracer destroyed with work traced ahead on its lane streams and nothing read, with per-kernel timing events recorded, and on a
caller's stream, which must outlive it; the next tracer made right after renders the frame of one that never traced ahead.  The sc_*
host-pointer entry points twice each in one process at sizes around one wave, one tile and one record tile, against numpy, each
leaving a positive sc_last_gpu_ms.  The veneer's pathtraceInit / pathtrace / pathtraceFree twice in one process with the module
timer around the calls (tests/veneer_timer_check.cpp).  cornell.txt at 70 x 5 (wider than one 64-pixel row segment, 350 pixels: no
multiple of the tile) and 160 x 90, depth 4.  What the owners do with handles is held without a device by test_hip_owned.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

SIZES = [(70, 5), (160, 90)]         # (W, H)
ITERS = 6                            # past one batch of 4: the second batch is being consumed and the third traced when the tracer goes
# render-ahead needs three lanes and more than one iteration per launch set (include/mi355x_pathtracer.h); asked for explicitly, so
# that it does not hang on the plan's rule for a frame this small.  cornell.txt renders with antialiasing: no first-bounce cache,
# so iteration 1 is traced ahead too.
LAYOUT = dict(batch=4, lanes=3)
_plain = {}


def _scene(pt, size):
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"), res=size, depth=4)
    s.apply_runcuda_camera()
    return s


def _plain_frame(pt, size):
    """ITERS iterations, one per call, by a tracer that never traced ahead (computed once per size)"""
    if size not in _plain:
        with pt.Tracer(_scene(pt, size), **LAYOUT) as T:
            for it in range(1, ITERS + 1):
                T.pathtrace(it)
            _plain[size] = T.read_image()
            assert T.stats()["iterations"] == ITERS and _plain[size].any()
        _plain[size].setflags(write=False)
    return _plain[size]


@pytest.mark.parametrize("timing", [False, True], ids=["ahead", "kernel_timing"])
@pytest.mark.parametrize("size", SIZES)
def test_tracer_destroyed_with_work_in_flight_and_made_again(gpu_product, size, timing):
    pt = gpu_product
    s = _scene(pt, size)
    want = _plain_frame(pt, size)

    def run(T):
        T.set_render_ahead(True)
        if timing:
            T.set_kernel_timing(True)                    # (the kev events: made as the launches need them, there at destroy)
        for it in range(1, ITERS + 1):
            T.pathtrace(it)
        # test_gpu_parity.py's check of its render-ahead cases: the loop time of a call served from a traced-ahead batch
        assert T.stats()["loop_ms_total"] > 0.0 and T.last_loop_ms() > 0.0

    A = pt.Tracer(s, **LAYOUT)
    run(A)
    A.close()                                            # nothing read: what was traced ahead is still on the lane streams
    with pt.Tracer(s, **LAYOUT) as B:
        run(B)
        if timing:
            assert sum(n for _, n in B.kernel_times().values()) > 0
        got = B.read_image()
        assert B.stats()["iterations"] == ITERS
    assert beq(got, want)


@pytest.mark.parametrize("size", SIZES)
def test_a_callers_stream_outlives_the_tracer(gpu_product, size):
    import torch
    pt = gpu_product
    st = torch.cuda.Stream()
    T = pt.Tracer(_scene(pt, size), stream_ptr=st.cuda_stream, **LAYOUT)
    assert T.stream_ptr() == st.cuda_stream
    T.set_render_ahead(True)
    for it in range(1, ITERS + 1):
        T.pathtrace(it)
    got = T.read_image()
    T.close()
    with torch.cuda.stream(st):                          # the stream is the caller's still: an op enqueued on it completes
        x = torch.arange(4096, device="cuda", dtype=torch.int64) * 3
    st.synchronize()
    assert int(x.sum().item()) == 3 * 4095 * 4096 // 2
    assert beq(got, _plain_frame(pt, size))


def _sc_sizes(sc):
    return [1, 255, 257, sc.records_tile() + 1]


@pytest.mark.parametrize("entry", ["efficient_scan", "efficient_compact", "sort_records_by_key", "radix_sort_records"])
def test_sc_host_entry_points_twice_each_leave_a_positive_gpu_time(gpu_product, entry):
    sc = gpu_product.StreamCompaction()
    rng = np.random.default_rng(11)
    for n in _sc_sizes(sc):
        for rep in range(2):
            a = rng.integers(0, 4, n).astype(np.int32)                       # zeros among them: compaction drops some
            rec = rng.integers(-2**31, 2**31, (n, 3), dtype=np.int64).astype(np.int32)
            if entry == "efficient_scan":
                assert np.array_equal(sc.efficient_scan(a), np.cumsum(a) - a), (n, rep)
            elif entry == "efficient_compact":
                assert np.array_equal(sc.efficient_compact(a), a[a != 0]), (n, rep)
            elif entry == "sort_records_by_key":
                (out,), perm, totals = sc.sort_records_by_key(a, rec, nkeys=4)
                order = np.argsort(a, kind="stable")
                assert np.array_equal(perm, order) and np.array_equal(out, rec[order]), (n, rep)
                assert np.array_equal(totals, np.bincount(a, minlength=4)), (n, rep)
            else:
                keys = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
                (out,), perm, keys_out = sc.radix_sort_records(keys, rec)
                order = np.argsort(keys, kind="stable")
                assert np.array_equal(perm, order) and np.array_equal(out, rec[order]) and np.array_equal(keys_out, keys[order]), (n, rep)
            assert sc.last_gpu_ms() > 0.0, (entry, n, rep)


def _veneer_timer(pt, tmp_path, size, *extra):
    exe = tmp_path / "veneer_timer_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "veneer_timer_check.cpp"),
                           "-L" + os.path.join(ROOT, "mygpuraytracer_amd"), "-lmi355x_pathtracer", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mygpuraytracer_amd") + ",-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe), os.path.join(ROOT, "scenes", "cornell.txt"), str(size[0]), str(size[1]), "4", str(ITERS)] + list(extra),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    ms = [float(l.split("interval ")[1]) for l in r.stdout.splitlines() if l.startswith("round ")]
    assert len(ms) == 2 and ms[0] > 0.0 and ms[1] > 0.0, r.stdout


@pytest.mark.parametrize("size", SIZES)
def test_veneer_timer_over_two_lives_of_the_module_tracer(gpu_product, tmp_path, size):
    _veneer_timer(gpu_product, tmp_path, size)


def test_veneer_timer_with_the_tracer_on_another_device_than_the_current_one(gpu_product, tmp_path):
    if gpu_product.load_library().ptx_device_count() < 2:
        pytest.skip("needs a second device")
    _veneer_timer(gpu_product, tmp_path, SIZES[1], "device=1")
