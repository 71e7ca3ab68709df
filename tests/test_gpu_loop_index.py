"""GPU: the local index written inside k_bounce's tile loop ("The sort"; pt_plan.h IndexPlan).  In the unsplit bounce with
up to 64 bins a pending lane of the direct epilogue stores its word of the index at bin * N2 + (its position inside the workgroup's
chunk), and the tail's pass over the stage keys is gone; PTX_DEBUG_TAIL_INDEX keeps the chunk-compact index the tail writes.  The index
is internal -- order, RNG stream indices and so every frame are the same bits -- so every case here is held, bit for bit,

  * against the CPU oracle: frame, rays per bounce, and the sorted stream captured behind every bounce (test_gpu_parity's comparison), and
  * against the same run under PTX_DEBUG_TAIL_INDEX: frame, rays per bounce, ray total, the captured streams field by field,

with the fence counter 0 in both, and with the form each run took asserted through the plan's report (Tracer.index_plan), never through
timing.  Frames: 96 x 64 (rows shorter than a tile of 256 paths) and 300 x 130 (rows longer than a tile and no multiple of it, 153 tiles,
the last one partial); the two-word case needs 516 tiles (see there)."""
import os

import numpy as np
import pytest

from conftest import ROOT, beq
from test_gpu_parity import check_sorted_streams

pytestmark = pytest.mark.gpu

SMALL, WIDE = (96, 64), (300, 130)
SWITCH = "PTX_DEBUG_TAIL_INDEX"
FIELDS = ("pix", "idx", "mat", "px", "py", "pz", "dx", "dy", "dz", "cr", "cg", "cb", "nx", "ny", "nz")


def _scene(pt, name, res, depth):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s


def _streams(T, O, d, depth):
    """the sorted stream behind every bounce that stores one: compared with the oracle's, and returned for the comparison of the two forms"""
    check_sorted_streams(T, O, d, depth)
    out = []
    for bounce in range(min(depth - 1, 5)):
        T.reset_image()
        T.debug_capture(bounce)
        T.pathtrace(1)
        g = T.debug_stream()
        out.append({k: np.array(g[k]) for k in FIELDS})
    T.debug_capture(-1)
    return out


def _drive(T, iters, drive):
    if drive == "render":
        T.render(1, iters)
    elif drive == "per_call":              # one iteration per call
        for it in range(1, iters + 1):
            T.pathtrace(it)
    elif drive == "ahead":                 # ... served from batches traced in the background
        T.set_render_ahead(True)
        for it in range(1, iters + 1):
            T.pathtrace(it)
        T.set_render_ahead(False)
    else:                                  # "reshape": the first call fills the cached camera bounce alone, the rest read it in sets of another shape
        T.pathtrace(1)
        T.render(2, iters - 1)
    return T.read_image(), T.stats()


def both_forms(pt, O, monkeypatch, s, depth, iters=3, drive="render", env=None, tile=None, loop=True, why=0, words=None, threads=1, **opt):
    d = s.dump()
    O.set_libm(1)
    O.create(d, d["textures"])
    O.set_options(aa=opt.get("antialiasing", 1), dof=0, sort=opt.get("sort_by_material", 1), cache=opt.get("cache_first_bounce", 1))
    if tile:
        O.set_tile(*tile)
        opt = dict(opt, tile_rows=tile[0], tile_rank=tile[1], tile_world=tile[2])
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv(SWITCH, raising=False)
    try:
        O.set_threads(threads)
        O.pt_init()
        for it in range(1, iters + 1):
            O.iterate(it)
        want, counts = O.image().copy(), O.live_counts().tolist()
        # (an iteration that takes the camera bounce from the first-bounce cache traces no camera ray: the tracer counts none for bounce 0)
        b0 = 1 if (not opt.get("antialiasing", 1) and opt.get("cache_first_bounce", 1) and iters > 1) else 0
        runs = []
        for tail in (False, True):
            if tail:
                monkeypatch.setenv(SWITCH, "1")
            with pt.Tracer(s, **opt) as T:
                plan = T.index_plan()
                img, st = _drive(T, iters, drive)
            O.pt_init()
            with pt.Tracer(s, **opt) as T:
                streams = _streams(T, O, d, depth)
                fenced = T.stats()["fenced"]
            print("tail" if tail else "default", plan, st["rays_per_bounce"][:depth], "fenced", st["fenced"], fenced)
            assert st["fenced"] == 0 and fenced == 0, tail
            assert beq(img, want), "against the oracle, %s" % ("the tail's index" if tail else "the default")
            assert st["rays_per_bounce"][b0: len(counts)] == counts[b0:], tail
            runs.append((plan, img, st, streams))
        (plan, img, st, streams), (plan0, img0, st0, streams0) = runs
        # which code ran: the report of the plan.  Under the switch always the tail; without it the bin-major index exactly where expected,
        # and otherwise the SAME plan as under the switch but for the reason.
        assert not plan0["loop"] and plan0["why"] == 1, plan0
        assert plan["loop"] == loop and plan["why"] == why, plan
        if loop:
            assert plan["entries"] == plan["seg_words"] // plan["words"] and (1 << plan["n2_log2"]) >= plan["slots"] > (1 << plan["n2_log2"]) // 2
            if words:
                assert plan["words"] == words, plan
        else:
            assert {k: v for k, v in plan.items() if k != "why"} == {k: v for k, v in plan0.items() if k != "why"}
        assert beq(img, img0)
        assert list(st["rays_per_bounce"]) == list(st0["rays_per_bounce"]) and st["rays_total"] == st0["rays_total"]
        assert len(streams) == len(streams0)
        for b, (g, g0) in enumerate(zip(streams, streams0)):
            for k in FIELDS:
                assert beq(g[k], g0[k]), (b, k)
        return img, st
    finally:
        monkeypatch.delenv(SWITCH, raising=False)
        for k in (env or {}):
            monkeypatch.delenv(k, raising=False)
        if tile:
            O.set_tile(0, 0, 1)
        O.set_threads(1)
        O.set_libm(0)


@pytest.mark.parametrize("res", [SMALL, WIDE], ids=lambda r: "%dx%d" % r)
@pytest.mark.parametrize("depth", [2, 3, 8])
def test_depths(gpu_product, oracle_lib, monkeypatch, res, depth):
    """Cornell with its mesh.  Depth 2: the writer is the camera bounce and the reader the light-only last bounce; 3: one later bounce
    writes and reads; 8: the bench's shape."""
    img, _ = both_forms(gpu_product, oracle_lib, monkeypatch, _scene(gpu_product, "cornellObj.txt", res, depth), depth)
    assert img.any()


@pytest.mark.parametrize("res", [SMALL, WIDE], ids=lambda r: "%dx%d" % r)
def test_sort_off_is_one_bin(gpu_product, oracle_lib, monkeypatch, res):
    both_forms(gpu_product, oracle_lib, monkeypatch, _scene(gpu_product, "cornellObj.txt", res, 4), 4, sort_by_material=0)


@pytest.mark.parametrize("drive,iters,opt", [("per_call", 3, {}), ("render", 5, dict(batch=2)), ("ahead", 7, dict(batch=2))],
                         ids=["one_per_call", "two_sets_in_flight", "render_ahead"])
def test_launch_sets(gpu_product, oracle_lib, monkeypatch, drive, iters, opt):
    """one iteration per call; five iterations as launch sets of two on lanes of their own (each lane its own segments of the index);
    the same sets traced ahead of per-call requests (their grids keep two slots per CU free: another chunk size)"""
    both_forms(gpu_product, oracle_lib, monkeypatch, _scene(gpu_product, "cornellObj.txt", WIDE, 4), 4, iters=iters, drive=drive, **opt)


@pytest.mark.parametrize("switch", ["PTX_DEBUG_NO_FAST", "PTX_DEBUG_NO_LAST"])
def test_general_kernel_and_full_last_bounce(gpu_product, oracle_lib, monkeypatch, switch):
    """PTX_DEBUG_NO_FAST: the general kernel writes and reads the index; PTX_DEBUG_NO_LAST: the last bounce is a full bounce that reads it"""
    both_forms(gpu_product, oracle_lib, monkeypatch, _scene(gpu_product, "cornellObj.txt", WIDE, 4), 4, env={switch: "1"})


def test_two_word_form_by_chunks_of_more_than_128_tiles(gpu_product, oracle_lib, monkeypatch):
    """The grid switches give a launch as few workgroups as they can -- one per CU over the launch's segments, and a set holds 64
    iterations at most: four workgroups per segment on 256 CUs -- so a chunk passes 128 tiles from 513 tiles on: 520 x 254 is 516.  One
    lane, so that the 64 iterations are ONE set.  Depth 3: the camera bounce and a later bounce write two words, a later bounce and the last read them."""
    s = _scene(gpu_product, "cornellObj.txt", (520, 254), 3)
    both_forms(gpu_product, oracle_lib, monkeypatch, s, 3, iters=64, env=dict(PTX_DEBUG_TOTAL_WG_PER_CU="1"), words=2, threads=16, lanes=1, batch=64)


def test_two_word_form_by_its_switch(gpu_product, oracle_lib, monkeypatch):
    both_forms(gpu_product, oracle_lib, monkeypatch, _scene(gpu_product, "cornellObj.txt", WIDE, 4), 4, env=dict(PTX_DEBUG_NO_IDX16="1"), words=2)


def test_row_tile_split(gpu_product, oracle_lib, monkeypatch):
    """rank 3 of 8, bands of 8 rows: the slots are those of the pixels the device owns (the oracle's tile carries slots as well)"""
    both_forms(gpu_product, oracle_lib, monkeypatch, _scene(gpu_product, "cornellObj.txt", WIDE, 4), 4, tile=(8, 3, 8))


@pytest.mark.parametrize("res", [SMALL, WIDE], ids=lambda r: "%dx%d" % r)
def test_cached_camera_bounce_read_by_sets_of_another_shape(gpu_product, oracle_lib, monkeypatch, res):
    """antialiasing off: the camera bounce is written once, by a launch of one segment, into the cached stage -- which remembers its
    form -- and read by every later iteration's launches, in sets of several segments and another grid"""
    both_forms(gpu_product, oracle_lib, monkeypatch, _scene(gpu_product, "cornell.txt", res, 4), 4, iters=6, drive="reshape", antialiasing=0)


@pytest.mark.parametrize("scene,opt,env,why", [("cornellSpaceship20k.txt", {}, {}, 2), ("cornellObj.txt", {}, dict(PTX_DEBUG_MEM_BUDGET_MB="7"), 6)],
                         ids=["bvh_mesh_split_bounce", "memory_rule"])
def test_predicate_sends_back_to_the_tail(gpu_product, oracle_lib, monkeypatch, scene, opt, env, why):
    """a mesh with a tree is searched by the split bounce, whose ranking pass writes keys for the tail; and 7 MB for all streams in flight
    hold two iterations per set of the chunk-compact index (176 B x 3 lanes x 6144 paths x 2 = 6.5 MB), not of the seven-fold bin-major one
    (227 B per path: 8.4 MB).  Both runs are then the same code path:
    the plans are equal but for the reason."""
    both_forms(gpu_product, oracle_lib, monkeypatch, _scene(gpu_product, scene, SMALL, 4), 4, env=env, loop=False, why=why, **opt)
