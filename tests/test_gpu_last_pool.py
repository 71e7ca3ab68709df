"""GPU: the pool of the light-only last bounce (k_bounce<false, 3, true>).  The rays that reach an emitter's inflated box are
collected over a workgroup's tiles in LDS and go through the pair tests once TILE of them are together (or after the workgroup's last
tile), with the pooled throughput colour and pixel slot deciding the deposit.  Every case is compared bit for bit with the CPU oracle
(frame, rays per bounce), with the same tracer under PTX_DEBUG_NO_LAST (the full bounce) and under PTX_DEBUG_LAST_INPLACE (every tile's
survivors tested where they are), and once more with PTX_DEBUG_GX_LAST = 1: at these frame sizes the launch has a workgroup per tile, so
only with ONE workgroup per segment does a workgroup see all the tiles -- its pool fills, drains with rays waiting, and drains again
behind the last tile, as it does at 1080p.  The fence counter stays 0 throughout.

Frames: 160 x 90 (57 tiles of 256 paths, the last one partial) and 257 x 33 (tiles wrap rows), three iterations."""
import pytest

from conftest import beq
from test_gpu_last_bounce import LIGHT, ROOM, _file_scene, _mesh, _render, _scene, _text, both_ways

pytestmark = pytest.mark.gpu

SIZES = [(160, 90), (257, 33)]


def every_way(pt, O, monkeypatch, s, iters=3, tile=None, **opt):
    """both_ways (oracle = pooled = full bounce), then: pooled = in place = pooled with one workgroup per segment = the latter in place"""
    monkeypatch.delenv("PTX_DEBUG_LAST_INPLACE", raising=False)
    monkeypatch.delenv("PTX_DEBUG_GX_LAST", raising=False)
    img, st = both_ways(pt, O, monkeypatch, s, iters=iters, tile=tile, **opt)
    if tile:
        opt = dict(opt, tile_rows=tile[0], tile_rank=tile[1], tile_world=tile[2])
    for env in (dict(PTX_DEBUG_LAST_INPLACE="1"), dict(PTX_DEBUG_GX_LAST="1"), dict(PTX_DEBUG_GX_LAST="1", PTX_DEBUG_LAST_INPLACE="1")):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            img1, st1 = _render(pt, s, iters, opt)
        finally:
            for k in env:
                monkeypatch.delenv(k)
        assert st1["fenced"] == 0, env
        assert beq(img1, img), env
        assert list(st1["rays_per_bounce"]) == list(st["rays_per_bounce"]) and st1["rays_total"] == st["rays_total"], env
    return img, st


@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("depth", [2, 3, 8])
def test_depths(gpu_product, oracle_lib, monkeypatch, res, depth):
    """depth 2: the last bounce reads the camera bounce's records directly; depth 8: the bench's shape"""
    s = _file_scene(gpu_product, "cornellObj.txt", res, depth)
    img, _ = every_way(gpu_product, oracle_lib, monkeypatch, s)
    assert img.any()


@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("opt", [dict(lanes=1), dict()], ids=["one_lane", "default_lanes"])
def test_lanes(gpu_product, oracle_lib, monkeypatch, res, opt):
    s = _file_scene(gpu_product, "cornellObj.txt", res, 5)
    every_way(gpu_product, oracle_lib, monkeypatch, s, **opt)


@pytest.mark.parametrize("res", SIZES)
def test_no_emitter_pools_nothing(gpu_product, oracle_lib, monkeypatch, tmp_path, res):
    s = _scene(gpu_product, tmp_path, _text(ROOM + [LIGHT, "sphere\nmaterial 4\nTRANS 0 3 0\nROTAT 0 0 0\nSCALE 3 3 3"], emittance=0), res, 4)
    img, st = every_way(gpu_product, oracle_lib, monkeypatch, s)
    assert not img.any() and st["rays_per_bounce"][3] > 0


@pytest.mark.parametrize("res", SIZES)
def test_emitter_box_encloses_the_room(gpu_product, oracle_lib, monkeypatch, tmp_path, res):
    """every ray of the last bounce reaches the emitter's box: a full tile fills the pool, which drains tile by tile"""
    s = _scene(gpu_product, tmp_path, _text(ROOM + ["cube\nmaterial 0\nTRANS 0 5 0\nROTAT 0 0 0\nSCALE 40 40 40",
                                                    "sphere\nmaterial 4\nTRANS 2 2 0\nROTAT 0 0 0\nSCALE 2.5 2.5 2.5"], emittance=1), res, 4)
    img, _ = every_way(gpu_product, oracle_lib, monkeypatch, s)
    assert img.any()


@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("depth", [2, 3])
def test_pool_fills_in_the_middle_of_a_tile(gpu_product, oracle_lib, monkeypatch, tmp_path, res, depth):
    """an emitter whose box is the room above y = 7 and far beyond: about 60 % of the last bounce's rays reach it (counted on the oracle's
    rays with tools/last_pool_census.py: 90 to 150 per tile on average, up to 250), so with one workgroup per segment the pool passes TILE
    in the middle of every second tile or so: some of that tile's rays go in, the others wait for the drain and go in behind it"""
    s = _scene(gpu_product, tmp_path, _text(ROOM + ["cube\nmaterial 0\nTRANS 0 30 0\nROTAT 0 0 0\nSCALE 60 46 60",
                                                    "sphere\nmaterial 4\nTRANS 2 2 0\nROTAT 0 0 0\nSCALE 2.5 2.5 2.5"], emittance=1), res, depth)
    img, _ = every_way(gpu_product, oracle_lib, monkeypatch, s)
    assert img.any()


@pytest.mark.parametrize("res", SIZES)
def test_small_mesh_emits(gpu_product, oracle_lib, monkeypatch, tmp_path, res):
    """mesh pairs (chunked triangle loops) inside a pooled call; the mesh is the only light"""
    objs = ROOM + [_mesh(tmp_path, "lamp", 4) + "\nTRANS -1 6 -1\nROTAT 0 15 0\nSCALE 1 .3 1", "cube\nmaterial 2\nTRANS 2 1 0\nROTAT 0 45 0\nSCALE 2 2 2"]
    s = _scene(gpu_product, tmp_path, _text(objs), res, 4)
    img, _ = every_way(gpu_product, oracle_lib, monkeypatch, s)
    assert img.any()


@pytest.mark.parametrize("res", SIZES)
def test_row_tile_split(gpu_product, oracle_lib, monkeypatch, res):
    """tile_world 2, rank 1: the pooled pixel slot is not the pixel, and is checked against the pixels this device owns"""
    s = _file_scene(gpu_product, "cornellObj.txt", res, 4)
    every_way(gpu_product, oracle_lib, monkeypatch, s, tile=(8, 1, 2))
