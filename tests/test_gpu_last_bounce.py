"""GPU: the light-only last bounce (k_bounce<false, 3, FAST> in pt_kernels_last.hip).  The launch of bounce traceDepth - 1 stores no path: a ray that
reaches no emitting geom's inflated box ends black at once, the others are tested against all their candidates and only the winner's
material is looked at.  Frames, rays per bounce, the ray total and the fence counter must be what the full bounce gives: every case is
compared bit for bit with the CPU oracle AND with the same tracer under PTX_DEBUG_NO_LAST (today's path).  Frames of 64 x 48 (twelve
tiles of 256 paths) and 300 x 7 (owned pixels no multiple of the tile, later bounces smaller than one tile), two or three iterations."""
import os

import numpy as np
import pytest

from conftest import ROOT, beq

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (300, 7)]
MAT = "MATERIAL %d\nRGB %g %g %g\nSPECEX 0\nSPECRGB %g %g %g\nREFL %g\nREFR %g\nREFRIOR %g\nEMITTANCE %g\n\n"
CAMERA = "CAMERA\nRES 64 48\nFOVY 45\nITERATIONS 10\nDEPTH 8\nFILE last\nEYE 0.0 5 10.5\nLOOKAT 0 5 0\nUP 0 1 0\n\n"
ROOM = ["cube\nmaterial 1\nTRANS 0 0 0\nROTAT 0 0 0\nSCALE 10 .01 10", "cube\nmaterial 1\nTRANS 0 10 0\nROTAT 0 0 90\nSCALE .01 10 10",
        "cube\nmaterial 1\nTRANS 0 5 -5\nROTAT 0 90 0\nSCALE .01 10 10", "cube\nmaterial 2\nTRANS -5 5 0\nROTAT 0 0 0\nSCALE .01 10 10",
        "cube\nmaterial 3\nTRANS 5 5 0\nROTAT 0 0 0\nSCALE .01 10 10"]
LIGHT = "cube\nmaterial 0\nTRANS 0 10 0\nROTAT 0 0 0\nSCALE 3 .3 3"


def _materials(emittance=5):
    """light (or not), white, red, green, mirror"""
    return (MAT % (0, 1, 1, 1, 0, 0, 0, 0, 0, 0, emittance) + MAT % (1, .98, .98, .98, 0, 0, 0, 0, 0, 0, 0) + MAT % (2, .85, .35, .35, 0, 0, 0, 0, 0, 0, 0) +
            MAT % (3, .35, .85, .35, 0, 0, 0, 0, 0, 0, 0) + MAT % (4, .98, .98, .98, .98, .98, .98, 1, 0, 0, 0))


def _text(objects, emittance=5):
    return _materials(emittance) + CAMERA + "".join("OBJECT %d\n%s\n\n" % (i, o) for i, o in enumerate(objects))


def _mesh(tmp_path, name, ke):
    """models/cube.obj (12 triangles: no BVH, the pair tests' chunked mesh loop) under another name, with a material library of its own"""
    (tmp_path / "models" / "materials").mkdir(parents=True, exist_ok=True)
    obj = open(os.path.join(ROOT, "models", "cube.obj")).read().replace("mtllib cube.mtl", "mtllib %s.mtl" % name)
    (tmp_path / "models" / (name + ".obj")).write_text(obj)
    (tmp_path / "models" / "materials" / (name + ".mtl")).write_text(
        "newmtl M\nNs 96\nKa 1 1 1\nKd 0.9 0.8 0.6\nKs 0 0 0\nKe %g %g %g\nNi 1\nd 1\nillum 2\n" % (ke, ke, ke))
    return "obj\n../models/%s.obj" % name


def _scene(pt, tmp_path, text, res, depth):
    (tmp_path / "scenes").mkdir(exist_ok=True)
    f = tmp_path / "scenes" / "scene.txt"
    f.write_text(text)
    s = pt.Scene(str(f), base_dir=str(tmp_path / "scenes"), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s


def _file_scene(pt, name, res, depth):
    s = pt.Scene(os.path.join(ROOT, "scenes", name), res=res, depth=depth)
    s.apply_runcuda_camera()
    return s


def _render(pt, s, iters, opt):
    with pt.Tracer(s, **opt) as T:
        T.render(1, iters)
        st = T.stats()
        return T.read_image(), st


def both_ways(pt, O, monkeypatch, s, iters=3, tile=None, apps=0, **opt):
    """the oracle's frame and counts, the tracer's, and the tracer's with the light-only variant switched off: all the same bits"""
    d = s.dump()
    O.set_libm(1)
    O.create(d, d["textures"])
    O.set_options(aa=opt.get("antialiasing", 1), dof=0, sort=opt.get("sort_by_material", 1), cache=opt.get("cache_first_bounce", 1))
    if tile:
        O.set_tile(*tile)
        opt = dict(opt, tile_rows=tile[0], tile_rank=tile[1], tile_world=tile[2])
    if apps:
        O.set_apps_variant(1)
        opt = dict(opt, apps_variant=1)
    try:
        O.pt_init()
        for it in range(1, iters + 1):
            O.iterate(it)
        want, counts = O.image().copy(), O.live_counts().tolist()
    finally:
        if tile:
            O.set_tile(0, 0, 1)
        if apps:
            O.set_apps_variant(0)
        O.set_libm(0)
    monkeypatch.delenv("PTX_DEBUG_NO_LAST", raising=False)
    img, st = _render(pt, s, iters, opt)
    monkeypatch.setenv("PTX_DEBUG_NO_LAST", "1")
    img0, st0 = _render(pt, s, iters, opt)
    monkeypatch.delenv("PTX_DEBUG_NO_LAST")
    assert st["fenced"] == 0 and st0["fenced"] == 0
    assert beq(img0, want), "today's path against the oracle"
    assert beq(img, want), "the light-only last bounce against the oracle"
    # (an iteration that takes the camera bounce from the first-bounce cache traces no camera ray: the tracer counts none for bounce 0)
    b0 = 1 if (not opt.get("antialiasing", 1) and opt.get("cache_first_bounce", 1) and iters > 1) else 0
    assert st["rays_per_bounce"][b0: len(counts)] == counts[b0:] and st0["rays_per_bounce"][b0: len(counts)] == counts[b0:]
    assert list(st["rays_per_bounce"]) == list(st0["rays_per_bounce"]) and st["rays_total"] == st0["rays_total"]
    return img, st


@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("depth,aa", [(1, 1), (2, 0), (2, 1), (8, 1)])
def test_depths(gpu_product, oracle_lib, monkeypatch, res, depth, aa):
    """depth 1: the camera bounce is the last one and keeps its kernel; depth 2 without antialiasing: the last launch reads the cached
    camera bounce (iterations 2 and 3); depth 2 with it; depth 8: the bench's shape"""
    s = _file_scene(gpu_product, "cornellObj.txt", res, depth)
    img, _ = both_ways(gpu_product, oracle_lib, monkeypatch, s, antialiasing=aa)
    assert depth == 1 or img.any()      # (the 300 x 7 strip does not see the light directly)


@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("opt", [dict(), dict(sort_by_material=0), dict(batch=1, lanes=1), dict(batch=1, lanes=1, sort_by_material=0),
                                 dict(batch=1, lanes=3), dict(batch=2, lanes=1)],
                         ids=["specialised", "general", "direct_adds", "direct_adds_general", "three_lanes", "two_segments"])
def test_kernels_and_batching(gpu_product, oracle_lib, monkeypatch, res, opt):
    """material sort on / off (specialised / general kernel), one launch set of one iteration at a time (ending paths add to the image
    directly), three lanes and two segments (they store into per-iteration buffers and set the lit bit)"""
    s = _file_scene(gpu_product, "cornellObj.txt", res, 5)
    both_ways(gpu_product, oracle_lib, monkeypatch, s, **opt)


@pytest.mark.parametrize("batch", [1, 2])
def test_apps_variant(gpu_product, oracle_lib, monkeypatch, batch):
    """x PI at the deposit (and the general kernel for the launch set that holds iteration 1)"""
    s = _file_scene(gpu_product, "cornellObj.txt", (64, 48), 4)
    both_ways(gpu_product, oracle_lib, monkeypatch, s, apps=1, batch=batch)


@pytest.mark.parametrize("res", SIZES)
def test_row_tile_split(gpu_product, oracle_lib, monkeypatch, res):
    """rank 1 of 2: the pixel slot is not the pixel"""
    s = _file_scene(gpu_product, "cornellObj.txt", res, 4)
    both_ways(gpu_product, oracle_lib, monkeypatch, s, tile=(2 if res[1] < 16 else 8, 1, 2))
    both_ways(gpu_product, oracle_lib, monkeypatch, s, tile=(2 if res[1] < 16 else 8, 1, 2), batch=1, lanes=1)


def _occluders(tmp_path):
    # a cube and a small mesh under the light: rays that reach the light's box from below must end on them, black
    return ROOM + [LIGHT, "cube\nmaterial 2\nTRANS 1.2 8.6 0.5\nROTAT 0 20 0\nSCALE 2.5 .2 2.5",
                   _mesh(tmp_path, "shade", 0) + "\nTRANS -2.5 7.6 -1.5\nROTAT 0 30 0\nSCALE 1.2 .15 1.2", "sphere\nmaterial 4\nTRANS 2 2 0\nROTAT 0 0 0\nSCALE 2.5 2.5 2.5"]


def _two_lights(tmp_path):
    return ROOM + [LIGHT, "sphere\nmaterial 0\nTRANS -2 3 1\nROTAT 0 0 0\nSCALE 1.5 1.5 1.5", "cube\nmaterial 3\nTRANS 2 1.5 -1\nROTAT 0 30 0\nSCALE 2 3 2"]


def _mesh_light(tmp_path):
    # (the only light: every deposit of the last bounce is a hit on the mesh)
    return ROOM + [_mesh(tmp_path, "lamp", 4) + "\nTRANS -1 6 -1\nROTAT 0 15 0\nSCALE 1 .3 1", "cube\nmaterial 2\nTRANS 2 1 0\nROTAT 0 45 0\nSCALE 2 2 2"]


def _many_boxes(tmp_path):
    # thin plates turned by 45 degrees: world boxes 3.5 wide and high that overlap along most rays -- more than four candidates a ray,
    # so the pair lists take a second pass -- while the plates themselves hide little
    plates = ["cube\nmaterial %d\nTRANS %g %g %g\nROTAT 0 0 %d\nSCALE 5 .05 3" % (1 + k % 3, -2.4 + 0.8 * k, 4 + 0.5 * (k % 3), -1 + 0.3 * k, 45 if k % 2 else -45)
              for k in range(7)]
    return ROOM + [LIGHT] + plates


@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("sort", [1, 0], ids=["specialised", "general"])
@pytest.mark.parametrize("build", [_occluders, _two_lights, _mesh_light, _many_boxes], ids=["occluders", "two_lights", "mesh_light", "many_boxes"])
def test_scenes_built_to_go_wrong(gpu_product, oracle_lib, monkeypatch, tmp_path, build, sort, res):
    s = _scene(gpu_product, tmp_path, _text(build(tmp_path)), res, 4)
    img, _ = both_ways(gpu_product, oracle_lib, monkeypatch, s, iters=2, sort_by_material=sort)
    assert img.any()


@pytest.mark.parametrize("sort", [1, 0], ids=["specialised", "general"])
def test_no_light_at_all(gpu_product, oracle_lib, monkeypatch, tmp_path, sort):
    """light_bits == 0: the frame is black and the last bounce still counts its rays"""
    s = _scene(gpu_product, tmp_path, _text(ROOM + [LIGHT, "sphere\nmaterial 4\nTRANS 0 3 0\nROTAT 0 0 0\nSCALE 3 3 3"], emittance=0), (64, 48), 4)
    d = s.dump()
    assert gpu_product.api.debug_light_bits(d["materials"], d["geom_ints"][:, 1]) == 0
    img, st = both_ways(gpu_product, oracle_lib, monkeypatch, s, iters=2, sort_by_material=sort)
    assert not img.any() and st["rays_per_bounce"][3] > 0


@pytest.mark.parametrize("opt", [dict(), dict(no_mesh_split=1)], ids=["split_mesh_search", "textured_unsplit"])
def test_split_and_textured_scenes_keep_their_path(gpu_product, oracle_lib, monkeypatch, opt):
    """a scene with a BVH mesh (the split bounce) and a textured one (emissive texels end a path where it scatters): refused by the
    predicate, same results as ever"""
    s = _file_scene(gpu_product, "cornellSpaceship.txt", (64, 48), 4)
    both_ways(gpu_product, oracle_lib, monkeypatch, s, iters=2, **opt)
