"""GPU: the camera bounce's shortcuts for waves whose 64 lanes agree (tileIntersect<SUBSET>: equal candidate masks -> pair-list slots
in closed form; the ranking: one bin, every lane alive -> rank = lane), and the packed scan that gives every other wave its slots.  There
is no switch for either: frames, rays per bounce and the sorted streams (as test_gpu_parity.py compares them) are held against the CPU
oracle bit for bit.

Scenes: cornellObj and cornell (its sphere) -- uniform and mixed waves side by side; one wall that fills the frame -- every wave uniform,
one candidate; five plates one behind the other that each fill the frame -- every wave uniform with FIVE candidates, more than a pass of
the pair lists takes (ITEMS_PER_PASS = 4), so the shortcut must step aside.  Frames of 64 x 48 (a row is one wave), 320 x 180 (a row is
five waves: tiles start mid-row) and 257 x 33 (waves straddle rows), antialiasing on (the specialised kernel) and off (with the camera
bounce's cache off, so that it is traced every iteration), depth 1 (the camera bounce stores nothing) and 3."""
import os

import pytest

from conftest import ROOT, beq
from test_gpu_last_bounce import _scene, _text
from test_gpu_parity import check_sorted_streams

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (320, 180), (257, 33)]
BEHIND = "cube\nmaterial 0\nTRANS 0 5 14\nROTAT 0 0 0\nSCALE 6 6 .3"      # a light behind the camera: in no camera tile's subset


def _wall(tmp_path):
    return ["cube\nmaterial 1\nTRANS 0 5 -5\nROTAT 0 0 0\nSCALE 60 60 .01", BEHIND]


def _five_plates(tmp_path):
    return ["cube\nmaterial %d\nTRANS 0 5 %g\nROTAT 0 0 0\nSCALE 60 60 .01" % (1 + k % 3, -1.0 - k) for k in range(5)] + [BEHIND]


def _build(pt, tmp_path, scene, res, depth):
    if isinstance(scene, str):
        s = pt.Scene(os.path.join(ROOT, "scenes", scene), res=res, depth=depth)
        s.apply_runcuda_camera()
        return s
    return _scene(pt, tmp_path, _text(scene(tmp_path)), res, depth)


@pytest.mark.parametrize("res", SIZES, ids=lambda r: "%dx%d" % r)
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("aa", [1, 0], ids=["aa", "no_aa"])
@pytest.mark.parametrize("scene", ["cornellObj.txt", "cornell.txt", _wall, _five_plates], ids=["cornellObj", "cornell", "wall", "five_plates"])
def test_camera_bounce(gpu_product, oracle_lib, tmp_path, scene, aa, depth, res):
    pt, O = gpu_product, oracle_lib
    s = _build(pt, tmp_path, scene, res, depth)
    d = s.dump()
    opt = dict(antialiasing=aa, cache_first_bounce=0)
    O.set_libm(1)
    try:
        O.create(d, d["textures"])
        O.set_options(aa=aa, dof=0, sort=1, cache=0)
        O.pt_init()
        for it in (1, 2):
            O.iterate(it)
        want, counts = O.image().copy(), O.live_counts().tolist()
        with pt.Tracer(s, **opt) as T:
            T.render(1, 2)
            st = T.stats()
            img = T.read_image()
        assert st["fenced"] == 0
        assert beq(img, want)
        assert st["rays_per_bounce"][: len(counts)] == counts
        O.pt_init()
        with pt.Tracer(s, **opt) as T:
            check_sorted_streams(T, O, d, depth)
            assert T.stats()["fenced"] == 0
    finally:
        O.set_libm(0)
