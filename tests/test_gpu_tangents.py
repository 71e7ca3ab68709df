"""GPU: a stored hit that names one of a cube's tabulated normals takes the tangent frame of the diffuse sampler from a table (DScene::ctan,
read in k_bounce's fetch) instead of building it per ray; every other lane builds it as before.  The table holds the sampler's own bits
(tests/test_cube_tangents.py), so nothing may change: on 96 x 54 frames, depth 8, three iterations, the frame, the rays per bounce and the
fence counter equal the CPU oracle's bit for bit, with the table and under PTX_DEBUG_NO_TANGENTS (every lane computes), and the two frames
equal each other.  Scenes: cornellObj.txt; cubes of tests/test_cube_tangents.py inside the Cornell room, one per axis the sampler can cross
the normal with; a cube scaled unevenly and turned about three axes; the eye inside a cube (hits from inside: the code's `outside` bit is
clear); a material shared by a cube and a sphere next to cubes-only materials (records with and without a code in one stream, waves that hold
both); cornellObj.txt through the general kernel (PTX_DEBUG_NO_FAST); the split scene on the stand-in mesh (pass 1's head); depth 2 (the
light-only last bounce reads the camera bounce's records); a tracer whose camera bounce was cached and then captured (the input's record
masks differ from the launch's).  No case is empty: with the table on, the run stores records that carry a normal code."""
import os

import numpy as np
import pytest

import tangent_ref as tr
from conftest import ROOT, beq
from test_cube_tangents import TRS
from test_gpu_mesh_walks import box_geoms, make_scene, oracle_for
from test_gpu_parity import O, fences_stay_silent      # noqa: F401  (fixtures; the fence check is autouse)

pytestmark = pytest.mark.gpu
f32 = np.float32
RES, DEPTH, ITERS = (96, 54), 8, 3


def _in_room(name, pos=(-1.0, 4.0, -1.0), scale=(3.0, 3.0, 3.0)):
    """a cube with the rotation of the CPU file's case, inside the room"""
    return tuple(pos) + tuple(TRS[name][3:6]) + tuple(scale)


def scene(pt, O, name):
    """-> (POD dict, tracer options, environment, the notNormal choice some face of the added cube must take or None)"""
    box, mats = box_geoms()

    def from_file(fname, depth=DEPTH):
        s = pt.Scene(os.path.join(ROOT, "scenes", fname), res=RES, depth=depth)
        s.apply_runcuda_camera()
        return s.dump()

    def room(extra, **kw):
        return make_scene(O, box + extra, mats, res=RES, depth=DEPTH, **kw)
    if name == "cornellObj":
        return from_file("cornellObj.txt"), {}, {}, None
    if name == "turned_diag":            # a face normal along (1,1,1)/sqrt(3): |x| and |y| at the threshold
        return room([("cube", 2, _in_room("diag"))]), {}, {}, None
    if name == "turned_y45":             # |x| >= sqrt(1/3) > |y|: the y axis
        return room([("cube", 2, _in_room("y45"))]), {}, {}, 1
    if name == "turned_z45":             # |x|, |y| >= sqrt(1/3): the z axis
        return room([("cube", 3, _in_room("z45"))]), {}, {}, 2
    if name == "uneven":
        return room([("cube", 3, (1.0, 4.0, -1.0, 50.0, 15.0, -80.0, 3.0, 0.6, 2.0))]), {}, {}, 0
    if name == "eye_inside":             # the room and the eye (0, 5, 10.5) inside one large turned cube
        return room([("cube", 3, (0.0, 5.0, 3.0, 0.0, 20.0, 0.0, 18.0, 14.0, 30.0))]), {}, {}, None
    if name == "shared_material":        # material 2: the left wall AND a sphere -- its records carry normals; materials 1 and 3: cubes only
        return room([("sphere", 2, (-1.0, 4.0, -1.0, 0.0, 0.0, 0.0, 3.0, 3.0, 3.0)), ("cube", 3, (2.0, 2.0, 1.0, 0.0, 30.0, 0.0, 2.0, 4.0, 2.0))]), {}, {}, None
    if name == "no_fast":
        return from_file("cornellObj.txt"), {}, {"PTX_DEBUG_NO_FAST": "1"}, None
    if name == "split":
        return from_file("cornellSpaceship.txt"), {}, {}, None
    if name == "depth2":
        return from_file("cornellObj.txt", depth=2), {}, {}, None
    raise KeyError(name)


SCENES = ["cornellObj", "turned_diag", "turned_y45", "turned_z45", "uneven", "eye_inside", "shared_material", "no_fast", "split", "depth2"]


def both_ways(pt, monkeypatch, d, opt, drive, check=None):
    """drive(T) on a tracer with the table and on one under PTX_DEBUG_NO_TANGENTS -> [(image, stats)] * 2; check(T): the path the tracer takes"""
    out = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("PTX_DEBUG_NO_TANGENTS", "1")
        else:
            monkeypatch.delenv("PTX_DEBUG_NO_TANGENTS", raising=False)
        with pt.Tracer.from_pod(d, **opt) as T:
            drive(T)
            out.append((T.read_image(), T.stats()))
            if check:
                check(T)
    monkeypatch.delenv("PTX_DEBUG_NO_TANGENTS", raising=False)
    return out


def compare(name, runs, want, counts, cached_camera_bounce=False):
    """cached_camera_bounce: the last iteration took its camera bounce from the cache -- the device traced no ray there and counts none"""
    if cached_camera_bounce:
        counts = [0] + counts[1:]
    for (img, st), how in zip(runs, ("table", "every lane computes")):
        print(name, how, "rays per bounce", st["rays_per_bounce"], "stored", st["stored_paths"], "with normal code", st["stored_with_normal_code"], "fenced", st["fenced"])
        assert beq(img, want), "%s, %s: %d of %d pixels differ from the oracle" % (name, how, int((img != want).any(axis=1).sum()), len(img))
        assert st["rays_per_bounce"][:len(counts)] == counts and not any(st["rays_per_bounce"][len(counts):]), (how, st["rays_per_bounce"], counts)
        assert st["fenced"] == 0
    assert beq(runs[0][0], runs[1][0]) and runs[0][0].any()
    assert runs[0][1]["rays_per_bounce"] == runs[1][1]["rays_per_bounce"]
    assert runs[0][1]["stored_with_normal_code"] > 0, "no record of this run carried a normal code: the table was never read"


@pytest.mark.parametrize("name", SCENES)
def test_frames_with_the_table_and_without(gpu_product, O, monkeypatch, name):
    pt = gpu_product
    d, opt, env, must_choose = scene(pt, O, name)
    depth = int(d["cam_ints"][3])
    assert tuple(d["cam_ints"][:2]) == RES and depth == (2 if name == "depth2" else DEPTH)
    # ---- on the CPU: what the case is there for
    if must_choose is not None:
        assert must_choose in {tr.choice(n) for n in tr.cube_normals(d["geom_mats"][-1][32:48])}
    if name == "turned_diag":
        near = [n for n in tr.cube_normals(d["geom_mats"][-1][32:48]) if abs(abs(n[0]) - tr.SQRT_OF_ONE_THIRD) < 1e-6 and abs(abs(n[1]) - tr.SQRT_OF_ONE_THIRD) < 1e-6]
        assert near, "no face normal along (1,1,1)/sqrt(3)"
    if name == "eye_inside":
        inv = d["geom_mats"][-1][16:32].astype(np.float64).reshape(4, 4).T
        eye = inv @ np.array([0.0, 5.0, 10.5, 1.0])
        assert np.all(np.abs(eye[:3]) < 0.5), eye
        oracle_for(O, d)
        O.pt_generate(1)
        first = O.compute_intersections(O.paths())
        assert ((first["t"] > 0) & (first["geomId"] == len(d["geom_ints"]) - 1)).mean() > 0.05      # camera rays that leave the room hit it from inside
    # ---- the oracle's iterations
    oracle_for(O, d)
    for it in range(1, ITERS + 1):
        O.iterate(it)
    want, counts = O.image().copy(), O.live_counts().tolist()
    # ---- on the device, both ways
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    meshes = [g for g in range(len(d["geom_ints"])) if int(d["geom_ints"][g][0]) == 3]

    def check(T):
        # the bounce the case is there for: split (pass 1 reads the coded records) only for "split", unsplit everywhere else
        assert [bool(T.mesh_plan(g)["split"]) for g in meshes] == [name == "split"] * len(meshes)
    if name == "split":
        assert meshes
    runs = both_ways(pt, monkeypatch, d, opt, lambda T: T.render(1, ITERS), check)
    compare(name, runs, want, counts)
    if name == "no_fast":
        # there is no query for the variant a launch took.  What can be shown: every precondition of the specialised kernel holds for this scene
        # (asked for regardless, it runs and gives the same frame), so the frames above differ from case "cornellObj" by the switch alone
        monkeypatch.delenv("PTX_DEBUG_NO_FAST")
        monkeypatch.setenv("PTX_DEBUG_FORCE_FAST", "1")
        with pt.Tracer.from_pod(d, **opt) as T:
            T.render(1, ITERS)
            assert beq(T.read_image(), want)
        monkeypatch.delenv("PTX_DEBUG_FORCE_FAST")
    if name == "shared_material":        # both kinds of record in the stream
        assert 0 < runs[0][1]["stored_with_normal_code"] < runs[0][1]["stored_paths"]


def test_captured_after_the_camera_bounce_was_cached(gpu_product, O, monkeypatch):
    """The call order of test_capture_after_the_camera_bounce_was_cached (tests/test_gpu_parity.py): without antialiasing iterations 1-3 fill
    and use the cached camera bounce, written with the record masks on; iteration 4 is captured, which switches the masks off for its own
    launches -- the bounce that reads the cache reads coded records, and their frames from the table, under a launch that writes none."""
    pt = gpu_product
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"), res=RES, depth=DEPTH)
    s.apply_runcuda_camera()
    d = s.dump()
    O.set_libm(1)
    O.create(d, d["textures"])
    O.set_options(aa=0, dof=0, sort=1, cache=1)
    O.pt_init()
    for it in range(1, 5):
        O.iterate(it)
    want, counts = O.image().copy(), O.live_counts().tolist()

    def drive(T):
        T.render(1, 3)
        T.debug_capture(1)
        T.pathtrace(4)
        assert len(T.debug_stream()["pix"]) > 100

    assert counts[0] == RES[0] * RES[1]
    compare("captured", both_ways(pt, monkeypatch, d, dict(antialiasing=0), drive), want, counts, cached_camera_bounce=True)
