"""GPU: small meshes are candidates of the rays that reach their OBJECT-space box (cullMask / objBoxReach, pt_device.h).  The
pre-test only decides which pairs are tested, so nothing may change: on 64 x 48 frames, depth 4, two iterations, the frame, the rays per
bounce, the sorted stream after every bounce and the fence counter are bit-identical to the CPU oracle, with the object-space boxes and
under PTX_DEBUG_NO_OBJCULL (the world boxes alone, the path before them).  Scenes: cornellObj.txt as it is; a mesh turned about two axes
and scaled unevenly; a flat quad; two bars whose world boxes overlap and whose own boxes do not; a mesh that is the scene's only light
(the last bounce looks only for light: cullMask through light_bits); a camera beyond CULL_FAR_ORIGIN (cull == 2: its rays keep every
candidate); depth of field (the general kernel); PTX_DEBUG_NO_FAST.

No case passes vacuously, shown on the CPU from the oracle's camera rays alone: some ray hits the mesh, the table has an entry for it,
and -- except for the flat quad and the far camera -- the restated device arithmetic (tests/test_cull_boxes.py for the world box,
tests/test_cull_objboxes.py for the object box) rejects a ray that the world box admits."""
import ctypes as C
import os

import numpy as np
import pytest

import meshcases as mc
from conftest import ROOT, beq
from test_cull_boxes import _device_slab
from test_cull_objboxes import device_objbox
from test_gpu_mesh_walks import box_geoms, make_scene, oracle_for
from test_gpu_parity import O, check_sorted_streams, fences_stay_silent      # noqa: F401  (fixtures; the fence check is autouse)

pytestmark = pytest.mark.gpu
f32 = np.float32
RES, DEPTH, ITERS = (64, 48), 4, 2


def cube_mesh():
    """the unit cube as 12 triangles, outward counter-clockwise"""
    tri = []
    for axis in range(3):
        for side in (0, 1):
            p = np.zeros((4, 3))
            p[:, axis] = 0.5 if side else -0.5
            p[:, (axis + 1) % 3] = [-0.5, 0.5, 0.5, -0.5]
            p[:, (axis + 2) % 3] = [-0.5, -0.5, 0.5, 0.5]
            if not side:
                p = p[::-1]
            tri += [p[[0, 1, 2]], p[[0, 2, 3]]]
    return mc.with_uv(np.array(tri))


def quad_mesh():
    p = np.array([[[-0.5, 0, -0.5], [0.5, 0, 0.5], [0.5, 0, -0.5]], [[-0.5, 0, -0.5], [-0.5, 0, 0.5], [0.5, 0, 0.5]],
                  [[-0.5, 0, -0.5], [0.5, 0, -0.5], [0.5, 0, 0.5]], [[-0.5, 0, -0.5], [0.5, 0, 0.5], [-0.5, 0, 0.5]]])      # both sides
    return mc.with_uv(p)


def scene(O, name):
    """-> (POD dict, mesh geom indices, tracer options, environment, must some camera ray be rejected by the object box alone)"""
    box, mats = box_geoms()
    cube = cube_mesh()
    turned = ("mesh", 2, (-1.0, 4.0, -1.0, 35.0, 0.0, 50.0, 3.0, 1.2, 2.0), cube)
    if name == "cornellObj":
        import mygpuraytracer_amd as pt
        s = pt.Scene(os.path.join(ROOT, "scenes", "cornellObj.txt"), res=RES, depth=DEPTH)
        s.apply_runcuda_camera()
        return s.dump(), [6], {}, {}, True
    if name == "two_axes_uneven":
        return make_scene(O, box + [turned], mats), [6], {}, {}, True
    if name == "flat_quad":
        return make_scene(O, box + [("mesh", 3, (0.5, 3.5, -1.0, 25.0, 30.0, 10.0, 4.0, 1.0, 3.0), quad_mesh())], mats), [6], {}, {}, False
    if name == "overlapping_bars":
        bars = [("mesh", 2, (-0.9, 5.0, -1.0, 0.0, 0.0, 45.0, 6.0, 0.5, 0.8), cube), ("mesh", 3, (0.9, 5.0, -1.0, 0.0, 0.0, 45.0, 6.0, 0.5, 0.8), cube)]
        return make_scene(O, box + bars, mats), [6, 7], {}, {}, True
    if name == "mesh_light":
        lamp = ("mesh", 0, (-0.5, 8.5, -0.5, 0.0, 40.0, 15.0, 3.0, 0.4, 2.0), cube)
        return make_scene(O, box[1:] + [lamp, ("cube", 2, (2.0, 1.5, 0.0, 0.0, 30.0, 0.0, 2.0, 3.0, 2.0))], mats), [5], {}, {}, True
    if name == "far_camera":
        d = make_scene(O, box + [turned], mats)
        cf = O.camera_from_loader(RES[0], RES[1], 0.4, (0.0, 5.0, 1200.0), (0.0, 5.0, 0.0), (0.0, 1.0, 0.0))
        O.lib.o_runcuda_camera(cf.ctypes.data_as(C.c_void_p))
        d["cam_floats"] = cf
        return d, [6], {}, {}, False
    if name == "depth_of_field":
        return make_scene(O, box + [turned], mats), [6], dict(depth_of_field=1), {}, True
    if name == "no_fast":
        return make_scene(O, box + [turned], mats), [6], {}, {"PTX_DEBUG_NO_FAST": "1"}, True
    raise KeyError(name)


SCENES = ["cornellObj", "two_axes_uneven", "flat_quad", "overlapping_bars", "mesh_light", "far_camera", "depth_of_field", "no_fast"]


def world_table(pt, d, g):
    """geom g's world box as the device reads it: make_world_aabb's rule (pt_scene.hip: the vertices' box widened by 1e-3 + 1e-4 |coordinate|)"""
    X = d["geom_mats"][g][:16].astype(np.float64).reshape(4, 4).T
    v = d["faces"][g].astype(np.float64).reshape(-1, 5)[:, :3]
    w = v @ X[:3, :3].T + X[:3, 3]
    lo, hi = w.min(axis=0), w.max(axis=0)
    m = 1e-3 + 1e-4 * np.maximum(np.abs(lo), np.abs(hi))
    corner = np.concatenate([np.nextafter(f32(lo - m), f32(-np.inf)), np.nextafter(f32(hi + m), f32(np.inf))]).astype(f32)
    return pt.api.debug_cull_boxes([corner])[0]


@pytest.mark.parametrize("name", SCENES)
def test_frames_with_and_without_the_object_boxes(gpu_product, O, monkeypatch, name):
    pt = gpu_product
    d, meshes, opt, env, must_reject = scene(O, name)
    dof = opt.get("depth_of_field", 0)
    assert tuple(d["cam_ints"][:2]) == RES and int(d["cam_ints"][3]) == DEPTH
    # ---- on the CPU: the case is not empty
    tab, bits = pt.api.debug_cull_objboxes(d["geom_ints"], d["geom_mats"], d["faces"])
    assert bits == sum(1 << g for g in meshes), bits
    oracle_for(O, d, dof=dof)
    O.pt_generate(1)
    cam = O.paths()
    o, dr = cam["origin"], cam["direction"]
    far = np.abs(o).max() > 1024.0
    assert far == (name == "far_camera")
    rejected = 0
    for g in meshes:
        hit = O.geom_test(g, np.concatenate([o, dr], axis=1))[:, 0] > 0
        in_world = _device_slab(world_table(pt, d, g), o, dr)
        in_obj = device_objbox(tab[g], o, dr)
        print(name, "geom", g, "camera rays", len(o), "hit the mesh", int(hit.sum()), "reach the world box", int(in_world.sum()),
              "of them the object box", int((in_world & in_obj).sum()))
        assert hit.sum() >= 1 and not np.any(hit & ~in_obj) and not np.any(hit & ~in_world)
        rejected += int((in_world & ~in_obj).sum())
    assert rejected >= 1 or not must_reject
    # ---- the oracle's two iterations
    oracle_for(O, d, dof=dof)
    for it in range(1, ITERS + 1):
        O.iterate(it)
    want, counts = O.image().copy(), O.live_counts().tolist()
    # ---- on the device, both ways
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    images = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("PTX_DEBUG_NO_OBJCULL", "1")
        else:
            monkeypatch.delenv("PTX_DEBUG_NO_OBJCULL", raising=False)
        with pt.Tracer.from_pod(d, **opt) as T:
            T.render(1, ITERS)
            img, st = T.read_image(), T.stats()
            assert beq(img, want), "%s: %d of %d pixels differ from the oracle" % ("world boxes alone" if off else "object boxes", int((img != want).any(axis=1).sum()), len(img))
            assert st["rays_per_bounce"][:len(counts)] == counts and not any(st["rays_per_bounce"][len(counts):]), (st["rays_per_bounce"], counts)
            assert st["fenced"] == 0
            oracle_for(O, d, dof=dof)
            check_sorted_streams(T, O, d, DEPTH)
            assert T.stats()["fenced"] == 0
        images.append(img)
    assert beq(images[0], images[1]) and images[0].any()
