"""CPU: the table of tangent frames k_bounce reads instead of building a frame per ray (DScene::ctan; cube_face_tables in pt_scene.hip with
the sampler's own tangentFrame of pt_device.h, handed out device-free by ptx_debug_cube_tangents).  A stored hit on a cube of a cubes-only
material names one of the cube's six tabulated normals; its record's reader takes perp1 and perp2 of that normal from the table, so the
table must hold the very bits the sampler computes: compared here, byte for byte, with a binary32 restatement (tests/tangent_ref.py: cross,
dot left to right, 1 / sqrt and multiply, one rounding each) over cubes under some forty transforms -- identity, the Cornell walls,
non-uniform scales with rotations about one, two and three axes, cubes turned so that a face normal is (1,1,1)/sqrt(3), and matrices whose
face normal has |x| or |y| a few ulps on either side of sqrt(1/3), where the sampler changes the axis it crosses the normal with.  All
three choices of that axis occur.  Geoms that are not cubes get zeros."""
import numpy as np
import pytest

import tangent_ref as tr
from conftest import beq, golden
import mygpuraytracer_amd as pt

f32 = np.float32
SPHERE, CUBE, MESH = 0, 1, 3

# (translation, rotation in degrees, scale)
TRS = {
    "identity": (0, 0, 0, 0, 0, 0, 1, 1, 1),
    "scaled": (1, 2, 3, 0, 0, 0, 3.0, 0.05, 0.6),
    "x30": (0, 5, 0, 30, 0, 0, 1.0, 2.0, 0.5), "y45": (-2, 4, -3, 0, 45, 0, 2, 2, 2), "z70": (1, 1, 1, 0, 0, 70, 0.7, 1.3, 0.9),
    "x_neg": (0, 0, 0, -110, 0, 0, 1.5, 1, 1), "y27": (2, 0, -3, 0, 27.5, 0, 3, 3.3, 3), "z45": (0, 0, 0, 0, 0, 45, 1, 1, 1),
    "xy": (0.3, 5, -0.5, 25, 40, 0, 1.2, 0.8, 1.0), "yz": (0, 0, 0, 0, -35, 20, 1.0, 1.1, 0.9), "xz": (0, 0, 0, 60, 0, -50, 0.5, 2.0, 4.0),
    "xyz": (0.3, 5.0, -0.5, 25.0, 40.0, -15.0, 1.2, 0.8, 1.0), "xyz2": (-0.5, 4.0, 0.5, -70.0, 10.0, 130.0, 0.7, 1.3, 0.9),
    "xyz3": (1.0, 2.0, 3.0, 50.0, 15.0, -80.0, 3.0, 0.05, 0.6), "xyz_tiny": (0.5, 5.0, 1.0, 10.0, 20.0, 30.0, 0.01, 0.01, 0.01),
    "xyz_huge": (20.0, -30.0, 10.0, 33.0, -20.0, 70.0, 300.0, 300.0, 300.0),
    # a face normal along (1,1,1)/sqrt(3): the x axis turned about z by asin(1/sqrt(3)), then about y by -45 (and the other order of angles)
    "diag": (0, 5, 0, 0, -45, 35.264389682754654, 1, 1, 1), "diag2": (0, 5, 0, 35.264389682754654, 45, 0, 1, 1, 1),
    "diag_scaled": (0, 5, 0, 0, -45, 35.264389682754654, 2, 2, 2),
}


def _walls():
    g = golden("loader_cornell.npz")
    return [(("cornell%d" % i), g["geom_mats"][i].copy()) for i in range(len(g["geom_ints"])) if int(g["geom_ints"][i][0]) == CUBE]


def _matrix_with_normal(v, axis=0):
    """48 floats whose invTranspose has column `axis` = v (the normal of that axis' two faces before normalize); the other columns are plain"""
    m = np.eye(4, dtype=f32)
    m[:3, (axis + 1) % 3] = (0.25, -2.0, 0.5)
    m[:3, (axis + 2) % 3] = (-1.5, 0.125, 3.0)
    m[:3, axis] = v
    flat = m.T.reshape(-1)                       # by columns
    return np.concatenate([np.eye(4, dtype=f32).reshape(-1), np.eye(4, dtype=f32).reshape(-1), flat]).astype(f32)


def _ulps(x, k):
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


def _near_threshold():
    """normals whose |x| (|y| large) resp. |y| (|x| large) crosses sqrt(1/3): (c, 1.2, t) and (1.2, c, t) with c = 1 and t near sqrt(0.56),
    moved in steps of 16 ulps -- each moves the normalised component by about two ulps"""
    out = []
    for k in range(-64, 65, 16):
        t = _ulps(np.sqrt(0.56), k)
        out.append(("x_near_%+d" % k, _matrix_with_normal((1.0, 1.2, t), 0)))
        out.append(("y_near_%+d" % k, _matrix_with_normal((1.2, 1.0, t), 2)))
    for k in (-2, -1, 0, 1, 2):                  # (1,1,1) itself and its neighbours
        out.append(("ones_%+d" % k, _matrix_with_normal((_ulps(1.0, k), 1.0, 1.0), 1)))
    return out


@pytest.fixture(scope="module")
def cases(oracle_lib):
    c = [(name, oracle_lib.build_transforms(np.array(t, f32))) for name, t in TRS.items()]
    return c + _walls() + _near_threshold()


def test_table_equals_the_restated_sampler(cases):
    assert 35 <= len(cases) <= 60, len(cases)
    gi = np.array([[CUBE, 1, 0]] * len(cases), np.int32)
    gm = np.stack([m for _, m in cases]).astype(f32)
    got = pt.api.debug_cube_tangents(gi, gm)
    assert got.shape == (len(cases), 6, 6) and got.dtype == f32
    seen, below_x, above_x, below_y, above_y = set(), 0, 0, 0, 0
    for k, (name, m) in enumerate(cases):
        want = tr.frames(m[32:48])
        normals = tr.cube_normals(m[32:48])
        assert np.isfinite(want).all(), name
        assert beq(got[k], want), "%s: sides %s differ\n%s\n%s" % (name, np.nonzero((got[k].view(np.uint32) != want.view(np.uint32)).any(axis=1))[0].tolist(), got[k], want)
        for n in normals:
            seen.add(tr.choice(n))
            dx, dy = abs(n[0]) - tr.SQRT_OF_ONE_THIRD, abs(n[1]) - tr.SQRT_OF_ONE_THIRD
            near = 16 * np.spacing(tr.SQRT_OF_ONE_THIRD)
            below_x += -near <= dx < 0; above_x += 0 <= dx <= near
            if abs(n[0]) >= tr.SQRT_OF_ONE_THIRD:
                below_y += -near <= dy < 0; above_y += 0 <= dy <= near
        # a frame is a frame: unit vectors, orthogonal to the normal and to each other (binary32 rounding and no more)
        for side, n in enumerate(normals):
            p1, p2 = got[k, side, :3].astype(np.float64), got[k, side, 3:].astype(np.float64)
            nn = np.array(n, np.float64)
            assert abs(p1 @ p1 - 1) < 1e-6 and abs(p2 @ p2 - 1) < 1e-6 and abs(p1 @ nn) < 1e-6 and abs(p2 @ nn) < 1e-6 and abs(p1 @ p2) < 1e-6, (name, side)
    print("notNormal choices seen:", sorted(seen), "normals within 16 ulps of the threshold: |x| below/above %d/%d, |y| below/above %d/%d" % (below_x, above_x, below_y, above_y))
    assert seen == {0, 1, 2}
    assert below_x and above_x and below_y and above_y


def test_other_geoms_get_zeros(oracle_lib):
    m = oracle_lib.build_transforms(np.array(TRS["xyz"], f32))
    gi = np.array([[SPHERE, 1, 0], [CUBE, 2, 0], [MESH, 1, 0], [7, 0, 0], [CUBE, 0, 0]], np.int32)
    got = pt.api.debug_cube_tangents(gi, np.stack([m] * 5))
    want = tr.frames(m[32:48])
    for g in (0, 2, 3):
        assert not got[g].view(np.uint32).any()
    assert beq(got[1], want) and beq(got[4], want) and got[1].any()
    assert pt.api.debug_cube_tangents(np.zeros((0, 3), np.int32), np.zeros((0, 48), f32)).shape == (0, 6, 6)


def test_bad_arguments_are_refused():
    L = pt.load_library()
    assert L.ptx_debug_cube_tangents(-1, None, None) < 0
    assert L.ptx_debug_cube_tangents(1, None, None) < 0
