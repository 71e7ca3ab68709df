"""The tangent frames of a cube's tabulated face normals (DScene::ctan: cube_face_tables in pt_scene.hip, tangentFrame in pt_device.h), restated
in numpy: every product, sum, square root and quotient rounded to binary32 on its own, sums left to right -- the exact arithmetic level, where
nothing is contracted.  frames(invT16) is what ptx_debug_cube_tangents hands out for one cube; choice(n) says which of the sampler's three
`notNormal` vectors a normal takes."""
import numpy as np

f32 = np.float32
SQRT_OF_ONE_THIRD = f32(0.5773502691896257645091487805019574556476)      # src/utilities.h:14, rounded to binary32 as the compiler does


def dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def cross(x, y):
    return (f32(f32(x[1] * y[2]) - f32(y[1] * x[2])), f32(f32(x[2] * y[0]) - f32(y[2] * x[0])), f32(f32(x[0] * y[1]) - f32(y[0] * x[1])))


def normalize(a):
    r = f32(f32(1.0) / np.sqrt(dot(a, a), dtype=f32))            # glm's inversesqrt: 1 / sqrt, two roundings
    return (f32(a[0] * r), f32(a[1] * r), f32(a[2] * r))


def choice(n):
    """0, 1, 2: notNormal is the x, y, z axis"""
    if abs(n[0]) < SQRT_OF_ONE_THIRD:
        return 0
    if abs(n[1]) < SQRT_OF_ONE_THIRD:
        return 1
    return 2


def tangent_frame(n):
    not_normal = [(f32(1), f32(0), f32(0)), (f32(0), f32(1), f32(0)), (f32(0), f32(0), f32(1))][choice(n)]
    perp1 = normalize(cross(n, not_normal))
    perp2 = normalize(cross(n, perp1))
    return perp1, perp2


def cube_normals(invT16):
    """the six normals of cnorm, side = axis * 2 + (sign > 0): normalize(invTranspose * (+-e_axis, 0)), the matrix as 16 floats by columns.
    (rows 0-2 of the matrix times the vector as mulRows does it: (r0 x + r1 y) + (r2 z + r3 w))"""
    m = np.asarray(invT16, f32)
    out = []
    for side in range(6):
        e = [f32(0)] * 3
        e[side >> 1] = f32(1.0 if side & 1 else -1.0)
        v = tuple(f32(f32(f32(m[0 * 4 + r] * e[0]) + f32(m[1 * 4 + r] * e[1])) + f32(f32(m[2 * 4 + r] * e[2]) + f32(m[3 * 4 + r] * f32(0)))) for r in range(3))
        out.append(normalize(v))
    return out


def frames(invT16):
    """(6, 6) float32: per side perp1 xyz, perp2 xyz"""
    out = np.zeros((6, 6), f32)
    with np.errstate(all="ignore"):
        for side, n in enumerate(cube_normals(invT16)):
            p1, p2 = tangent_frame(n)
            out[side, :3], out[side, 3:] = p1, p2
    return out
