"""The denoiser's guides followed through mirrors and glass (include/mi355x_pathtracer.h: ptx_set_guide_bounces; DESIGN.md 10 "Guides
through mirrors and glass") restated in numpy float32 on the CPU oracle, and the small scenes its tests use.

A guide ray's chain is built segment by segment: the segments come from the oracle's compute_intersections on paths built here, the
mirror step from the oracle's shade on a path of colour (1, 1, 1) -- that branch draws no random number, so origin, direction and
factor come out exactly -- and the glass step is restated below, one fp32 operation per operation of scatterRay's refractive branch
with its draw taken as "not reflected" (the double-precision sqrt as written).  numpy neither contracts nor reorders, so the result is
the definition's, bit for bit.  followed_samples() yields samples in the form tests/guides_ref.py's sampled_guides() takes, unchanged:
the recorded surface's point goes in as the sample's origin with a direction of -0, so that sampled_guides' o + t*d returns the point
itself (p + t * -0 = p + -0 = p for every p, -0 and +0 included) while t carries the sum of the segments' t."""
import os

import numpy as np

from guides_ref import G_OBJ, untextured_albedo

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_BASE = os.path.join(ROOT, "scenes")          # base_dir of the scenes below: "../models/cube.obj" is the repository's


# ---- the definition -------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(f32) + a[:, 2] * b[:, 2]).astype(f32)


def _reflect(I, N):
    """glm reflect: I - N * dot(N, I) * 2"""
    return (I - ((N * _dot(N, I)[:, None]).astype(f32) * f32(2.0)).astype(f32)).astype(f32)


def _refract(I, N, eta):
    """glm refract: k = 1 - eta * eta * (1 - d * d); (eta * I - (eta * d + sqrt(k)) * N) * float(k >= 0)"""
    d = _dot(N, I)
    k = (f32(1.0) - ((eta * eta).astype(f32) * (f32(1.0) - (d * d).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    f = ((eta * d).astype(f32) + np.sqrt(k).astype(f32)).astype(f32)
    r = ((I * eta[:, None]).astype(f32) - (N * f[:, None]).astype(f32)).astype(f32)
    return (r * (k >= 0).astype(f32)[:, None]).astype(f32)


def glass_step(o, d, t, n, ior, speccolor):
    """scatterRay's refractive branch (csrc/pt_device.h scatterRayT) with the draw taken as "not reflected": (origin, direction,
    colour factor) of the continued ray.  o, d, n: (N, 3); t, ior: (N,); speccolor: (N, 3); all float32."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        intersect = (o + (d * t[:, None]).astype(f32)).astype(f32)
        cos = _dot(-d, n)
        flip = cos < 0
        n = np.where(flip[:, None], (n * f32(-1.0)).astype(f32), n)
        ior1 = np.where(flip, ior, f32(1.0)).astype(f32)
        ior2 = np.where(flip, f32(1.0), ior).astype(f32)
        cos = np.where(flip, np.abs(cos), cos).astype(f32)
        sin = np.sqrt(1.0 - (cos * cos).astype(f32).astype(np.float64)).astype(f32)
        eta = (ior1 / ior2).astype(f32)
        tir = (eta * sin).astype(f32) > f32(1.0)
        nd = np.where(tir[:, None], _reflect(d, n), _refract(d, n, eta)).astype(f32)
        return (intersect + (nd * f32(0.01)).astype(f32)).astype(f32), nd, np.asarray(speccolor, f32).copy()


def followed(dump, material, geom):
    """the hits a chain continues through, budget aside: not an OBJ mesh, emittance <= 0, hasReflective > 0 or else hasRefractive > 0"""
    m = np.ascontiguousarray(dump["materials"], f32).reshape(-1, 11)[material]
    gtype = np.asarray(dump["geom_ints"], np.int32).reshape(-1, 3)[:, 0][geom]
    return (gtype != G_OBJ) & ~(m[:, 10] > 0) & ((m[:, 7] > 0) | (m[:, 8] > 0))


def follow(O, dump, paths, beff, iteration=1):
    """The chains of `paths` (cpulibs.PATH_DTYPE records: the guide rays) with at most `beff` continuations each.  Returns per-ray
    arrays: hit (N,) bool, point (N, 3) = o + t*d of the recorded surface's own segment, t (N,) = the segments' t summed in order,
    normal (N, 3), material, geom (N,) int32, T (N, 3) = the throughput on arrival, continuations (N,) int32, origin / direction
    (N, 3) of the recorded surface's own segment and seg_t (N,) its t."""
    mats = np.ascontiguousarray(dump["materials"], f32).reshape(-1, 11)
    paths = np.array(paths, copy=True)
    n = len(paths)
    T = np.ones((n, 3), f32)
    live = np.ones(n, bool)
    out = dict(hit=np.zeros(n, bool), point=np.zeros((n, 3), f32), t=np.full(n, -1, f32), normal=np.zeros((n, 3), f32),
               material=np.zeros(n, np.int32), geom=np.zeros(n, np.int32), T=np.ones((n, 3), f32), continuations=np.zeros(n, np.int32),
               origin=np.zeros((n, 3), f32), direction=np.zeros((n, 3), f32), seg_t=np.zeros(n, f32))
    for seg in range(beff + 1):
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        sub = paths[idx]
        s = O.compute_intersections(sub)
        hit = s["t"] > 0
        live[idx[~hit]] = False                          # a miss: the record stays the surface the ray left (none on the first segment)
        h, sub, s = idx[hit], sub[hit], s[hit]
        o, d, t = sub["origin"], sub["direction"], s["t"]
        out["hit"][h] = True
        out["point"][h] = (o + (t[:, None] * d).astype(f32)).astype(f32)
        out["t"][h] = t if seg == 0 else (out["t"][h] + t).astype(f32)
        out["normal"][h], out["material"][h], out["geom"][h] = s["normal"], s["materialId"], s["geomId"]
        out["T"][h] = T[h]
        out["origin"][h], out["direction"][h], out["seg_t"][h] = o, d, t
        fol = followed(dump, s["materialId"], s["geomId"]) & (seg < beff)
        live[h[~fol]] = False
        m = mats[s["materialId"]]
        refl = fol & (m[:, 7] > 0)
        refr = fol & ~refl
        if refl.any():
            q = sub[refl].copy()
            q["color"] = 1
            q["remainingBounces"] = 2                    # (neither the last bounce nor ended: shade scatters)
            q = O.shade(iteration, 0, np.arange(len(q), dtype=np.int32), s[refl], q)
            k = h[refl]
            paths["origin"][k], paths["direction"][k] = q["origin"], q["direction"]
            T[k] = (T[k] * q["color"]).astype(f32)
        if refr.any():
            no, nd, fac = glass_step(o[refr], d[refr], t[refr], s["normal"][refr], m[refr, 9], m[refr, 4:7])
            k = h[refr]
            paths["origin"][k], paths["direction"][k] = no, nd
            T[k] = (T[k] * fac).astype(f32)
        out["continuations"][h[fol]] += 1
    return out


def effective_bounces(dump, bounces):
    """Beff = min(B, traceDepth - 1), not below 0: a path of depth d has at most d segments"""
    return max(min(int(bounces), int(dump["cam_ints"][3]) - 1), 0)


def followed_samples(O, dump, iter_first, count, bounces, albedo=untextured_albedo, stats=None):
    """The guide rays of iterations iter_first .. iter_first + count - 1 followed `bounces` times at most, as samples for
    guides_ref.sampled_guides, from an oracle that holds the scene with its options set and pt_init() done (antialiasing and depth of
    field off, iter_first = count = 1: the pixel-centre mode).  stats: a list that receives each sample's follow() result."""
    beff = effective_bounces(dump, bounces)
    for it in range(iter_first, iter_first + count):
        O.pt_generate(it)
        p = O.paths()
        assert np.array_equal(p["pixelIndex"], np.arange(len(p), dtype=np.int32))
        r = follow(O, dump, p, beff, it)
        if stats is not None:
            stats.append(r)
        a = None
        if albedo is not None:
            a = (r["T"] * albedo(dump, r["material"], r["geom"], r["hit"])).astype(f32)
            a[~r["hit"]] = 0
        yield dict(origin=r["point"], direction=np.full_like(r["point"], -0.0), t=r["t"], normal=r["normal"], material=r["material"],
                   geom=r["geom"], albedo=a)


# ---- the scenes: Cornell-like boxes of cubes, x in [-5, 5], y in [0, 10], z in [-5, 5] ---------------------------------------------
def _material(i, rgb, specex=0, specrgb=(0, 0, 0), refl=0, refr=0, ior=0, emittance=0):
    return ("MATERIAL %d\nRGB         %g %g %g\nSPECEX      %g\nSPECRGB     %g %g %g\nREFL        %g\nREFR        %g\nREFRIOR     %g\n"
            "EMITTANCE   %g\n\n" % ((i,) + tuple(rgb) + (specex,) + tuple(specrgb) + (refl, refr, ior, emittance)))


def _object(i, kind, material, trans, rotat, scale):
    head = "OBJECT %d\n%s\n" % (i, kind) + ("" if material is None else "material %d\n" % material)
    return head + "TRANS       %g %g %g\nROTAT       %g %g %g\nSCALE       %g %g %g\n\n" % (tuple(trans) + tuple(rotat) + tuple(scale))


def _camera(res, depth, eye, lookat):
    return ("CAMERA\nRES         %d %d\nFOVY        45\nITERATIONS  16\nDEPTH       %d\nFILE        guides\nEYE         %g %g %g\n"
            "LOOKAT      %g %g %g\nUP          0 1 0\n\n" % (tuple(res) + (depth,) + tuple(eye) + tuple(lookat)))


LIGHT, WHITE, RED, GREEN, BLUE = 0, 1, 2, 3, 4
BASE_MATERIALS = [dict(rgb=(1, 1, 1), emittance=5), dict(rgb=(.98, .98, .98)), dict(rgb=(.85, .35, .35)), dict(rgb=(.35, .85, .35)),
                  dict(rgb=(.25, .35, .9))]
MIRROR = dict(rgb=(.98, .98, .98), specrgb=(.98, .98, .98), refl=1)
Z = (0, 0, 0)
# light, floor, ceiling, left wall, right wall
BOX = [("cube", LIGHT, (0, 10, 0), Z, (3, .3, 3)), ("cube", WHITE, (0, 0, 0), Z, (10, .01, 10)), ("cube", WHITE, (0, 10, 0), Z, (10, .01, 10)),
       ("cube", RED, (-5, 5, 0), Z, (.01, 10, 10)), ("cube", GREEN, (5, 5, 0), Z, (.01, 10, 10))]
BACK = ("cube", WHITE, (0, 5, -5), Z, (10, 10, .01))
FRONT = ("cube", BLUE, (0, 5, 5), Z, (10, 10, .01))          # the wall behind a camera that stands inside the box
OUTSIDE, INSIDE = ((0, 5, 10.5), (0, 5, 0)), ((0, 5, 4), (0, 5, 0))


def scene_text(name, res=(97, 61), depth=8):
    """(text, names): the scene and the index of every object it names, by role"""
    mats, objs, cam, names = list(BASE_MATERIALS), list(BOX), OUTSIDE, {}

    def add(role, *obj):
        names[role] = len(objs)
        objs.append(obj)

    def mat(**kw):
        mats.append(kw)
        return len(mats) - 1

    if name == "a":            # a mirror cube face-on to the camera, a coloured wall behind the camera
        cam = INSIDE
        add("back", *BACK); add("front", *FRONT)
        add("mirror", "cube", mat(**MIRROR), (0, 5, -2), Z, (4, 4, .5))
    elif name == "b":          # a glass sphere in front of a two-colour wall (the seam at x = -1, behind the sphere)
        add("wall_red", "cube", RED, (-3, 5, -5), Z, (4, 10, .01)); add("wall_green", "cube", GREEN, (2, 5, -5), Z, (6, 10, .01))
        add("glass", "sphere", mat(rgb=(.98, .98, .98), specrgb=(.85, .85, .98), refr=1, ior=1.65), (0, 5, 4), Z, (5, 5, 5))
    elif name == "c":          # two facing mirrors, the camera between them
        cam = ((0, 5, 2), (0, 5, 0))
        add("back", *BACK); add("front", *FRONT)
        m = mat(**MIRROR)
        add("mirror_far", "cube", m, (0, 5, -4), Z, (6, 6, .5)); add("mirror_near", "cube", m, (0, 5, 4), Z, (6, 6, .5))
    elif name == "d":          # a mirror that sends the camera's rays back out of the open side
        add("back", *BACK)
        add("mirror", "cube", mat(**MIRROR), (0, 5, 0), Z, (4, 4, .5))
    elif name == "e":          # a mirror material that emits, a mirror material on a mesh (set by mesh_mirror below), a plain mirror
        add("back", *BACK)
        add("emitter", "cube", mat(rgb=(.9, .8, .7), specrgb=(.98, .98, .98), refl=1, emittance=2), (-2.5, 3, 0), (0, 30, 0), (2, 2, 2))
        add("mirror", "cube", mat(**MIRROR), (0, 7.5, -1), (0, 35, 0), (3, 3, .5))
        add("mesh", "obj", None, (2.5, 3, 0), (0, 45, 0), (2, 2, 2))
    elif name == "f":          # (a) with a glossy exponent, a share below 1 and a non-white specular colour
        cam = INSIDE
        add("back", *BACK); add("front", *FRONT)
        add("mirror", "cube", mat(rgb=(.98, .98, .98), specex=4, specrgb=(.9, .6, .3), refl=.75), (0, 5, -2), Z, (4, 4, .5))
    elif name == "g":          # nothing specular
        add("back", *BACK)
        add("cube", "cube", BLUE, (-2, 3, 0), (0, 30, 0), (3, 3, 3)); add("sphere", "sphere", WHITE, (2, 4, 1), Z, (3, 3, 3))
    else:
        raise KeyError(name)
    text = "".join(_material(i, **m) for i, m in enumerate(mats)) + _camera(res, depth, *cam)
    for i, (kind, material, trans, rotat, scale) in enumerate(objs):
        text += _object(i, kind + ("\n../models/cube.obj" if kind == "obj" else ""), material, trans, rotat, scale)
    return text, names


def write_scene(directory, name, res=(97, 61), depth=8):
    """writes scene `name` into `directory`; (path, names).  Load it with base_dir=SCENE_BASE."""
    text, names = scene_text(name, res, depth)
    path = os.path.join(str(directory), "guide_bounces_%s_%dx%d_d%d.txt" % ((name,) + tuple(res) + (depth,)))
    with open(path, "w") as f:
        f.write(text)
    return path, names


def mesh_mirror(dump, names):
    """scene (e): the mesh's material (the loader takes it from the .mtl, which has no mirror) made a mirror in the dumped scene"""
    m = dump["materials"]
    k = int(dump["geom_ints"][names["mesh"]][1])
    m[k, 4:7], m[k, 7] = (.98, .98, .98), 1
    return dump
