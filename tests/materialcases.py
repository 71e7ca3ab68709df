"""Scene texts over the material parameter space, shared by tests/test_materials_cpu.py (oracle against the reference and the fixtures)
and tests/test_gpu_materials.py (the bounce kernels against the oracle).  Plain builders, everything from fixed seeds.

A material is the tuple of its file fields in file order: RGB 3, SPECEX, SPECRGB 3, REFL, REFR, REFRIOR, EMITTANCE -- which is also the
order of the 11 floats a loader dump holds per material.

zoo_text: the lit box of the fuzzers with 25 random cubes and spheres and one models/cube.obj, 32 geoms (the fast path with candidate
masks applies), 18 materials + the mesh's own.  The material order makes record_masks' direction rule ask for three runs of bins
(4-12, 15-16, the mesh's), so its gap-filling loop runs.  single_text: the same box around one sphere, one rotated cube and a second
sphere that share the material under test.  GRID / NONFINITE: the materials single_text is run with."""
import numpy as np

CAMERA = "CAMERA\nRES %d %d\nFOVY 45\nITERATIONS 10\nDEPTH %d\nFILE materials\nEYE 0.0 5 10.5\nLOOKAT 0 5 0\nUP 0 1 0\n\n"
MAT = "MATERIAL %d\nRGB %s %s %s\nSPECEX %s\nSPECRGB %s %s %s\nREFL %s\nREFR %s\nREFRIOR %s\nEMITTANCE %s\n\n"

# light, floor, ceiling, back wall, red wall, green wall: materials 0, 1, 1, 1, 2, 3
BOX = ["cube\nmaterial 0\nTRANS 0 10 0\nROTAT 0 0 0\nSCALE 4 .3 4", "cube\nmaterial 1\nTRANS 0 0 0\nROTAT 0 0 0\nSCALE 11 .01 11",
       "cube\nmaterial 1\nTRANS 0 10 0\nROTAT 0 0 90\nSCALE .01 11 11", "cube\nmaterial 1\nTRANS 0 5 -5\nROTAT 0 90 0\nSCALE .01 11 11",
       "cube\nmaterial 2\nTRANS -5 5 0\nROTAT 0 0 0\nSCALE .01 11 11", "cube\nmaterial 3\nTRANS 5 5 0\nROTAT 0 0 0\nSCALE .01 11 11"]


def material(rgb=(.9, .9, .9), specex=0, specrgb=(0, 0, 0), refl=0, refr=0, ior=0, emit=0):
    return tuple(rgb) + (specex,) + tuple(specrgb) + (refl, refr, ior, emit)


def materials_text(mats):
    return "".join(MAT % ((i,) + tuple("%.9g" % float(v) for v in m)) for i, m in enumerate(mats))


def scene_text(mats, objects, res, depth):
    return materials_text(mats) + CAMERA % (res[0], res[1], depth) + "".join("OBJECT %d\n%s\n\n" % (i, o) for i, o in enumerate(objects))


W = (.95, .95, .95)
ZOO_MATERIALS = [
    material((1, 1, 1), emit=5),                                              # 0  light
    material((.9, .9, .9)),                                                   # 1  white diffuse
    material((.8, .3, .3)),                                                   # 2  red diffuse
    material((.3, .8, .3)),                                                   # 3  green diffuse
    material(W, 0, W, refl=1),                                                # 4  mirror
    material(W, 20.5, (.95, .8, .6), refl=1),                                 # 5  glossy mirror, coloured specular
    material(W, 3, (.7, .9, .95), refl=.5),                                   # 6  half-strength glossy
    material(W, 0, (.9, .9, .95), refl=1, refr=1, ior=1.5),                   # 7  reflective and refractive: reflective wins
    material(W, 0, (.9, .95, .9), refr=1, ior=1),                             # 8  refractive, index 1
    material(W, 0, (.95, .9, .9), refr=1, ior=.75),                           # 9  refractive, index below 1
    material(W, 0, (.8, .85, .95), refr=.3, ior=2.4),                         # 10 fractional refractive
    material(W, 0, (.85, .95, .8), refl=-1, refr=1, ior=1.5),                 # 11 negative reflective: falls through to refraction
    material(W, 0, (.9, .9, .9), refl=1, emit=2),                             # 12 emitting mirror
    material((.6, .7, .9), emit=-1),                                          # 13 negative emittance: no light
    material((.9, .8, .5), emit=.25),                                         # 14 dim second light
    material(W, .5, (.9, .85, .95), refl=1),                                  # 15 fractional exponent
    material(W, 200, (.95, .95, .85), refl=1),                                # 16 large exponent
    material((0, 0, 0)),                                                      # 17 black diffuse
]
ZOO_OBJ_MATERIAL = len(ZOO_MATERIALS)          # the loaders append the mesh's own material
ZOO_DIRECTION_MATERIALS = [4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, ZOO_OBJ_MATERIAL]
# (kind, material) of the 25 random primitives.  Non-diffuse: 15, 16 on cubes only, 5, 8, 11 on spheres only, 4, 6, 7, 9, 10, 12 on both;
# diffuse: the box's on cubes only, 13 on spheres only, 14 and 17 on both.  The materials that only cubes have make two runs of bins
# (0-3 and 15-16), which record_masks keeps: the box's records travel with a normal code, 13's, 14's and 17's with their normal.
ZOO_PRIMITIVES = [("cube", 4), ("sphere", 4), ("sphere", 5), ("sphere", 5), ("cube", 6), ("sphere", 6), ("sphere", 7), ("cube", 7),
                  ("sphere", 8), ("sphere", 8), ("cube", 9), ("sphere", 9), ("sphere", 10), ("cube", 10), ("sphere", 11), ("cube", 12),
                  ("sphere", 12), ("sphere", 13), ("sphere", 13), ("cube", 14), ("sphere", 14), ("cube", 15), ("cube", 16), ("cube", 17),
                  ("sphere", 17)]
ZOO_SEED = 0
ZOO_MIN_RECORDS = 50          # every material is the hit material of at least this many records of iteration 1 at 96 x 72


def zoo_objects(seed=None):
    rng = np.random.default_rng(20261020 + (ZOO_SEED if seed is None else seed))
    prims = [ZOO_PRIMITIVES[i] for i in rng.permutation(len(ZOO_PRIMITIVES))]
    heads = ["%s\nmaterial %d" % p for p in prims]
    heads.insert(int(rng.integers(0, len(heads))), "obj\n../models/cube.obj")
    objs = list(BOX)
    for head in heads:
        pos = rng.uniform([-3.8, 0.8, -3.8], [3.8, 8.2, 3.2])
        rot = rng.uniform(-180, 180, 3)
        sc = rng.uniform(0.7, 1.8, 3)
        objs.append(head + "\nTRANS %.4f %.4f %.4f\nROTAT %.3f %.3f %.3f\nSCALE %.4f %.4f %.4f" % (tuple(pos) + tuple(rot) + tuple(sc)))
    assert len(objs) == 32
    return objs


def zoo_text(res=(96, 72), depth=8, seed=None):
    return scene_text(ZOO_MATERIALS, zoo_objects(seed), res, depth)


def single_text(mat, res=(48, 36), depth=8):
    """light, white, red, green and the material under test (4) on a sphere, a rotated cube and a second sphere"""
    mats = ZOO_MATERIALS[:4] + [tuple(mat)]
    objs = BOX + ["sphere\nmaterial 4\nTRANS -1.6 3.8 -0.5\nROTAT 0 0 0\nSCALE 3.6 3.6 3.6",
                  "cube\nmaterial 4\nTRANS 2.2 2.4 0.8\nROTAT 15 35 -20\nSCALE 2.2 3.6 2",
                  "sphere\nmaterial 4\nTRANS 1.2 7 -2\nROTAT 40 10 70\nSCALE 2.6 1.6 2.2"]
    return scene_text(mats, objs, res, depth)


def _grid():
    spec = (.95, .85, .7)
    g = []
    for ex in (0, .5, 1, 2, 20.5, 200, 1e4):
        for refl in (.25, 1, 3):
            g.append(("specex%g-refl%g" % (ex, refl), material(W, ex, spec, refl=refl)))
    for ior in (0, .25, .5, .75, 1, 1.0001, 1.33, 2.4, 10, 1e6, -1.5):
        for refr in (.3, 1):
            g.append(("ior%g-refr%g" % (ior, refr), material(W, 0, spec, refr=refr, ior=ior)))
    g += [("refl1-refr1-specex2", material(W, 2, spec, refl=1, refr=1, ior=1.5)),
          ("refl1-emit3", material(W, 0, spec, refl=1, emit=3)),
          ("refr1-emit3", material(W, 0, spec, refr=1, ior=1.5, emit=3)),
          ("emit-2", material(W, emit=-2)),
          ("refl-1-refr-1", material(W, 0, spec, refl=-1, refr=-1, ior=1.5)),
          ("rgb-above-1", material((1.5, 1.2, 1))),
          ("emit1e-30", material(W, emit=1e-30))]
    return g


GRID = _grid()
NONFINITE = [("specex-1-refl1", material(W, -1, (.95, .85, .7), refl=1)), ("specex-20.5-refl1", material(W, -20.5, (.95, .85, .7), refl=1))]
assert len(GRID) == 50 and len({n for n, _ in GRID + NONFINITE}) == 52


def hit_counts(O, nmat, it=1):
    """records per hit material in the sorted streams of iteration `it`, summed over the bounces, from an oracle that holds the scene
    with its options set and pt_init() done"""
    counts = np.zeros(nmat, np.int64)
    O.pt_generate(it)
    while True:
        n = O.num_paths()
        O.pt_bounce(it, 3)
        s = O.isects()[:n]
        counts += np.bincount(s["materialId"][s["t"] > 0], minlength=nmat)
        if O.pt_bounce(it, 12) == 0:
            break
    return counts
