"""The denoiser's parameter grid: the cases tests/test_denoise_grid_cpu.py proves well conditioned (with the float32 probe of
tests/denoise_f32.py) and tests/test_gpu_denoise_grid.py then runs on the device against the float64 restatements.

Three kernel families: "plain" (ptx_denoise_buffers: k_atrous_pass<false, *>), "given" (ptx_denoise_buffers_variance with a variance:
k_atrous_pass<true, *>) and "spatial" (the same without one: k_variance_spatial in front).  Shapes sit on the 64 x 4 workgroup and on the
tap steps, hit masks on the workgroup's early exits and aprons; every parameter is swept one at a time around the defaults on (9, 130),
and a seeded set of random combinations follows.

Conditioning.  The luminance weight's constant is log2 e / (phi_luminance sqrt(g) + epsilon): as that denominator ("sigma") goes to 0 one
float32 ulp of a luminance difference moves a weight by more than the bound the device is held to, so a correct kernel cannot meet it.
The prefilter keeps g away from 0 (it averages nine neighbours) unless phi_luminance is small as well.  Hence:
  * prefilter = 1 and phi_luminance >= 1: random_frame as it is (albedo 0, colour 40), a given variance with exact zeros;
  * prefilter = 0 or phi_luminance < 1: tame_frame (albedo >= 0.25, colour <= 1.5, normals and positions that change by blocks and not by
    pixel, so that the spatial estimate sees a full window) and a given variance of SIGMA_FLOOR^2 / phi_luminance^2 at the least, i.e.
    phi_luminance sqrt(v0) >= SIGMA_FLOOR going in.  tests/test_denoise_grid_cpu.py states the probe figures that led to SIGMA_FLOOR.
The spatial estimate cannot be floored; its ill-conditioned cases use tame_frame with its 85 % mask, and one or two passes (every pass
shrinks v by up to (sum b^2)^2 = 0.075)."""
import numpy as np

from atrous_ref import random_frame

# (h, w): the smallest frame; one short of a tile's width and under its height; one tile; one pixel into a second tile both ways; whole
# tiles only; taps at +-64 inside the frame (step 32, passes = 6); tall and thin; taps at +-512 (step 256, passes = 9) and at +-1024
# (step 512, passes = 10) inside the frame
SHAPES = [(1, 1), (3, 63), (4, 64), (5, 65), (8, 128), (9, 130), (70, 2), (3, 1100), (2, 2100)]
MASK_SHAPES = [(5, 65), (9, 130)]
MASKS = ["random", "all_hit", "all_miss", "single", "checker", "hole_tile", "last_tile"]
MULTI_TILE = [s for s in SHAPES if s[0] > 4 or s[1] > 64]

VALUES = dict(passes=[1, 2, 5, 6, 8, 10], demodulate=[0, 1], phi_color=[0.25, 16.0, 1e3], phi_normal=[0.005, 0.1, 10.0],
              phi_position=[0.01, 0.5, 50.0], phi_luminance=[0.25, 1.0, 4.0, 64.0], epsilon=[1e-8, 1e-4, 1.0], spatial_radius=[1, 2, 3],
              prefilter=[0, 1])
DEFAULTS = dict(passes=5, demodulate=1, phi_color=16.0, phi_normal=0.1, phi_position=0.5, phi_luminance=4.0, epsilon=1e-4,
                spatial_radius=3, prefilter=1)
PLAIN_KEYS = ("passes", "demodulate", "phi_color", "phi_normal", "phi_position")
VAR_KEYS = ("passes", "demodulate", "phi_normal", "phi_position", "phi_luminance", "epsilon", "spatial_radius", "prefilter")

SIGMA_FLOOR = 1.0           # phi_luminance sqrt(v0) of the ill-conditioned corner's given variances is at least this


def f32(v):
    """the value the library sees: ptx_denoise_params and ptx_variance_params hold floats"""
    return float(np.float32(v))


def mask(name, h, w, seed):
    m = np.zeros((h, w), bool)
    if name == "random":
        return None                                      # the frame's own 85 % mask
    if name == "all_hit":
        m[:] = True
    elif name == "single":
        m[h // 2, w - 2] = True
    elif name == "checker":
        m[(np.add.outer(np.arange(h), np.arange(w)) & 1) == 0] = True
    elif name == "hole_tile":                            # the first 64 x 4 tile has no hit of its own, its apron has
        m[:] = True
        m[:4, :64] = False
    elif name == "last_tile":                            # only the last, partial tile has hits
        m[(h - 1) // 4 * 4:, (w - 1) // 64 * 64:] = True
    elif name != "all_miss":
        raise ValueError(name)
    return m


def tame_frame(h, w, seed):
    """random_frame without what the ill-conditioned corner cannot take: albedo in [0.25, 1], colour in [0.15, 1.5], and guides that are
    constant over blocks of 17 columns (one normal, a position ramp without noise), so that neighbours weigh about 1"""
    f = random_frame(h, w, seed)
    rng = np.random.default_rng(seed + 77)
    normals = np.array([[0, 0, 1], [1, 0, 0], [0, 0.6, 0.8]], np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    f["normal"] = normals[(xx // 17).astype(int) % 3]
    f["position"] = np.stack([xx * 0.04, yy * 0.04, (xx // 17) * 0.7], -1).astype(np.float32)
    f["albedo"] = (0.25 + 0.75 * rng.random((h, w, 3))).astype(np.float32)
    f["rgb"] = (0.15 + 1.35 * rng.random((h, w, 3))).astype(np.float32)
    return f


class Case:
    def __init__(self, family, shape, mask="random", seed=0, ids=False, tame=False, **params):
        assert family in ("plain", "given", "spatial")
        self.family, self.shape, self.mask, self.seed, self.ids, self.tame = family, tuple(shape), mask, seed, bool(ids), bool(tame)
        keys = PLAIN_KEYS if family == "plain" else VAR_KEYS
        assert set(params) <= set(keys), params
        self.params = {k: (f32(params.get(k, DEFAULTS[k])) if isinstance(DEFAULTS[k], float) else int(params.get(k, DEFAULTS[k])))
                       for k in keys}
        self.sensitive = family != "plain" and (self.params["prefilter"] == 0 or self.params["phi_luminance"] < 1.0)
        if self.sensitive:
            self.tame = True

    @property
    def id(self):
        p = ",".join("%s=%g" % (k, v) for k, v in self.params.items() if v != (f32(DEFAULTS[k]) if isinstance(DEFAULTS[k], float) else DEFAULTS[k]))
        return "%s-%dx%d-%s%s%s-s%d%s" % (self.family, self.shape[0], self.shape[1], self.mask, "-ids" if self.ids else "",
                                         "-tame" if self.tame else "", self.seed, "-" + p if p else "")

    def build(self):
        """(frame dict of random_frame's keys, ids or None, variance or None)"""
        h, w = self.shape
        f = (tame_frame if self.tame else random_frame)(h, w, 1000 * h + w + self.seed)
        m = mask(self.mask, h, w, self.seed)
        if m is not None:
            f["hit"] = m
        rng = np.random.default_rng(7 * h + w + self.seed)
        ids = rng.integers(0, 2, (h, w, 2)).astype(np.int32) if self.ids else None
        var = None
        if self.family == "given":
            var = (rng.random((h, w)) * 0.3).astype(np.float32)
            if self.sensitive:
                var += np.float32((SIGMA_FLOOR / self.params["phi_luminance"]) ** 2)
            else:
                var[rng.random((h, w)) < 0.05] = 0.0
        return f, ids, var


def _sweeps(family, keys, base, **fixed):
    out = []
    for k in keys:
        for v in VALUES[k]:
            if v != DEFAULTS[k]:
                out.append(Case(family, base, **dict(fixed, **{k: v})))
    return out


def _random(family, keys, n, seed, shapes):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        prm = {k: VALUES[k][rng.integers(len(VALUES[k]))] for k in keys}
        if family == "spatial" and (prm["prefilter"] == 0 or prm["phi_luminance"] < 1.0):
            prm["passes"] = min(prm["passes"], 2)
        out.append(Case(family, shapes[i % len(shapes)], seed=i + 1, ids=bool(rng.integers(2)), **prm))
    return out


def _cases():
    big = (9, 130)
    # passes at which the shape's taps reach their largest unclamped step (SHAPES)
    deep = {(9, 130): 6, (3, 1100): 9, (2, 2100): 10, (70, 2): 6}
    rand_shapes = [(9, 130), (5, 65), (8, 128), (3, 63), (70, 2), (3, 1100)]
    cs = [Case("plain", big)]
    cs += _sweeps("plain", PLAIN_KEYS, big)
    cs += [Case("plain", s, seed=1, passes=deep.get(s, 5)) for s in SHAPES]
    cs += [Case("plain", s, m, passes=6 if m == "checker" else 5) for s in MASK_SHAPES for m in MASKS[1:]]
    cs += _random("plain", PLAIN_KEYS, 10, 11, rand_shapes)

    cs += [Case("given", big)]
    cs += _sweeps("given", [k for k in VAR_KEYS if k != "spatial_radius"], big)
    cs += [Case("given", s, seed=1, passes=deep.get(s, 5)) for s in SHAPES]
    cs += [Case("given", s, seed=2, prefilter=0, passes=deep.get(s, 5)) for s in [(5, 65), (8, 128), (70, 2), (2, 2100)]]
    cs += [Case("given", s, m) for s in MASK_SHAPES for m in MASKS[1:]]
    cs += [Case("given", s, m, prefilter=0) for s in MASK_SHAPES for m in ("checker", "hole_tile")]
    cs += _random("given", [k for k in VAR_KEYS if k != "spatial_radius"], 8, 12, rand_shapes)

    # the radius through the one-pass, prefilter = 1 output (v0 goes through it undamped), with and without ids
    cs += [Case("spatial", big, ids=ids, passes=1, spatial_radius=r) for r in (1, 2, 3) for ids in (False, True)]
    cs += [Case("spatial", big, ids=True)]
    cs += _sweeps("spatial", [k for k in VAR_KEYS if k not in ("prefilter", "phi_luminance")], big, ids=True)
    cs += [Case("spatial", big, passes=2, phi_luminance=v) for v in (0.25, 1.0, 64.0)]
    cs += [Case("spatial", s, passes=p, prefilter=0, spatial_radius=r) for s, p, r in (((9, 130), 1, 3), ((5, 65), 2, 1), ((8, 128), 1, 2))]
    cs += [Case("spatial", s, seed=1, ids=i % 2 == 1, passes=min(deep.get(s, 5), 6), spatial_radius=1 + i % 3) for i, s in enumerate(SHAPES)]
    cs += [Case("spatial", s, m, ids=i % 2 == 1, spatial_radius=1 + (i + j) % 3, passes=1 if m in ("single", "last_tile") else 5)
           for j, s in enumerate(MASK_SHAPES) for i, m in enumerate(MASKS[1:])]
    cs += _random("spatial", VAR_KEYS, 8, 13, rand_shapes)
    seen = {}
    for c in cs:                                         # (a sweep's value may be one of the listed cases already)
        seen.setdefault(c.id, c)
    return list(seen.values())


CASES = _cases()


def of_family(family):
    return [c for c in CASES if c.family == family]


_REFERENCE = {}


def reference(case):
    """(the five frame arrays, ids, variance, the float64 restatement's colour, its variance or None) of a case: computed once, shared by
    every test of a run and read-only"""
    from atrous_ref import atrous
    from variance_ref import denoise_buffers_variance
    if case.id not in _REFERENCE:
        f, ids, var = case.build()
        args = (f["rgb"], f["albedo"], f["normal"], f["position"], f["hit"])
        if case.family == "plain":
            c, v = atrous(*args, **case.params), None
        else:
            c, v, _ = denoise_buffers_variance(*args, ids=ids, variance=var, **case.params)
        for a in args + (ids, var, c, v):
            if a is not None:
                a.setflags(write=False)
        _REFERENCE[case.id] = (args, ids, var, c, v)
    return _REFERENCE[case.id]
