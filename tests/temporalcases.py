"""The reprojection's parameter grid: the cases tests/test_temporal_grid_cpu.py proves well conditioned (with the float32 probe of
tests/temporal_f32.py) and tests/test_gpu_temporal_grid.py then runs on the device, through ptx_kat_reproject, against the float64
restatements (temporal_ref.reproject / mix, variance_ref.temporal_variance, temporal_measured_ref.temporal_measured_variance).

One case is one frame with its hist state and hist camera; every case runs through the three kernels (variant 0 plain, 1 variance,
2 measured).  The guides are synthetic and need not be physically consistent.  A pinhole at (0, 0, 10) looks down -z at the plane z = 0,
a pixel is PX = 0.02 wide there.  Every guide is a function of the world (x, y) a camera's pixel-centre ray has on that plane, so the
hist camera's pixels carry what the current pixels that reproject onto them carry.  Six bands across the frame (BANDS) differ in geom
id, material id (one specular, one -1, one == nmats), normal (axis-aligned and tilted) and depth (z = 0 or 0.5); the upper half of the
frame has other geom ids.  In a horizontal strip hist's positions are 0.25 further along z: the plane test rejects those taps at the
default tolerance and accepts them at 0.5.

Conditioning.  A bilinear result carries delta_u (D_q+1 - D_q): hist's D, V and n are smooth in the world position (under 5 % from one
pixel to the next) within a band, and jump by a factor between bands, so that a tap taken from the wrong side of an id, normal or
plane test moves the result by 10 % or more.  Albedo is 0.25 at the least, the scatter matrices are sums of positive vectors' outer
products (no cancellation in g^T M g).  Frames are 260 wide at the most: the float32 error of u grows with u.

`exact` cases sit on the thresholds normal_cos = 1 and plane_tolerance = 0: every normal is (0, 0, 1) and every z is 0, 0.25, 0.5 or 0.75,
so that the compared quantities are exact in binary32 and both precisions decide alike; their `near` leaves out the two threshold terms.
"""
import numpy as np

import temporal_ref as T
from denoisecases import f32, mask
from moments_ref import from_cov6
from temporal_measured_ref import temporal_measured_variance
from variance_ref import temporal_variance

# (h, w): as tests/denoisecases.py's, without the frames too wide for `near` to judge; (6, 257): an odd width over four waves
SHAPES = [(1, 1), (3, 63), (4, 64), (5, 65), (8, 128), (9, 130), (70, 2), (6, 257)]
BASE = (9, 130)
MASK_SHAPES = [(5, 65), (9, 130)]
MASKS = ["random", "all_hit", "all_miss", "single", "checker", "hole_tile", "last_tile"]
# (current, hist): every mask on either side once, and the pairs in which both sides have few hits
MASK_PAIRS = [("all_hit", "all_miss"), ("all_miss", "all_hit"), ("all_hit", "single"), ("single", "all_hit"), ("checker", "checker"),
              ("random", "checker"), ("hole_tile", "random"), ("random", "hole_tile"), ("last_tile", "all_hit"), ("all_hit", "last_tile"),
              ("last_tile", "last_tile"), ("all_hit", "all_hit")]

VALUES = dict(max_history=[0, 1, 3, 16], specular_history=[0, 1], normal_cos=[-1.0, 0.5, 0.9, 1.0], plane_tolerance=[0.0, 0.01, 0.5],
              spp=[1, 2, 7], batches=[2, 4, 9], has_v=[0, 1])
DEFAULTS = dict(max_history=16, specular_history=0, normal_cos=0.9, plane_tolerance=0.01, spp=2, batches=4, has_v=1)
TEMPORAL_KEYS = ("max_history", "specular_history", "normal_cos", "plane_tolerance")

# hist cameras: the moves that leave a projection (CAMERAS) and the three that leave none
CAMERAS = ["subpixel", "pan", "lose_third", "dolly", "roll", "aniso", "skew"]
NOTHING = ["none", "singular", "behind"]

NMATS = 4
SPEC = np.array([0, 0, 1, 0], np.uint8)                  # material 2 is specular
DIST, PX = 10.0, 0.02
PL = PX / DIST
#        geom, material, normal, z, factor of hist's D / V / n
BANDS = [(2, 1, (0.0, 0.0, 1.0), 0.0, 1.0),
         (2, 1, (0.0, 0.6, 0.8), 0.0, 1.5),              # the same ids, another normal: dot = 0.8
         (3, 1, (0.0, 0.6, 0.8), 0.0, 0.7),              # the same material and normal, another geom
         (3, 2, (0.0, 0.0, 1.0), 0.5, 1.2),              # the same geom, another material: the specular one
         (4, -1, (0.6, 0.0, 0.8), 0.5, 0.9),
         (5, NMATS, (0.0, 0.0, 1.0), 0.0, 1.3)]
UPPER_GEOM, UPPER_FACTOR = 10, 1.15
ALT_BAND, ALT_FACTOR = 1, 1.25
STRIP, STRIP_DZ = (0.2, 0.45), 0.25                      # hist's displaced strip, in frame heights


def _round(cam):
    """the camera the library sees: ptx_camera holds floats"""
    return {k: (np.asarray(v, np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}


def base_camera(h, w):
    return _round(dict(position=np.array([0.0, 0.0, DIST]), view=np.array([0.0, 0.0, -1.0]), right=np.array([1.0, 0.0, 0.0]),
                       up=np.array([0.0, 1.0, 0.0]), pl=np.array([PL, PL]), W=w, H=h))


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(3)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def hist_camera(kind, h, w):
    """camera_dict of the hist camera, None for "none"; pans are in pixels of the plane z = 0"""
    if kind == "none":
        return None
    c = base_camera(h, w)
    move = dict(subpixel=(0.37, 0.21, 0.0), pan=(3.3, 0.4, -0.8), lose_third=(0.34 * w + 0.3, 0.27, 0.0), dolly=(2.3, 1.2, -0.93),
                roll=(0.4, 0.3, 0.0), aniso=(0.3, 0.2, 0.0), skew=(0.45, 0.15, 0.0), singular=(0.37, 0.21, 0.0), behind=(0.37, 0.21, -2 * DIST))[kind]
    c["position"] = c["position"] + np.array([move[0] * PX, move[1] * PX, move[2]])
    r = np.eye(3)
    if kind == "pan":                                    # small yaw and pitch, and a roll that spreads v over both edges of the frame
        r = _rot(1, 0.003) @ _rot(0, 0.002) @ _rot(2, 0.02)
    if kind == "roll":
        r = _rot(2, np.radians(10.0))
    for k in ("view", "right", "up"):
        c[k] = r @ c[k]
    if kind == "aniso":
        c["pl"] = c["pl"] * np.array([1.07, 0.93])
    if kind == "skew":                                   # right and up neither orthogonal nor of one length
        c["right"] = c["right"] + 0.1 * c["up"]
        c["up"] = 0.95 * c["up"] - 0.05 * c["right"]
    if kind == "singular":
        c["right"] = np.zeros(3)
    return _round(c)


def world_xy(cam):
    """(H, W, 2): where the pixel-centre rays of `cam` meet z = 0"""
    y, x = np.mgrid[0:cam["H"], 0:cam["W"]].astype(np.float64)
    d = (cam["view"] - cam["right"] * cam["pl"][0] * (x - cam["W"] / 2.0)[..., None]
         - cam["up"] * cam["pl"][1] * (y - cam["H"] / 2.0)[..., None])
    t = -cam["position"][2] / d[..., 2]
    return (cam["position"] + t[..., None] * d)[..., :2]


def _smooth(xy, k, lo, hi):
    """a field in [lo, hi] that changes by under 2 % of hi - lo per pixel"""
    x, y = xy[..., 0], xy[..., 1]
    return lo + (hi - lo) * (0.5 + 0.5 * np.sin(1.1 * x + 0.7 * y + 1.3 * k) * np.cos(0.5 * y - 0.4 * k))


def _count(xy):
    """hist's sample counts: 0.5 to 40, fractional, flat where they are small"""
    return 0.5 + 39.5 * (0.5 + 0.5 * np.sin(2.2 * xy[..., 0] + 0.9 * xy[..., 1]))


def guides(xy, h, w, exact):
    """the G-buffer at world (x, y) (float32 arrays), the band factor, and the strip flag"""
    tx, ty = xy[..., 0] / (PX * w) + 0.5, xy[..., 1] / (PX * h) + 0.5
    band = np.clip(np.floor(tx * len(BANDS)), 0, len(BANDS) - 1).astype(int)
    upper = ty > 0.5
    pick = lambda i: np.array([b[i] for b in BANDS])[band]
    normal = pick(2).astype(np.float32)
    alt = (band == ALT_BAND) & (np.floor(ty * 4) % 2 == 1)                # band 1 in stripes: the normal test along rows too
    normal[alt] = (0.0, 0.0, 1.0)
    if exact:
        normal = np.zeros(xy.shape[:-1] + (3,), np.float32)
        normal[..., 2] = 1.0
    pos = np.concatenate([xy, pick(3)[..., None]], -1).astype(np.float32)
    g = dict(position=pos, normal=normal, material=pick(1).astype(np.int32), geom=(pick(0) + UPPER_GEOM * upper).astype(np.int32))
    return g, pick(4) * np.where(upper, UPPER_FACTOR, 1.0) * np.where(alt, ALT_FACTOR, 1.0), (ty >= STRIP[0]) & (ty < STRIP[1])


def _mask(name, h, w, rng):
    m = mask(name, h, w, 0)
    return rng.random((h, w)) < 0.85 if m is None else m


class Case:
    def __init__(self, shape, camera="pan", masks=("random", "random"), seed=0, exact=False, poison=False, **params):
        assert camera in CAMERAS + NOTHING and set(params) <= set(DEFAULTS), (camera, params)
        self.shape, self.camera, self.masks, self.seed = tuple(shape), camera, tuple(masks), seed
        self.exact, self.poison = bool(exact), bool(poison)
        self.params = {k: (f32(params.get(k, v)) if isinstance(v, float) else int(params.get(k, v))) for k, v in DEFAULTS.items()}
        if self.params["normal_cos"] == 1.0 or self.params["plane_tolerance"] == 0.0:
            self.exact = True                            # on a threshold: only frames that are exact in binary32

    @property
    def tparams(self):
        return {k: self.params[k] for k in TEMPORAL_KEYS}

    @property
    def id(self):
        p = ",".join("%s=%g" % (k, v) for k, v in self.params.items() if v != (f32(DEFAULTS[k]) if isinstance(DEFAULTS[k], float) else DEFAULTS[k]))
        return "%dx%d-%s-%s/%s%s%s-s%d%s" % (self.shape[0], self.shape[1], self.camera, self.masks[0], self.masks[1],
                                             "-exact" if self.exact else "", "-poison" if self.poison else "", self.seed, "-" + p if p else "")

    def build(self):
        """dict: cur (the G-buffer, Tracer.gbuffer()'s keys), rgb, hist_cam (camera_dict or None), prev (temporal_ref.state's layout
        with V), scatter (H, W, 6); float32 / int32 / bool arrays, as the library takes them"""
        h, w = self.shape
        rng = np.random.default_rng(1000 * h + w + 17 * self.seed)
        cur, _, _ = guides(world_xy(base_camera(h, w)), h, w, self.exact)
        cur["hit"] = _mask(self.masks[0], h, w, rng)
        cur["albedo"] = (0.25 + 0.75 * rng.random((h, w, 3))).astype(np.float32)
        spp = self.params["spp"]
        rgb = (spp * (0.1 + 0.9 * rng.random((h, w, 3)))).astype(np.float32)
        cam = hist_camera(self.camera, h, w)
        # (a camera without a projection: hist's guides are those of the sub-pixel pan)
        hxy = world_xy(cam if self.camera in CAMERAS else hist_camera("subpixel", h, w))
        pg, factor, strip = guides(hxy, h, w, self.exact)
        pg["position"][..., 2] += np.float32(STRIP_DZ) * strip
        pg["hit"] = _mask(self.masks[1], h, w, rng)
        D = np.stack([_smooth(hxy, k, 0.45, 0.9) for k in range(3)], -1) * factor[..., None]
        prev = dict(gbuf=pg, D=D.astype(np.float32), n=(_count(hxy) * np.minimum(factor, 1.0)).astype(np.float32),
                    V=(_smooth(hxy, 4, 0.03, 0.08) * factor).astype(np.float32))
        B = self.params["batches"]
        x = 0.05 + 0.25 * rng.random((B, h, w, 3))       # the batch means' deviations, all positive
        scatter = np.stack([(x[..., i] * x[..., j]).sum(0) for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))], -1).astype(np.float32)
        poisoned = np.zeros((h, w), bool)
        if self.poison:
            bad = [np.nan, np.inf, -np.inf]
            for k, i in enumerate(rng.choice(h * w, 12, replace=False)):
                y, xx = divmod(int(i), w)
                if k < 6:                                # the current frame: positions and normals
                    (cur["position"] if k % 2 else cur["normal"])[y, xx, k % 3] = bad[k % 3]
                    cur["hit"][y, xx] = True
                    poisoned[y, xx] = True
                else:                                    # hist: NaN in normals, NaN and inf in positions
                    if k % 2:
                        pg["position"][y, xx, k % 3] = bad[k % 3]
                    else:
                        pg["normal"][y, xx, k % 3] = np.nan
                    pg["hit"][y, xx] = True
        return dict(cur=cur, rgb=rgb, hist_cam=cam, prev=prev, scatter=scatter, poisoned=poisoned)


def _sweeps(keys):
    out = []
    for k in keys:
        for v in VALUES[k]:
            if v != DEFAULTS[k]:
                out.append(Case(BASE, **{k: v}))
    return out


def _random(n, seed):
    rng = np.random.default_rng(seed)
    shapes = [(9, 130), (5, 65), (8, 128), (3, 63), (70, 2), (6, 257)]
    out = []
    for i in range(n):
        prm = {k: VALUES[k][rng.integers(len(VALUES[k]))] for k in VALUES}
        out.append(Case(shapes[i % len(shapes)], CAMERAS[rng.integers(len(CAMERAS))],
                        (MASKS[rng.integers(len(MASKS))], MASKS[rng.integers(len(MASKS))]), seed=i + 1, **prm))
    return out


def _cases():
    cs = [Case(BASE)]
    cs += _sweeps(VALUES)
    cs += [Case(BASE, max_history=m, camera="subpixel", seed=3) for m in (1, 3)]
    cs += [Case(s, seed=1) for s in SHAPES]
    cs += [Case(s, "subpixel", seed=2, has_v=i % 2, batches=(2, 4, 9)[i % 3]) for i, s in enumerate(SHAPES)]
    cs += [Case(BASE, c) for c in CAMERAS + NOTHING]
    cs += [Case((5, 65), c, seed=4, specular_history=1) for c in CAMERAS + NOTHING]
    cs += [Case(s, "subpixel" if i % 2 else "pan", m, seed=5) for s in MASK_SHAPES for i, m in enumerate(MASK_PAIRS)]
    cs += [Case(BASE, c, exact=True, seed=6, normal_cos=1.0, plane_tolerance=0.0) for c in ("subpixel", "roll")]
    cs += [Case(BASE, "pan", poison=True, seed=7), Case((5, 65), "subpixel", poison=True, seed=8, specular_history=1)]
    cs += _random(20, 21)
    seen = {}
    for c in cs:
        seen.setdefault(c.id, c)
    return list(seen.values())


CASES = _cases()


def of_variant(variant):
    """the cases a variant runs: all of them.  (has_v and batches do not reach variant 0, whose cases they leave as they are.)"""
    assert variant in (0, 1, 2)
    return list(CASES)


def api_arguments(case, b, variant):
    """positional and keyword arguments of mygpuraytracer_amd.reproject_buffers for a built case `b`"""
    cur, prev = b["cur"], b["prev"]
    pg = prev["gbuf"]
    hist = dict(hit=pg["hit"], normal=pg["normal"], position=pg["position"], n=prev["n"], D=prev["D"],
                V=prev["V"] if case.params["has_v"] else None, ids=np.stack([pg["material"], pg["geom"]], -1))
    args = (b["rgb"], cur["albedo"], cur["normal"], cur["position"], np.stack([cur["material"], cur["geom"]], -1), cur["hit"], SPEC)
    kw = dict(hist=hist, hist_camera=b["hist_cam"], spp=case.params["spp"], variant=variant, **case.tparams)
    if variant == 2:
        kw.update(scatter=b["scatter"], batches=case.params["batches"])
    return args, kw


_REFERENCE = {}


def reference(case):
    """the built case with what the float64 restatements say of it, computed once and read-only: h, nh, mix, n, D, c32 (rgb / spp in
    float32), V1 (variant 1: NaN where the device leaves -1 to the spatial estimate), V2 (variant 2), q (the measured variance alone),
    near (the pixels to leave out of the comparison with float32), reasons (temporal_ref.reproject's)"""
    if case.id in _REFERENCE:
        return _REFERENCE[case.id]
    b = case.build()
    cur, prev, cam, spp = b["cur"], b["prev"], b["hist_cam"], case.params["spp"]
    h, w = case.shape
    hit = cur["hit"]
    clean = cur
    if b["poisoned"].any():                              # the poisoned pixels' expectation is stated below; the others do not read them
        clean = dict(cur, position=np.where(b["poisoned"][..., None], np.float32(0), cur["position"]),
                     normal=np.where(b["poisoned"][..., None], np.float32([0, 0, 1]), cur["normal"]))
    C = from_cov6(b["scatter"]) / (case.params["batches"] - 1.0)
    c32 = b["rgb"] / np.float32(spp)
    state_v = dict(prev) if case.params["has_v"] else {k: v for k, v in prev.items() if k != "V"}
    reasons = {}
    with np.errstate(invalid="ignore", over="ignore"):
        q = temporal_measured_variance(None, clean, None, SPEC, c32, spp, C, case.params["batches"], min_batches=2)
        if case.camera in ("none", "singular"):          # stated directly: nothing is inherited (the linear solve cannot take right = 0)
            hh, nh, near = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w), bool)
            V1, V2 = np.where(hit, np.nan, 0.0), q
        else:
            hh, nh, near = T.reproject(cam, clean, prev, SPEC, reasons=reasons, **case.tparams)
            if case.exact:                               # on the thresholds by construction, and exactly so in both precisions
                near = reasons["s"] | reasons["grid"]
            if case.params["has_v"]:
                V1 = temporal_variance(cam, clean, prev, SPEC, c32, spp, **case.tparams)
            else:
                V1 = np.where(hit, np.nan, 0.0)
            V2 = temporal_measured_variance(cam, clean, state_v, SPEC, c32, spp, C, case.params["batches"], min_batches=2, **case.tparams)
    if b["poisoned"].any():
        p = b["poisoned"]
        hh, nh, near = np.where(p[..., None], 0.0, hh), np.where(p, 0.0, nh), near & ~p
        V1, V2 = np.where(p, np.nan, V1), np.where(p, q, V2)
    m, n, _ = T.mix(b["rgb"], spp, hit, hh, nh)
    D = T.state(cur, m, n)["D"]
    out = dict(b, h=hh, nh=nh, mix=m, n=n, D=D, c32=c32, V1=V1, V2=V2, q=q, near=near, reasons=reasons)
    for v in list(out.values()) + list(cur.values()) + list(prev["gbuf"].values()) + [prev["D"], prev["n"], prev["V"]]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _REFERENCE[case.id] = out
    return out
