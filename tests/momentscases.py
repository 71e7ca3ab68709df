"""The cases of the moments grid (tests/test_moments_grid_cpu.py, tests/test_gpu_moments_grid.py): accumulation buffers of frames that are
converging, where a batch mean lies close to the running mean and the scatter term D = W acc - W' snap of k_moments_add
(pt_moments.hip) is a difference of two large, nearly equal numbers -- and the measures that hold a state to the float64 restatement
(tests/moments_ref.py) there, scaled by the state's own size and without a floor.

Buffers (frames): tests/test_gpu_moments.py's _frames with the relative noise sigma as a parameter.  Per pixel a colour in [0.05, 1]^3,
per add an increment fl32(k c max(1 + z / sqrt(k), 0)) with z = sigma (n + 0.4 n_k), n common to the channels and n_k each channel's own
(sigma = 0.5 is _frames' noise), summed in fp32; an add's batch is synthesised as one increment, the first of 2^24 - 40 samples too.
sigma = None is the dyadic case: colours that are multiples of 2^-6, no noise, totals <= 2^17, so every sum and every product is exact,
D is exactly 0 and the mean is the colour bit for bit.  With eta, the noise is anti-correlated between the channels (eval_frames).

Three special pixels are planted in every frame of at least four pixels (special_pixels): a black one, whose buffer is always 0; one whose
green is 0; one of colour 1e4 in every channel, the scale of a firefly (2^13 in the dyadic case, which needs exact products).  At
W = 2^24, k = 8 and sigma = 0.5 its D is about sqrt(k) W c sigma = 2.4e11 and D D = 6e22, den = k W W' = 2e15: all finite in fp32
(tests/test_moments_grid_cpu.py asserts it on the probe).

Measures, B = the adds so far (per pixel after a tiled add):
    covariance  |C_ij - C_ij^ref| <= (B + 8) 2^-23 sqrt(C_ii^ref C_jj^ref); where a diagonal entry of the reference is exactly 0 the
                entries of its row and column must be exactly 0.  D is right to about 1.5 ulp, each term D_i D_j / den adds three
                roundings, B accumulations follow and the read's / (B - 1): about B + 6 half-ulps, doubled.
    mean        |mean - mean^ref| <= (B + 2) 2^-23 |mean^ref| per channel, exactly 0 where the reference is 0.
    quad form   |max(q, 0) - max(q^ref, 0)| <= 10 2^-23 S, S = sum_ij |g_i g_j C_ij|: six triple products, five adds, a division and
                the rounding of the read cov6, about 10 half-ulps, doubled.  q^ref is float64 from the state the device reads back.
The bounds are derived, not tuned."""
import collections
import functools

import numpy as np

from moments_ref import LUM, PAIRS, Moments, from_cov6, quad

F = np.float32
EPS = 2.0 ** -23

SIGMAS = (0.5, 1e-2, 1e-4, 1e-6)
SEQUENCES = collections.OrderedDict([
    ("mixed", [1000, 1, 3, 12, 1, 3]),                   # tests/test_gpu_moments.py's last sequence
    ("k8x64", [8] * 64),
    ("1e5_then_8x32", [100000] + [8] * 32),
    ("2p20_then_64x16", [2 ** 20] + [64] * 16),
    ("k16x1024", [16] * 1024),
    ("to_2p24", [2 ** 24 - 40] + [8] * 5),               # ends exactly at 2^24, the largest total an add accepts
])
SHAPES = ((5, 65), (1, 1))                               # one pixel over a 4 x 64 workgroup both ways, odd width; one pixel
LONG = "k16x1024"                                        # at 5 x 65 only
DYADIC_MAX_TOTAL = 1 << 17
TILED_SHAPES = ((3, 257), (5, 65))                       # pairs straddle tiles of 256 pixels
TILED_KS = (0, 1, 3, 12, 100)
TILED_ADDS = 24

Case = collections.namedtuple("Case", "id seq ks sigma shape seed")


def _cases():
    out = []
    for si, (name, ks) in enumerate(SEQUENCES.items()):
        for shape in SHAPES:
            if name == LONG and shape != SHAPES[0]:
                continue
            sig = SIGMAS + ((None,) if sum(ks) <= DYADIC_MAX_TOTAL else ())
            for gi, sigma in enumerate(sig):
                sid = "dyadic" if sigma is None else "%g" % sigma
                out.append(Case("%s-%s-%dx%d" % (name, sid, shape[1], shape[0]), name, tuple(ks), sigma, shape,
                                7919 * si + 101 * gi + shape[0] * shape[1]))
    return out


CASES = _cases()


def of_sequence(name):
    return [c for c in CASES if c.seq == name]


def checkpoints(nadds):
    """the adds after which a state is compared: 1, 2, 4, 8, ... and the last"""
    return sorted({1 << i for i in range(nadds.bit_length()) if (1 << i) <= nadds} | {nadds})


def special_pixels(h, w):
    """name -> (y, x); none in a frame of fewer than four pixels.  The black pixel is the odd half of the first pair, the one with a
    channel of 0 the last pixel of a middle row (alone in its pair when the width is odd)."""
    if h * w < 4:
        return {}
    return dict(black=(0, 1), green0=(h // 2, w - 1), firefly=(h - 1, (w // 2) | 1 if w > 2 else 0))


def colours(h, w, rng, dyadic=False):
    if dyadic:
        c = rng.integers(4, 65, (h, w, 3)).astype(np.float64) / 64.0
    else:
        c = 0.05 + 0.95 * rng.random((h, w, 3))
    c = c.astype(F)
    sp = special_pixels(h, w)
    if sp:
        c[sp["black"]] = 0
        c[sp["green0"]][1] = 0
        c[sp["firefly"]] = 8192.0 if dyadic else 1e4
    return c


def frames(h, w, ks, sigma, seed):
    """[(buffer (H, W, 3) float32, read-only, samples_total)]; sigma None = the dyadic case"""
    rng = np.random.default_rng(seed)
    c = colours(h, w, rng, dyadic=sigma is None).astype(np.float64)
    s = 0.0 if sigma is None else float(sigma)
    acc, n, out = np.zeros((h, w, 3), F), 0, []
    for k in ks:
        z = s * (rng.standard_normal((h, w, 1)) + 0.4 * rng.standard_normal((h, w, 3)))
        acc = (acc + (k * c * np.maximum(1 + z / np.sqrt(k), 0)).astype(F)).astype(F)
        n += k
        acc.setflags(write=False)
        out.append((acc, n))
    return out


@functools.lru_cache(maxsize=None)
def case_frames(c):
    return frames(c.shape[0], c.shape[1], c.ks, c.sigma, c.seed)


@functools.lru_cache(maxsize=None)
def reference(c):
    """{adds so far: dict(mean (H, W, 3), cov6 (H, W, 6), W)} at the checkpoints, float64, computed once and read-only"""
    ref, out, cps = Moments(*c.shape), {}, set(checkpoints(len(c.ks)))
    for b, (acc, n) in enumerate(case_frames(c), 1):
        ref.add(acc, n)
        if b in cps:
            out[b] = dict(mean=ref.mean.copy(), cov6=ref.cov6(), W=ref.W)
            for v in (out[b]["mean"], out[b]["cov6"]):
                v.setflags(write=False)
    return out


# ---- the measures ------------------------------------------------------------------------------------------------------------------------

def cov_ratio(cov, ref6, B):
    """(the largest |C_ij - C_ij^ref| over its bound, the entries that had to be exactly 0 and are not); B an int or (H, W)"""
    ref6 = np.asarray(ref6, np.float64)
    got = np.asarray(cov, np.float64)
    B = np.asarray(B, np.float64)[..., None]
    scale = np.sqrt(np.stack([ref6[..., i] * ref6[..., j] for i, j in PAIRS], -1))
    bound = (B + 8) * EPS * scale
    zero = scale == 0
    wrong = int((got[zero] != 0).sum())
    r = np.abs(got - ref6)[~zero] / bound[~zero]
    return (float(r.max()) if r.size else 0.0), wrong


def mean_ratio(mean, ref, B):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(mean, np.float64)
    bound = (np.asarray(B, np.float64)[..., None] + 2) * EPS * np.abs(ref)
    zero = ref == 0
    wrong = int((got[zero] != 0).sum())
    r = np.abs(got - ref)[~zero] / np.broadcast_to(bound, ref.shape)[~zero]
    return (float(r.max()) if r.size else 0.0), wrong


def quad_bound(cov6, g):
    """(max(q^ref, 0), 10 2^-23 S) per pixel in float64 from a read-back cov6; g: (3,) or (H, W, 3)"""
    C = from_cov6(cov6)
    g = np.broadcast_to(np.asarray(g, np.float64), C.shape[:-1])
    S = np.einsum("...i,...ij,...j->...", np.abs(g), np.abs(C), np.abs(g))
    return np.maximum(quad(C, g), 0.0), 10 * EPS * S


def rel2_bound(mean, cov6, W, floor):
    """(rel^2 of the restatement, its bound) per pixel: rel^2 = max(q, 0) / (W max(l(mean), floor)^2), bound = the quad form's over the
    same denominator.  W: an int or (H, W)."""
    q, b = quad_bound(cov6, LUM)
    den = np.maximum(np.asarray(W, np.float64), 1.0) * np.maximum(np.asarray(mean, np.float64) @ LUM, floor) ** 2
    return q / den, b / den


def threshold_in_the_widest_gap(rel, bound):
    """a threshold that every pixel's rel is further from than its own bound allows it to move: the middle of the gap between
    neighbouring sorted rel that is widest after both bounds are taken off.  Returns (threshold as a float32 value, gap, the larger
    of the two neighbours' bounds)."""
    o = np.argsort(rel.ravel())
    r, b = rel.ravel()[o], bound.ravel()[o]
    room = (r[1:] - b[1:]) - (r[:-1] + b[:-1])
    i = int(np.argmax(room))
    thr = float(F((r[i] + b[i] + r[i + 1] - b[i + 1]) / 2))
    return thr, float(r[i + 1] - r[i]), float(max(b[i], b[i + 1]))


def rel_bound(rel2, b2):
    """|sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b))"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.minimum(np.sqrt(b2), np.where(rel2 > 0, b2 / np.sqrt(rel2), np.inf))


# ---- anti-correlated colour noise: the evaluators of quad_form under cancellation -------------------------------------------------------

ETAS = (1.0, 1e-2, 1e-3)
EVAL_KS = (12, 3, 100, 12, 1, 16, 16, 16)
EVAL_SIGMA = 0.2
EVAL_SHAPES = dict(prep=(16, 16), summary=(5, 65), select=(3, 257))


def eval_frames(h, w, seed, ks=EVAL_KS, sigma=EVAL_SIGMA):
    """frames whose channel noise nearly cancels in the luminance: per pixel an eta from ETAS and a direction v with
    sum_k l_k c_k v_k = 0 (a fixed vector less its component along l c, largest entry 1); the noise of channel k is
    sigma (n v_k + eta n'), so the luminance's is eta times a channel's and g^T C g with g = Rec. 709 is eta^2 of its terms.
    Returns ([(buffer, samples_total)], eta (H, W))."""
    rng = np.random.default_rng(seed)
    c = (0.05 + 0.95 * rng.random((h, w, 3))).astype(F).astype(np.float64)
    eta = np.asarray(ETAS)[rng.integers(0, len(ETAS), (h, w))]
    wv = LUM * c
    u = np.array([1.0, -1.0, 0.5])
    v = u - (wv @ u / (wv * wv).sum(-1))[..., None] * wv
    v = v / np.abs(v).max(-1, keepdims=True)
    assert (np.abs((wv * v).sum(-1)) < 1e-15).all()
    acc, n, out = np.zeros((h, w, 3), F), 0, []
    for k in ks:
        z = sigma * (rng.standard_normal((h, w, 1)) * v + eta[..., None] * rng.standard_normal((h, w, 1)))
        acc = (acc + (k * c * np.maximum(1 + z / np.sqrt(k), 0)).astype(F)).astype(F)
        n += k
        acc.setflags(write=False)
        out.append((acc, n))
    return out, eta


# ---- the tiled add: every tile its own sigma and, per add, its own k ---------------------------------------------------------------------

TILED_REPS = len(SIGMAS)                                 # tile t takes SIGMAS[(t + rep) % 4]: every tile meets every sigma


def tiled_case(h, w, tile_px, rep):
    """(rows (adds, tiles) of k from TILED_KS, sigma per tile, [(buffer, samples per tile)]) through tests/test_gpu_adaptive.py's
    tiled_frames, whose `scale` multiplies its noise of 0.5"""
    from adaptive_ref import num_tiles
    from test_gpu_adaptive import schedule, tiled_frames
    sig = np.array([SIGMAS[(t + rep) % len(SIGMAS)] for t in range(num_tiles(h, w, tile_px))])
    seed = 100000 * h + 100 * w + rep
    rows = schedule(h, w, tile_px, TILED_ADDS, seed)
    return rows, sig, tiled_frames(h, w, tile_px, rows, seed, scale=sig / 0.5)
