"""CPU: the moments grid (tests/momentscases.py) before it goes to the device (tests/test_gpu_moments_grid.py).

Conditioning: on every case and at every checkpoint the float32 probe of k_moments_add (tests/moments_f32.py) stays within HALF of the
bounds of tests/momentscases.py against the float64 restatement -- covariance (B + 8) 2^-23 sqrt(C_ii C_jj), mean (B + 2) 2^-23 |mean|,
exact zeros where the restatement has them -- so float32 arithmetic alone leaves a twofold margin and a failure on the device points at
the kernel or at its build flags (the error-free D needs -ffp-contract=off: a contracted acc * wo - p2 is no longer the residual of a
rounded product).  The probe in the naive form, d = fl(fl(acc - snap) / k - mean), D = d k W, breaks the covariance bound on every
case with sigma <= 1e-4, the single pixels included, so the measure bites.

Worst share of its bound the probe reached, covariance / mean, over the four sigma, the dyadic case (0 / 0 everywhere) and both frame
sizes, per sequence of k -- and what the naive probe made of the covariance bound at 65 x 5 (at 1 x 1 in brackets), sigma = 0.5, 1e-2,
1e-4, 1e-6:

    1000, 1, 3, 12, 1, 3     0.178 / 0.283     naive 69     1.8e3  3.9e4  3.9e4   (0.95  3.6   701    4.6e3)
    8 x 64                   0.111 / 0.165     naive 4.1    21     3.0e3  3.4e5   (0.31  3.1   645    7.7e4)
    100000, 8 x 32           0.127 / 0.348     naive 35     7.6e4  2.6e5  3.5e5   (1.9   21    569    470)
    2^20, 64 x 16            0.140 / 0.399     naive 5.3    192    307    307     (0.56  39    307    307)
    16 x 1024 (65 x 5 only)  0.114 / 0.154     naive 1.5    104    4.2e3  4.4e5
    2^24 - 40, 8 x 5         0.139 / 0.232     naive 4.1    4.1    4.1    4.1     (0.83  4.0   4.0    3.9)
    tiled, 24 adds           0.158 / 0.358     (257 x 3 and 65 x 5, every tile its own sigma and k)

The 1e4 pixel's D D / den stayed finite in every case.  The cancelling frames (eval_frames): the median g^T C g over the sum of its terms' sizes is 1,
4e-4 and 5e-6 at eta = 1, 1e-2 and 1e-3, and the threshold of pixels_over stands in a gap of 3e-3 .. 7e-3 in rel beside per-pixel
bounds below 1e-6.
"""
import numpy as np
import pytest

import momentscases as MC
import moments_f32 as probe
from adaptive_ref import TiledMoments, tile_of
from moments_ref import to_cov6

F = np.float32


def _run(c, naive=False):
    """{checkpoint: (cov ratio, mean ratio, wrong zeros)} of the probe on a case, and the probe"""
    p, out, ref = probe.Probe(*c.shape, naive=naive), {}, MC.reference(c)
    last = 0
    for b, (acc, n) in enumerate(MC.case_frames(c), 1):
        p.add(acc, n - last, n)
        last = n
        if b in ref:
            rc, zc = MC.cov_ratio(p.cov6(), ref[b]["cov6"], b)
            rm, zm = MC.mean_ratio(p.mean, ref[b]["mean"], b)
            out[b] = (rc, rm, zc + zm)
    return out, p


@pytest.mark.parametrize("seq", list(MC.SEQUENCES))
def test_the_probe_stays_within_half_of_each_bound(seq):
    for c in MC.of_sequence(seq):
        res, p = _run(c)
        assert sorted(res) == MC.checkpoints(len(c.ks))
        wc, wm = max(v[0] for v in res.values()), max(v[1] for v in res.values())
        print("%-28s probe: cov %.3f of its bound, mean %.3f" % (c.id, wc, wm))
        assert wc <= 0.5 and wm <= 0.5 and not any(v[2] for v in res.values()), (c.id, res)
        assert p.term_finite, c.id                       # the 1e4 pixel's D D / den too
        assert (p.B == len(c.ks)).all() and (p.W == sum(c.ks)).all()
        sp = MC.special_pixels(*c.shape)
        if sp:
            assert np.isfinite(p.M[sp["firefly"]]).all() and (c.sigma != 0.5 or p.M[sp["firefly"]][:3].all())
            assert not p.M[sp["black"]].any() and not p.mean[sp["black"]].any()
            assert not p.M[sp["green0"]][[1, 3, 5]].any() and (c.sigma != 0.5 or p.M[sp["green0"]][0] > 0)


@pytest.mark.parametrize("seq", list(MC.SEQUENCES))
def test_the_dyadic_case_is_exact(seq):
    """every sum and product exact: no scatter at all, and the mean is the colour bit for bit, after every add"""
    cases = [c for c in MC.of_sequence(seq) if c.sigma is None]
    assert bool(cases) == (sum(MC.SEQUENCES[seq]) <= MC.DYADIC_MAX_TOTAL)
    for c in cases:
        colour = MC.colours(c.shape[0], c.shape[1], np.random.default_rng(c.seed), dyadic=True)
        assert (colour * 64 == np.round(colour * 64)).all()
        p, last = probe.Probe(*c.shape), 0
        for acc, n in MC.case_frames(c):
            assert (acc.astype(np.float64) == n * colour.astype(np.float64)).all()
            p.add(acc, n - last, n)
            last = n
            assert not p.cov6().any() and not p.M.any() and np.array_equal(p.mean.view(np.uint32), colour.view(np.uint32)), (c.id, n)


@pytest.mark.parametrize("seq", list(MC.SEQUENCES))
def test_the_naive_form_breaks_the_covariance_bound(seq):
    for c in MC.of_sequence(seq):
        if c.sigma is None:
            continue
        res, _ = _run(c, naive=True)
        wc = max(v[0] for v in res.values())
        print("%-28s naive form: cov %.3g of its bound" % (c.id, wc))
        if c.sigma <= 1e-4:
            assert wc > 1.0, (c.id, wc)


@pytest.mark.parametrize("shape", MC.TILED_SHAPES)
def test_the_probe_on_the_tiled_cases(product, shape):
    """every tile its own sigma and its own k per add: the same bounds per pixel with the pixel's own B"""
    h, w = shape
    tp = product.tile_pixels()
    tile = tile_of(h, w, tp)
    for rep in range(MC.TILED_REPS):
        rows, sig, frames = MC.tiled_case(h, w, tp, rep)
        assert set(np.unique(rows)) == set(MC.TILED_KS)
        p, ref, last = probe.Probe(h, w), TiledMoments(h, w, tp), np.zeros(len(sig), np.int64)
        worst = [0.0, 0.0]
        for b, (acc, n) in enumerate(frames, 1):
            p.add(acc, (n - last)[tile], n[tile])
            ref.add(acc, n)
            last = n
            if b in MC.checkpoints(len(frames)):
                B = ref.B_pixels()
                rc, zc = MC.cov_ratio(p.cov6(), to_cov6(ref.cov()), B)
                rm, zm = MC.mean_ratio(p.mean, ref.mean, B)
                worst = [max(worst[0], rc), max(worst[1], rm)]
                assert rc <= 0.5 and rm <= 0.5 and not zc and not zm, (shape, rep, b, rc, rm)
                assert (p.B == B).all() and (p.W == ref.W_pixels()).all()
        print("%dx%d sigma per tile %s: cov %.3f of its bound, mean %.3f" % (w, h, sig, worst[0], worst[1]))
        assert p.term_finite and ref.B.max() >= 12


@pytest.mark.parametrize("what", list(MC.EVAL_SHAPES))
def test_the_threshold_gap_of_the_cancelling_cases(what):
    """the anti-correlated frames: g^T C g with g = Rec. 709 is a small share of its terms where eta is small, and the threshold of
    pixels_over stands in a gap of more than twice the per-pixel bound on rel -- or the case is built wrongly"""
    h, w = MC.EVAL_SHAPES[what]
    frames, eta = MC.eval_frames(h, w, seed=h * w)
    p, last = probe.Probe(h, w), 0
    for acc, n in frames:
        p.add(acc, n - last, n)
        last = n
    for floor in (0.05, 0.4):
        q, b = MC.quad_bound(p.cov6(), MC.LUM)
        rel2, b2 = MC.rel2_bound(p.mean, p.cov6(), last, floor)
        share = q / (b / (10 * MC.EPS))
        for e in MC.ETAS:                                # the cancellation is there: q / S is a few eta^2 (1 at eta = 1)
            print("%s eta %g: median q / S %.3g" % (what, e, np.median(share[eta == e])))
            assert np.median(share[eta == e]) <= min(10 * e * e, 1.0)
        rel, rb = np.sqrt(rel2), MC.rel_bound(rel2, b2)
        thr, gap, bnd = MC.threshold_in_the_widest_gap(rel, rb)
        print("%s floor %g: threshold %.6g, gap %.3g, per-pixel bound %.3g" % (what, floor, thr, gap, bnd))
        assert gap > 2 * bnd and (np.abs(rel - thr) > rb).all()
        assert 0 < (rel > thr).sum() < rel.size
    # the probe's own quad_form stays within the bound of the float64 one of its state
    got = np.maximum(probe.quad_form(MC.LUM, p.M, p.B), F(0))
    assert (np.abs(got - q) <= 0.5 * b).all()
