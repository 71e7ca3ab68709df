"""GPU: the network denoiser's convolution (k_nn_conv<NCO>, pack_weights; csrc/pt_nn.hip) over the channel space a weight blob may bring
-- "enc_conv0 takes 3, 6 or 9, dec_conv0 gives 3, none above 256" -- where tests/test_gpu_nn.py stays on OIDN 1.4's standard table, whose
widest layer is 112 channels: NCO = 8, two groups in the grid's z (Cout 129 .. 256) with a padded block that must not be stored, Cout
that is no multiple of 16 or of 4 in the fp16 and fp32 forms, Cin that is no multiple of 16 or 8, two sources inside one chunk and up
to 16 chunks, the pooled form for each.  Then the edges of fp16: subnormal operands and results, the rounding to infinity.  Then the
whole network on two channel tables off the standard one, and a blob of type h (fp16) against the same values stored as fp32.

A layer of Cout channels runs as `groups` launches in z of NCO blocks of 16 channels: blocks = ceil(Cout / 16), groups = ceil(blocks / 8),
NCO = ceil(blocks / groups) (split_cout); the input channels, each source padded to 16, go by in chunks of 32.

Every single-layer case runs at 38 x 22: the tile is 16 x 16, so both directions cross it and leave a remainder of 6."""
import numpy as np
import pytest

import unet_ref as U
from conftest import beq
from nncases import exact_case, random_case, scaled_case

pytestmark = pytest.mark.gpu

W, H = 38, 22
BOTH = (True, False)
ICS = (3, 6, 9)

_P = pytest.param
# (cin, cout, also at 1 x 1)
PLAIN = [
    _P(1, 1, True, id="1-1-the-smallest-of-everything"),
    _P(7, 5, False, id="7-5-ragged-both-sides-below-8"),
    _P(9, 15, False, id="9-15-ragged-both-sides-one-under-a-block"),
    _P(17, 17, False, id="17-17-one-channel-over-a-block"),
    _P(31, 33, False, id="31-33-one-under-a-chunk-one-over-two-blocks"),
    _P(33, 48, False, id="33-48-two-chunks-the-second-half-empty"),
    _P(48, 128, False, id="48-128-NCO-8-one-group"),
    _P(40, 129, False, id="40-129-two-groups-of-5-the-last-block-all-padding"),
    _P(64, 144, False, id="64-144-two-groups-of-5-a-full-ninth-block"),
    _P(24, 136, False, id="24-136-two-groups-of-5-half-a-ninth-block"),
    _P(16, 200, False, id="16-200-two-groups-of-7-the-last-block-all-padding"),
    _P(3, 256, False, id="3-256-two-groups-of-8-from-one-ragged-block"),
    _P(256, 3, False, id="256-3-8-chunks-into-the-fp32-form"),
    _P(256, 256, False, id="256-256-two-groups-of-8-8-chunks"),
]
F32 = [
    _P(8, 4, id="8-4-all-four-fp32-channels"),
    _P(17, 1, id="17-1-one-channel-three-padded"),
    _P(33, 2, id="33-2-two-channels-two-chunks"),
    _P(256, 3, id="256-3-8-chunks"),
]
# (cin0 upsampled, cin1 skip, cout, also at 2 x 2)
TWO = [
    _P(1, 1, 1, True, id="1-1-1-both-sources-in-one-chunk"),
    _P(16, 16, 16, False, id="16-16-16-both-sources-fill-one-chunk"),
    _P(17, 1, 7, False, id="17-1-7-ragged-first-source-over-a-block"),
    _P(48, 40, 24, False, id="48-40-24-a-chunk-straddles-the-sources-ragged-skip"),
    _P(80, 9, 20, False, id="80-9-20-odd-count-of-blocks-ragged-skip"),
    _P(200, 129, 144, False, id="200-129-144-both-ragged-above-128-two-groups"),
    _P(256, 256, 256, False, id="256-256-256-16-chunks-two-groups"),
]
# (cin, cout, also at 2 x 2)
POOLED = [
    _P(1, 1, True, id="1-1-the-smallest"),
    _P(9, 5, False, id="9-5-ragged-padded-pooled-block"),
    _P(20, 20, False, id="20-20-cout-a-multiple-of-4-not-16"),
    _P(17, 40, False, id="17-40-three-blocks-the-last-half"),
    _P(72, 129, False, id="72-129-two-groups-padded-block-in-the-second"),
    _P(128, 256, False, id="128-256-two-groups-of-8"),
]


@pytest.mark.parametrize("cin,cout,small", PLAIN)
def test_one_layer_exact_plain(gpu_product, cin, cout, small):
    for k, (w, h) in enumerate(((W, H), (1, 1)) if small else ((W, H),)):
        exact_case(gpu_product, w, h, cin, 0, cout, False, 11000 * cin + cout + k, relus=BOTH)


@pytest.mark.parametrize("cin,cout", F32)
def test_one_layer_exact_fp32_form(gpu_product, cin, cout):
    """exact_case holds the fp32 output's channels below cout to the integers and those from cout to 3 to exactly 0"""
    exact_case(gpu_product, W, H, cin, 0, cout, False, 13000 * cin + cout, relus=BOTH)


@pytest.mark.parametrize("cin0,cin1,cout,small", TWO)
def test_one_layer_exact_two_sources(gpu_product, cin0, cin1, cout, small):
    for k, (w, h) in enumerate(((W, H), (2, 2)) if small else ((W, H),)):
        exact_case(gpu_product, w, h, cin0, cin1, cout, False, 17000 * cin0 + 10 * cin1 + cout + k, relus=BOTH)


@pytest.mark.parametrize("cin,cout,small", POOLED)
def test_one_layer_exact_pooled(gpu_product, cin, cout, small):
    for k, (w, h) in enumerate(((W, H), (2, 2)) if small else ((W, H),)):
        exact_case(gpu_product, w, h, cin, 0, cout, True, 19000 * cin + cout + k, relus=BOTH)


@pytest.mark.parametrize("cin0,cin1,cout", [(48, 0, 128), (40, 0, 129), (256, 0, 256), (48, 40, 24), (256, 256, 256)])
def test_one_layer_random_within_the_summation_bound(gpu_product, cin0, cin1, cout):
    """test_gpu_nn.py's derivation (nncases.random_case) at NCO = 8, at two groups with a padded block, and at 8 and 16 chunks"""
    random_case(gpu_product, cin0, cin1, cout)


# ---- the edges of fp16 ---------------------------------------------------------------------------------------------------------------
def _magnitudes(rng, shape):
    """uniform over 0 .. 1023: times 2^-24, zero or an fp16 subnormal"""
    return rng.integers(0, 1024, shape).astype(np.int64)


def _sparse_signs(rng, shape, terms):
    """{-1, 0, 1}, nonzero with the probability that leaves `terms` nonzero taps per output channel on average (all of them when there
    are fewer): the sums then stay around 2^10 units however many input channels there are"""
    cin = shape[1]
    keep = min(1.0, terms / (9.0 * cin))
    return (rng.integers(0, 2, shape) * 2 - 1) * (rng.random(shape) < keep)


# (cin0, cin1, cout, pooled)
SUBNORMAL = [
    _P(1, 0, 1, False, id="1-1"),
    _P(9, 0, 16, False, id="9-16"),
    _P(48, 0, 128, False, id="48-128-NCO-8"),
    _P(17, 1, 7, False, id="17-1-7-two-sources"),
    _P(20, 0, 20, True, id="20-20-pooled"),
]


@pytest.mark.parametrize("mirror", [False, True], ids=["subnormal-inputs", "subnormal-weights"])
@pytest.mark.parametrize("cin0,cin1,cout,pooled", SUBNORMAL)
def test_subnormal_operands_and_results_are_kept(gpu_product, cin0, cin1, cout, pooled, mirror):
    """Inputs k 2^-24 with k in 0 .. 1023 -- every one zero or an fp16 subnormal -- against weights in {-1, 0, 1}; mirrored: weights
    +-k 2^-24 against inputs in {0, 1, 2}.  The bias is 0 or a multiple of 2^-24.  Every sum is n 2^-24 with |n| <= 9 Cin 2046 + 512
    < 2^24, exact in fp32 in any order, so the expected bits are the one correct rounding of n 2^-24 to fp16: a subnormal below
    n = 1024, where the conversion of the result is pinned too.  The weights are thinned so that the sums straddle 1024 at every Cin;
    at least a tenth of the expected outputs are nonzero subnormals and a tenth normal (asserted).  A matrix core that flushed
    subnormal operands would give zeros throughout, a flushed result zeros below 2^-14."""
    rng = np.random.default_rng(23000 * cin0 + 100 * cin1 + cout + (7 if mirror else 0))
    two = cin1 > 0
    s0 = (H // 2, W // 2, cin0) if two else (H, W, cin0)
    wshape = (cout, cin0 + cin1, 3, 3)
    if mirror:
        x0 = rng.integers(0, 3, s0).astype(np.int64)
        x1 = rng.integers(0, 3, (H, W, cin1)).astype(np.int64) if two else None
        wi = _magnitudes(rng, wshape) * _sparse_signs(rng, wshape, 5)
        xs, ws = 1.0, 2.0 ** -24
    else:
        x0 = _magnitudes(rng, s0)
        x1 = _magnitudes(rng, (H, W, cin1)) if two else None
        wi = _sparse_signs(rng, wshape, 9)
        xs, ws = 2.0 ** -24, 1.0
    bi = rng.integers(-512, 513, cout) * rng.integers(0, 2, cout)
    tiny = np.float64(np.finfo(np.float16).tiny)                      # 2^-14, the smallest normal
    for relu in BOTH:
        got, want = scaled_case(gpu_product, W, H, x0, x1, wi, bi, xs, ws, pooled, relu)
        a = np.abs(want.astype(np.float64))
        sub, normal = float(((a > 0) & (a < tiny)).mean()), float((a >= tiny).mean())
        bad = got.view(np.uint16) != want.view(np.uint16)
        print("cin %d+%d cout %d pooled %d relu %d %s: expected %.2f nonzero subnormal, %.2f normal; %d of %d differ, %d of them zeros on the device" % (
            cin0, cin1, cout, pooled, relu, "subnormal weights" if mirror else "subnormal inputs", sub, normal, int(bad.sum()), bad.size,
            int((got[bad] == 0).sum())))
        assert sub >= 0.1 and normal >= 0.1                           # the case itself
        assert beq(got, want)


def test_the_rounding_at_the_top_of_fp16(gpu_product):
    """No sum, only the one rounding: zero weights, the bias alone.  65520 = 65504 + half an ulp is the tie that nearest-even sends to
    2^16, which fp16 does not have: 65504 and the fp32 just below 65520 give 65504, +-65520 give +-inf."""
    rng = np.random.default_rng(29)
    x = rng.integers(0, 2, (H, W, 3)).astype(np.float16)
    below = np.nextafter(np.float32(65520), np.float32(0))
    bias = np.array([65504, below, 65520, -65520], np.float32)
    assert below < 65520 and float(below) > 65519.99
    got = gpu_product.kat_nn_conv(x, np.zeros((4, 3, 3, 3), np.float32), bias, relu=False)
    with np.errstate(over="ignore"):
        want = np.broadcast_to(bias.astype(np.float16), got.shape)
    assert beq(want[0, 0], np.array([65504, 65504, np.inf, -np.inf], np.float16))
    assert beq(got, want)


@pytest.mark.parametrize("cin,cout", [(48, 128), (256, 256)])
def test_sums_that_pass_the_top_of_fp16_round_to_infinity(gpu_product, cin, cout):
    """The exact scheme with weights in {-1, 0, 1} 2048 and biases k 2048: every sum is n 2048 with |n| <= 9 Cin + 8 < 2^13, exact in
    fp32; 63488 = 31 x 2048 is the largest that fp16 keeps and 32 x 2048 = 65536 >= 65520 rounds to infinity"""
    rng = np.random.default_rng(31000 * cin + cout)
    x = rng.integers(0, 2, (H, W, cin)).astype(np.int64)
    wi = rng.integers(-1, 2, (cout, cin, 3, 3)).astype(np.int64)
    bi = rng.integers(-8, 9, cout).astype(np.int64)
    for relu in BOTH:
        got, want = scaled_case(gpu_product, W, H, x, None, wi, bi, 1.0, 2048.0, False, relu)
        fin = np.isfinite(want)
        print("cin %d cout %d relu %d: %.3f of the expected outputs +inf, %.3f -inf, finite maximum %g" % (
            cin, cout, relu, float((want == np.inf).mean()), float((want == -np.inf).mean()), float(np.abs(want[fin]).max())))
        assert (want == np.inf).any() and fin.any() and np.abs(want[fin]).max() == 63488
        assert relu or (want == -np.inf).any()
        assert beq(got, want)


# ---- the whole network on other channel tables ---------------------------------------------------------------------------------------
TABLES = {"narrow": U.NARROW, "wide": U.WIDE}
_NET = {}


def _net_case(name, ic, w, h, seed):
    """one synthetic network on the named table and one frame, made once"""
    key = (name, ic, w, h, seed)
    if key not in _NET:
        rng = np.random.default_rng(seed)
        channels = U.standard_channels(ic) if name == "standard" else U.table(ic, *TABLES[name])
        weights = U.synthetic_weights(ic, seed, channels=channels)
        rgb = rng.random((h, w, 3), dtype=np.float32)
        alb = rng.random((h, w, 3), dtype=np.float32) if ic >= 6 else None
        nrm = (rng.random((h, w, 3), dtype=np.float32) * 2 - 1) if ic >= 9 else None
        _NET[key] = dict(channels=channels, weights=weights, rgb=rgb, alb=alb, nrm=nrm)
    return _NET[key]


# One seed per case, fixed from the two restatements alone: of the seeds 1, 2, 3 (the condition below holds on the CPU for all three, in
# every case) the one whose restatements differ most in the RMS.  A few thousand activations give few flipped roundings -- on the narrow
# table max|A - B| runs from 3e-5 (no fp16 rounding flipped at all, fp32 summation order alone) to 2.8e-3 over the seeds -- and a
# yardstick that has seen no flip does not measure one.
SEEDS = {("narrow", 3, 16): 2, ("narrow", 3, 33): 3, ("narrow", 6, 16): 3, ("narrow", 6, 33): 2, ("narrow", 9, 16): 1, ("narrow", 9, 33): 1,
         ("wide", 3, 16): 2, ("wide", 3, 33): 1, ("wide", 6, 16): 3, ("wide", 6, 33): 2, ("wide", 9, 16): 3, ("wide", 9, 33): 1}


@pytest.mark.parametrize("w,h", [(16, 16), (33, 17)])
@pytest.mark.parametrize("ic", ICS)
@pytest.mark.parametrize("name", sorted(TABLES))
def test_whole_network_on_other_tables_against_the_float64_restatement(gpu_product, name, ic, w, h):
    """test_gpu_nn.py's rule on tables off the standard one, linear mode: A = the float64 restatement, B = the float32 one,
    max|gpu - A| <= 4 max|A - B| and the same for the RMS; 4 max|A - B| <= rms(A) / 4 (asserted), so that the bound cannot hide a wiring
    error -- a group's weights or bias taken from the wrong place, a padded block stored over a neighbour, the channel map of a ragged
    source -- which costs O(rms(A)).  The handle reports the table, and its macs are the header's formula."""
    pt = gpu_product
    c = _net_case(name, ic, w, h, SEEDS[name, ic, w])
    A = U.denoise(c["rgb"], c["weights"], c["alb"], c["nrm"], srgb=1)
    B = U.denoise(c["rgb"], c["weights"], c["alb"], c["nrm"], srgb=1, dtype_name="float32")
    with pt.NN(w, h, U.weights_blob(c["weights"])) as nn:
        got = nn.host(c["rgb"], c["alb"], c["nrm"], srgb=1).astype(np.float64)
        info = nn.info()
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    print("%s ic %d %dx%d: max|A-B| %.3g rms|A-B| %.3g rms(A) %.3g; max|gpu-A| %.3g rms|gpu-A| %.3g" % (
        name, ic, w, h, np.abs(A - B).max(), rms(A - B), rms(A), np.abs(got - A).max(), rms(got - A)))
    assert 4 * np.abs(A - B).max() <= rms(A) / 4
    assert np.abs(got - A).max() <= 4 * np.abs(A - B).max()
    assert rms(got - A) <= 4 * rms(A - B)
    flat = [(n, sum(ci) if isinstance(ci, tuple) else ci, co) for n, ci, co in c["channels"]]
    assert info["input_channels"] == ic and info["layers"] == flat
    wp, hp = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    assert (info["padded_width"], info["padded_height"]) == (wp, hp)
    assert info["macs"] == sum(9 * ci * co * (wp >> lv) * (hp >> lv) for (_, ci, co), lv in zip(flat, U.LEVELS))


@pytest.mark.parametrize("name", ["standard", "wide"])
def test_a_blob_of_fp16_tensors_runs_as_the_same_values_in_fp32(gpu_product, name):
    """type h (OIDN 2 ships such files): weights and biases rounded to fp16, stored once as float16 and once, the same values, as
    float32.  The reader converts h exactly, so the two results are the same bits: no tolerance."""
    pt = gpu_product
    ic, w, h = 6, 33, 17
    c = _net_case(name, ic, w, h, 2)
    half = {k: v.astype(np.float16) for k, v in c["weights"].items()}
    blob_h = U.weights_blob(half)
    blob_f = U.weights_blob({k: v.astype(np.float32) for k, v in half.items()})
    assert {t[3] for t in pt.debug_tza_list(blob_h)} == {"h"} and {t[3] for t in pt.debug_tza_list(blob_f)} == {"f"}
    assert any((v != c["weights"][k]).any() for k, v in half.items())               # the rounding changed something: h is not f renamed
    got_h = pt.nn_denoise_buffers(blob_h, c["rgb"], c["alb"], None, srgb=1)
    got_f = pt.nn_denoise_buffers(blob_f, c["rgb"], c["alb"], None, srgb=1)
    assert beq(got_h, got_f) and got_h.any() and np.isfinite(got_h).all()
    # and it is the network of those values: the restatement on them, by the rule above
    wf = {k: v.astype(np.float32) for k, v in half.items()}
    A = U.denoise(c["rgb"], wf, c["alb"], None, srgb=1)
    B = U.denoise(c["rgb"], wf, c["alb"], None, srgb=1, dtype_name="float32")
    assert 4 * np.abs(A - B).max() <= np.sqrt(np.mean(np.square(A))) / 4
    assert np.abs(got_h - A).max() <= 4 * np.abs(A - B).max()
