"""One convolution layer of the network denoiser (ptx_kat_nn_conv, which runs the production k_nn_conv) against plain integer and
float64 arithmetic: the cases tests/test_gpu_nn.py runs over the standard channel table and tests/test_gpu_nn_channels.py over the rest
of the accepted channel space (every count in 1 .. 256, two sources, the pooled form) and at the edges of fp16.

Three schemes, each with the device's expected bits or bound derived from the data alone:
  * exact_case: inputs in {0, 1}, weights in {-1, 0, 1} / 16, biases k / 16 -- integer arithmetic, bit for bit;
  * scaled_case: integer inputs, weights and biases times powers of two chosen so that every sum is an integer multiple of one power
    of two below 2^24 of it: exact in fp32 in any order, so the expected bits are ONE correct rounding of the float64 value to fp16.
    With 2^-24 on the inputs or the weights every operand is an fp16 subnormal; with 2048 on the weights the sums pass 65520 and the
    rounding gives infinities;
  * random_case: random fp16 data against the standard summation bound.
The frame is W x H of the convolution's output before the pool; the kernel's tile is 16 x 16."""
import numpy as np

from conftest import beq


def int_conv(x, w):
    """(H, W, Cout) in w's dtype: the 3 x 3 cross-correlation with zero padding of x (H, W, Cin) and w (Cout, Cin, 3, 3).  Integer
    arrays go through float64 matrix products, which are exact while sum |x| |w| < 2^53 (asserted): numpy multiplies integer matrices
    without BLAS, seconds at 512 channels."""
    if np.issubdtype(w.dtype, np.integer):
        assert float(np.abs(x).max()) * float(np.abs(w).max()) * 9 * x.shape[2] < 2.0 ** 53
        return np.rint(int_conv(x.astype(np.float64), w.astype(np.float64))).astype(w.dtype)
    h, wd, cin = x.shape
    xp = np.zeros((h + 2, wd + 2, cin), w.dtype)
    xp[1:-1, 1:-1] = x
    out = np.zeros((h * wd, w.shape[0]), w.dtype)
    for ky in range(3):
        for kx in range(3):
            out += np.ascontiguousarray(xp[ky:ky + h, kx:kx + wd]).reshape(h * wd, cin) @ np.ascontiguousarray(w[:, :, ky, kx].T)
    return out.reshape(h, wd, w.shape[0])


def up(x):
    return x.repeat(2, axis=0).repeat(2, axis=1)


def pool(x):
    h, w, c = x.shape
    return x.reshape(h // 2, 2, w // 2, 2, c).max(axis=(1, 3))


def default_relus(pooled, two):
    return (True, False) if not pooled and not two else (True,)


def exact_case(pt, w, h, cin0, cin1, cout, pooled, seed, relus=None):
    """inputs in {0, 1}, weights in {-1, 0, 1} / 16, biases multiples of 1 / 16: every sum is an integer multiple of 2^-4 below
    128 = 2048 * 2^-4 (asserted), exact in fp32 and in fp16; the device's bits are those of integer arithmetic.  relus: the ReLU
    settings to run; by default both in the plain form and ReLU alone in the pooled and two-source forms.  With cout <= 4 the unpooled
    form's fp32 output is held to the same integers, and its channels from cout to 3 (zero weights, zero bias) to 0."""
    rng = np.random.default_rng(seed)
    two = cin1 > 0
    x0 = rng.integers(0, 2, ((h // 2, w // 2, cin0) if two else (h, w, cin0))).astype(np.int64)
    x1 = rng.integers(0, 2, (h, w, cin1)).astype(np.int64) if two else None
    wi = rng.integers(-1, 2, (cout, cin0 + cin1, 3, 3)).astype(np.int64)      # no symmetry among taps, channels or outputs
    bi = rng.integers(-8, 9, cout).astype(np.int64)
    x = np.concatenate([up(x0), x1], axis=2) if two else x0
    for relu in (default_relus(pooled, two) if relus is None else relus):
        want = int_conv(x, wi) + bi
        if relu:
            want = np.maximum(want, 0)
        if pooled:
            want = pool(want)
        assert np.abs(want).max() < 2048
        src1 = None if x1 is None else x1.astype(np.float16)
        got = pt.kat_nn_conv(x0.astype(np.float16), wi.astype(np.float32) / 16, bi.astype(np.float32) / 16, src1=src1, upsample=two, relu=relu, pool=pooled)
        assert beq(got, (want / 16.0).astype(np.float16)), (w, h, cin0, cin1, cout, pooled, relu, int((got != (want / 16.0).astype(np.float16)).sum()))
        if cout <= 4 and not pooled:
            got32 = pt.kat_nn_conv(x0.astype(np.float16), wi.astype(np.float32) / 16, bi.astype(np.float32) / 16, src1=src1, upsample=two, relu=relu, f32=True)
            assert beq(got32[..., :cout], (want / 16.0).astype(np.float32)), (w, h, cin0, cin1, cout, relu)
            assert not got32[..., cout:].any() and not np.signbit(got32[..., cout:]).any(), (w, h, cin0, cin1, cout, relu)


def scaled_case(pt, w, h, x0i, x1i, wi, bi, xs, ws, pooled, relu):
    """The layer on x = xi * xs, weights wi * ws, bias bi * xs * ws, all integer arrays times powers of two (xs, ws) under which every
    operand is an fp16 value.  Every sum is an integer n times xs * ws with |n| < 2^24 (asserted): exact in fp32 whatever the order.
    Returns (got, want): the device's fp16 output and the one correct rounding of n * xs * ws from float64 to fp16 (overflow -> inf)."""
    two = x1i is not None
    unit = xs * ws
    x = np.concatenate([up(x0i), x1i], axis=2) if two else x0i
    n = int_conv(x.astype(np.int64), wi.astype(np.int64)) + bi.astype(np.int64)
    assert np.abs(n).max() < 2 ** 24
    if relu:
        n = np.maximum(n, 0)
    if pooled:
        n = pool(n)
    half = lambda a, s: (a.astype(np.float64) * s).astype(np.float16)
    for a, s in ((x0i, xs), (wi, ws)) + (((x1i, xs),) if two else ()):
        assert np.array_equal(half(a, s).astype(np.float64), a.astype(np.float64) * s)      # the operands are fp16 values as they stand
    bias = (bi.astype(np.float64) * unit).astype(np.float32)
    assert np.array_equal(bias.astype(np.float64), bi.astype(np.float64) * unit)
    got = pt.kat_nn_conv(half(x0i, xs), (wi.astype(np.float64) * ws).astype(np.float32), bias, src1=half(x1i, xs) if two else None,
                         upsample=two, relu=relu, pool=pooled)
    with np.errstate(over="ignore"):
        want = (n.astype(np.float64) * unit).astype(np.float16)
    return got, want


def random_case(pt, cin0, cin1, cout, w=38, h=22):
    """Inputs from {0} and [2^-10, 2) (no fp16 subnormals), He-scaled weights, both fp16 values.  s = the float64 result on them;
    E = 2 K 2^-24 (|b| + sum |w| |x|), K = 9 Cin: twice the standard summation bound, the matrix core's order and rounding being its own;
    every output is within E + 2^-11 (|relu(s)| + E) + 2^-25 of relu(s): the sum's error, then one rounding to fp16."""
    rng = np.random.default_rng(50000 + 300 * cin0 + 7 * cin1 + cout)
    two = cin1 > 0
    draw = lambda shape: np.where(rng.random(shape) < 0.2, 0.0, 2.0 ** rng.uniform(-10, 0.999, shape)).astype(np.float16)
    x0 = draw((h // 2, w // 2, cin0) if two else (h, w, cin0))
    x1 = draw((h, w, cin1)) if two else None
    cin = cin0 + cin1
    wt = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float16)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    assert x0.max() < 2 and (x0[x0 > 0].min() >= 2.0 ** -10)
    x = np.concatenate([up(x0), x1], axis=2) if two else x0
    s = int_conv(x.astype(np.float64), wt.astype(np.float64)) + b.astype(np.float64)
    mag = int_conv(np.abs(x).astype(np.float64), np.abs(wt).astype(np.float64)) + np.abs(b).astype(np.float64)
    E = 2 * 9 * cin * 2.0 ** -24 * mag
    want = np.maximum(s, 0.0)
    got = pt.kat_nn_conv(x0, wt.astype(np.float32), b, src1=x1, upsample=two).astype(np.float64)
    excess = np.abs(got - want) - (E + 2.0 ** -11 * (want + E) + 2.0 ** -25)
    print("cin %d+%d cout %d: max |gpu - relu(s)| %.3g, largest excess over the bound %.3g" % (cin0, cin1, cout, np.abs(got - want).max(), excess.max()))
    assert (excess <= 0).all()
