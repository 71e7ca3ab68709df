"""GPU: the image metrics (ptx_metrics_*, csrc/pt_metrics.hip) against their restatements (tests/metrics_ref.py: A float64, B float32; the
cases and d of tests/metricscases.py, held to the reference's ssim.py by tests/test_metrics_cpu.py).

Bounds.
  SSIM family (ssim, msssim, per channel, mcs, the map pixel by pixel): |gpu - A| <= 4 d, d the largest |A - B| over the whole case list
  -- the factor the network tests use for the same A / B scheme.
  Pointwise sums against A.  Inputs are in [0, 1] and every transform maps [0, 1] into [0, 1], so with u = 2^-24 a transformed value is off by
  e = K u: NONE K = 0 (nothing is rounded: the divisor is 1); SNORM K = 2 (a product, a sum); SRGB K = 8 (powf to 2 ulp, a product, a sum,
  and the branch's other arm one product); HDR K = 300: the curve is about 20 roundings of values below 1.4 over a divisor of 0.867, and
  the sRGB curve that follows has slope 12.92 at 0, which multiplies them: 12.92 * 20 + 8 < 300.  Then, per term and so for the means:
    l1    : | |d'| - |d| | <= 2 e + u |d|                               -> 2 e + 2 u l1
    mse   : |d'^2 - d^2| <= 2 e (2 |d| + 2 e) + 3 u d^2                  -> 4 e l1 + 4 e^2 + 4 u mse
    mape  : the denominator is >= 0.01 and itself off by e + 2 u          -> 2 e / 0.01 + mape (e / 0.01 + 4 u)
    smape : the same with 2 e in the denominator                         -> 2 e / 0.01 + smape (2 e / 0.01 + 4 u)
    grad  : four values and three subtractions of magnitude <= 1 each   -> 4 e + 3 u
  The fp64 accumulation adds 2^-53 per term: nothing visible.
Largest values seen are in DESIGN.md 10."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import metrics_ref as R
import metricscases as M
from conftest import beq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
K = dict(none=0, snorm=2, srgb=8, hdr=300)
SCALARS = ("mse", "psnr", "l1", "mape", "smape", "grad", "l1_msssim", "ssim", "msssim", "max_error", "num_errors", "nonfinite_a", "nonfinite_b",
           "exposure", "valid")
ARRAYS = ("ssim_c", "msssim_c", "mcs")


def same_bits(x, y):
    """two result dicts hold the same bits (NaN == NaN)"""
    return all(beq(np.float64(x[k]), np.float64(y[k])) for k in SCALARS) and all(beq(x[k], y[k]) for k in ARRAYS) and \
        (("map" in x) == ("map" in y)) and ("map" not in x or beq(x["map"], y["map"]))


def pointwise_bounds(A, transform):
    e = K[transform] * U
    return dict(l1=2 * e + 2 * U * A["l1"], mse=4 * e * A["l1"] + 4 * e * e + 4 * U * A["mse"], mape=2 * e / 0.01 + A["mape"] * (e / 0.01 + 4 * U),
                smape=2 * e / 0.01 + A["smape"] * (2 * e / 0.01 + 4 * U), grad=4 * e + 3 * U)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("shape", M.SHAPES, ids=M.shape_id)
def test_random_images_under_every_transform(gpu_product, shape):
    pt = gpu_product
    w, h = shape
    d = M.d_of_the_list()
    worst = dict(ssim=0.0, pointwise=0.0)
    with pt.Metrics(w, h) as m:
        for case in M.cases([shape]):
            _, dist, seed, transform = case
            a, b = M.images(shape, dist, seed)
            A, B = M.restated(case)
            got = m.host(a, b, transform=transform, exposure=M.EXPOSURE, want_map=min(shape) >= 11)
            print(case, {k: got[k] for k in ("mse", "l1", "mape", "smape", "grad", "ssim", "msssim")})
            assert got["valid"] == A["valid"] and got["nonfinite_a"] == got["nonfinite_b"] == 0
            assert got["num_errors"] == A["num_errors"] and got["max_error"] == B["max_error"]
            assert got["exposure"] == (M.EXPOSURE if transform == "hdr" else 1.0)
            for k, bound in pointwise_bounds(A, transform).items():
                if k == "grad" and min(shape) < 2:
                    assert math.isnan(got["grad"])
                    continue
                assert abs(got[k] - A[k]) <= bound, (case, k, got[k], A[k], bound)
                worst["pointwise"] = max(worst["pointwise"], abs(got[k] - A[k]))
            assert got["psnr"] == 10.0 * math.log10(1.0 / got["mse"])
            if min(shape) < 11:
                assert math.isnan(got["ssim"]) and math.isnan(got["msssim"]) and np.all(np.isnan(got["mcs"])) and np.all(np.isnan(got["ssim_c"]))
                continue
            diff = M.ssim_difference(got, A)
            worst["ssim"] = max(worst["ssim"], diff)
            assert diff <= 4 * d, (case, diff, d)
            assert got["map"].shape == (h - 10, w - 10) and beq(np.isnan(got["mcs"]), np.isnan(A["mcs"]))
            if min(shape) > 160:
                assert got["l1_msssim"] == 0.16 * got["l1"] + 0.84 * (1.0 - got["msssim"])
            else:
                assert math.isnan(got["msssim"]) and math.isnan(got["l1_msssim"])
    print("largest |gpu - A|: SSIM family %.4g (d = %.4g), pointwise %.4g" % (worst["ssim"], d, worst["pointwise"]))


@pytest.mark.parametrize("shape", [(1, 1), (11, 11), (27, 21), (161, 161), (200, 163)], ids=M.shape_id)
def test_an_image_against_itself_is_exact(gpu_product, shape):
    """mse 0, psnr +inf, no error counted, and SSIM and MS-SSIM exactly 1: xx, yy and xy are formed by the same operations"""
    pt = gpu_product
    _, b = M.images(shape, "uniform", 1)
    with pt.Metrics(*shape) as m:
        for transform in M.TRANSFORMS:
            r = m.host(b, b.copy(), transform=transform, exposure=2.0, want_map=min(shape) >= 11)
            assert r["mse"] == 0.0 and r["psnr"] == math.inf and r["l1"] == r["mape"] == r["smape"] == 0.0
            assert r["num_errors"] == 0 and r["max_error"] == 0.0
            if min(shape) >= 2:
                assert r["grad"] == 0.0
            if min(shape) >= 11:
                assert r["ssim"] == 1.0 and np.all(r["ssim_c"] == 1.0) and np.all(r["map"] == 1.0)
            if min(shape) > 160:
                assert r["msssim"] == 1.0 and np.all(r["mcs"] == 1.0) and r["l1_msssim"] == 0.0


@pytest.mark.parametrize("shape", [(10, 10), (12, 11), (27, 21), (193, 170), (161, 161)], ids=M.shape_id)
def test_values_on_a_grid_give_the_float64_bits(gpu_product, shape):
    """k / 16 in [0, 1] under NONE: every pointwise term is exact in fp32 and every sum exact in fp64, whatever its order"""
    pt = gpu_product
    w, h = shape
    rng = np.random.default_rng([7, w, h])
    a = (rng.integers(0, 17, (h, w, 3)) / 16.0).astype(np.float32)
    b = (rng.integers(0, 17, (h, w, 3)) / 16.0).astype(np.float32)
    A = R.metrics(a, b, np.float64, threshold=0.25)
    with pt.Metrics(w, h) as m:
        r = m.host(a, b, threshold=0.25)
    for k in ("mse", "l1", "grad", "num_errors", "max_error", "psnr"):
        assert beq(np.float64(r[k]), np.float64(A[k])), (k, r[k], A[k])
    assert 0 < r["num_errors"] < 3 * w * h and r["max_error"] == 1.0


def test_constant_images(gpu_product):
    """c1 against c2.  SSIM is the closed form (2 c1 c2 + C1) / (c1^2 + c2^2 + C1) times cs = 1.  In fp32 a filtered constant is c S with
    S the window's two-pass sum, off from 1 by at most 24 u (22 additions, two roundings of products that are exact here or not), and each
    of the five filtered values by its own 24 u: l moves by 4 * 24 u c^2 / (c1^2 + c2^2 + C1), cs by 4 * 24 u c^2 / C2 (c = the larger).
    cs = 1 holds on every scale only where no pool pads -- padded zeros make a constant image's border darker, the two images' borders
    by different amounts -- so the scales are held to 1 at 176 x 176 (176 -> 88 -> 44 -> 22 -> 11), and at 161 x 161, where every pool
    pads, scale 0 is and the lower ones are held to A within 4 d."""
    pt = gpu_product
    c1, c2 = 0.5, 0.25
    closed = (2 * c1 * c2 + R.C1) / (c1 * c1 + c2 * c2 + R.C1)
    cs_bound = 4 * 24 * U * c1 * c1 / R.C2
    l_bound = 4 * 24 * U * c1 * c1 / (c1 * c1 + c2 * c2 + R.C1)
    d = M.d_of_the_list()
    for (w, h) in ((11, 11), (27, 21), (176, 176), (161, 161)):
        a, b = np.full((h, w, 3), c1, np.float32), np.full((h, w, 3), c2, np.float32)
        with pt.Metrics(w, h) as m:
            r = m.host(a, b, want_map=True)
        print((w, h), r["ssim"] - closed, r["mcs"])
        assert abs(r["ssim"] - closed) <= l_bound + cs_bound and np.all(np.abs(r["map"] - closed) <= l_bound + cs_bound)
        assert r["mse"] == (c1 - c2) ** 2 and r["l1"] == c1 - c2 and r["grad"] == 0.0
        if (w, h) == (176, 176):
            assert np.all(np.abs(r["mcs"][:4] - 1.0) <= cs_bound) and np.all(np.abs(r["mcs"][4] - closed) <= l_bound + cs_bound)
        if (w, h) == (161, 161):
            A = R.metrics(a, b, np.float64)
            assert np.all(np.abs(r["mcs"][0] - 1.0) <= cs_bound) and np.all(np.abs(r["mcs"] - A["mcs"]) <= max(4 * d, cs_bound))
            assert abs(r["msssim"] - A["msssim"]) <= max(4 * d, cs_bound)


def test_layouts_give_the_packed_bits(gpu_product):
    """float4, half4, a row pitch and an offset; a half image is the packed float image of its widened values"""
    pt = gpu_product
    w, h = 27, 21
    a, b = M.images((w, h), "normal", 2)
    with pt.Metrics(w, h) as m:
        want = m.host(a, b, transform="srgb", want_map=True)
        a4 = np.full((h, w, 4), np.nan, np.float32); a4[..., :3] = a            # the fourth channel is never read into a result
        b4 = np.full((h, w, 4), np.inf, np.float32); b4[..., :3] = b
        assert same_bits(m.host(a4[..., :3], b4[..., :3], transform="srgb", want_map=True), want)
        pitched = np.full((h + 2, w + 5, 3), np.nan, np.float32)               # a row pitch and an offset: a window of a larger frame
        pitched[1:h + 1, 3:w + 3] = a
        assert same_bits(m.host(pitched[1:h + 1, 3:w + 3], b4[..., :3], transform="srgb", want_map=True), want)
        odd = np.full(3 * w * h + 1, np.nan, np.float32)                        # 4-byte aligned only
        odd[1:] = b.reshape(-1)
        assert same_bits(m.host(a, odd[1:].reshape(h, w, 3), transform="srgb", want_map=True), want)
        ah, bh = a.astype(np.float16), b.astype(np.float16)
        want_half = m.host(ah.astype(np.float32), bh.astype(np.float32), transform="hdr", want_map=True)
        assert same_bits(m.host(ah, bh, transform="hdr", want_map=True), want_half)
        h4 = np.zeros((h, w + 1, 4), np.float16); h4[:, 1:, :3] = ah
        assert same_bits(m.host(h4[:, 1:, :3], bh, transform="hdr", want_map=True), want_half)
        assert same_bits(m.host(ah, bh.astype(np.float32), transform="hdr", want_map=True), want_half)     # the two images' formats are their own
        assert not same_bits(want_half, m.host(a, b, transform="hdr", want_map=True))


def test_two_calls_and_another_stream_give_the_same_bits(gpu_product):
    import torch
    pt = gpu_product
    w, h = 193, 170
    a, b = M.images((w, h), "uniform", 3)
    da, db = _dev(a), _dev(b)
    ia = pt.nn_image_of(da.data_ptr(), format=pt.NN_FORMAT_FLOAT3)
    ib = pt.nn_image_of(db.data_ptr(), format=pt.NN_FORMAT_FLOAT3)
    dmap = torch.zeros((h - 10) * (w - 10), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    with pt.Metrics(w, h) as m:
        first = m.host(a, b, transform="hdr", want_map=True)
        assert same_bits(m.host(a, b, transform="hdr", want_map=True), first)
        on_default = m.device(ia, ib, transform="hdr", map_ptr=dmap.data_ptr())
        on_default["map"] = dmap.cpu().numpy().reshape(h - 10, w - 10)
        assert same_bits(on_default, first)
        other = torch.cuda.Stream()
        dmap.zero_()
        torch.cuda.synchronize()
        on_other = m.device(ia, ib, transform="hdr", map_ptr=dmap.data_ptr(), stream=other.cuda_stream)
        on_other["map"] = dmap.cpu().numpy().reshape(h - 10, w - 10)
        assert same_bits(on_other, first)
        with pt.Metrics(w, h) as fresh:                                       # and a handle that never held anything
            assert same_bits(fresh.host(a, b, transform="hdr", want_map=True), first)
        with pytest.raises(pt.PathTracerError, match="image a"):
            m.device(pt.nn_image_of(da.data_ptr(), format=pt.NN_FORMAT_FLOAT3, pixel_stride=8), ib)
        # the pointwise metrics alone: the same bits, the SSIM family left out
        alone = m.host(a, b, transform="hdr", pointwise_only=1)
        assert all(beq(np.float64(alone[k]), np.float64(first[k])) for k in ("mse", "psnr", "l1", "mape", "smape", "grad", "max_error", "num_errors"))
        assert alone["valid"] == R.VALID_GRAD and math.isnan(alone["ssim"]) and math.isnan(alone["msssim"]) and np.all(np.isnan(alone["mcs"]))
        with pytest.raises(pt.PathTracerError, match="pointwise_only"):
            m.host(a, b, want_map=True, pointwise_only=1)


def test_non_finite_inputs_are_counted_and_sanitised(gpu_product):
    pt = gpu_product
    w, h = 27, 21
    a, b = M.images((w, h), "uniform", 1)
    a, b = a.copy(), b.copy()
    a[0, 0, 0], a[3, 4, 1], a[5, 5, 2], a[20, 26, 0] = np.nan, np.inf, -np.inf, np.nan
    b[1, 1, 1], b[7, 2, 0], b[9, 9, 2] = np.nan, np.inf, -np.inf
    clean_a = np.nan_to_num(a, nan=0.0, posinf=R.FLT_MAX, neginf=-R.FLT_MAX)
    clean_b = np.nan_to_num(b, nan=0.0, posinf=R.FLT_MAX, neginf=-R.FLT_MAX)
    with pt.Metrics(w, h) as m:
        for transform in M.TRANSFORMS:
            r = m.host(a, b, transform=transform, exposure=1.5, want_map=True)
            assert (r["nonfinite_a"], r["nonfinite_b"]) == (4, 3)
            for k in ("mse", "psnr", "l1", "mape", "smape", "grad", "max_error"):
                assert not math.isnan(r[k]), (transform, k)
            # a set bit means a number.  Under HDR every sample is at most 1 and SSIM is one; elsewhere a sanitised infinity squares to
            # +inf inside the window, SSIM is inf - inf as in ssim.py, and its bit is clear
            assert r["valid"] & R.VALID_GRAD and not r["valid"] & R.VALID_MSSSIM
            assert bool(r["valid"] & R.VALID_SSIM) == (not math.isnan(r["ssim"])) == (transform == "hdr"), (transform, r["ssim"])
            if transform == "hdr":
                assert not np.any(np.isnan(r["ssim_c"])) and not np.any(np.isnan(r["map"]))
            want = m.host(clean_a, clean_b, transform=transform, exposure=1.5, want_map=True)
            assert (want["nonfinite_a"], want["nonfinite_b"]) == (0, 0)
            want["nonfinite_a"], want["nonfinite_b"] = 4, 3
            assert same_bits(r, want)                                          # sanitised as defined: the values np.nan_to_num gives
            B = R.metrics(a, b, np.float32, transform, exposure=1.5)
            assert r["num_errors"] == B["num_errors"] and r["max_error"] == B["max_error"] and r["valid"] == B["valid"]
        none = m.host(a, b)
        assert none["max_error"] == float(np.float32(R.FLT_MAX)) and none["mse"] == math.inf


def test_the_automatic_exposure_is_the_display_meter_of_b(gpu_product):
    pt = gpu_product
    w, h = 97, 61
    rng = np.random.default_rng(11)
    b = (10.0 ** rng.normal(0.0, 0.7, (h, w, 1)) * rng.uniform(0.3, 1.5, (h, w, 3))).astype(np.float32)
    a = (b * rng.uniform(0.8, 1.25, (h, w, 3))).astype(np.float32)
    with pt.Metrics(w, h) as m, pt.Display(w, h) as D:
        D.host(b * np.float32(3), 3)
        metered = D.status()["metered"]
        r = m.host(a, b * np.float32(3), transform="hdr", samples_b=3)
        assert beq(np.float32(r["exposure"]), np.float32(metered)) and metered != 1.0
        assert same_bits(m.host(a, b * np.float32(3), transform="hdr", exposure=metered, samples_b=3), r)
        b4 = np.zeros((h, w, 4), np.float32); b4[..., :3] = b * np.float32(3)   # a layout that is gathered for the meter
        assert same_bits(m.host(a, b4[..., :3], transform="hdr", samples_b=3), r)
        A = R.metrics(a, b * np.float32(3), np.float64, "hdr", exposure=metered, samples_b=3)
        assert abs(r["ssim"] - A["ssim"]) <= 4 * M.d_of_the_list() and abs(r["l1"] - A["l1"]) <= 4 * K["hdr"] * U


def _scene(pt, res):
    s = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"), res=res, depth=4)
    s.apply_runcuda_camera()
    return s


def test_through_the_tracer(gpu_product):
    """Tracer.compare is Metrics.host of the frame read back, for both sources, and the tracer goes on as one that never saw the call"""
    pt = gpu_product
    W, H, spp = 64, 48, 4
    s = _scene(pt, (W, H))
    ref = np.random.default_rng(3).uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    with pt.Metrics(W, H) as m, pt.Metrics(W, H) as mh, pt.Tracer(s) as T, pt.Tracer(s) as plain:
        T.render(1, spp)
        plain.render(1, spp)
        with pytest.raises(pt.PathTracerError, match="no ptx_denoise"):
            T.compare(m, ref, spp, source="denoised")
        for transform in ("none", "hdr"):
            got = T.compare(m, ref, spp, transform=transform)
            frame = T.read_image().reshape(H, W, 3)
            assert same_bits(got, mh.host(frame / np.float32(spp), ref, transform=transform))
            assert same_bits(got, mh.host(frame, ref, transform=transform, samples_a=spp)) and got["mse"] > 0
        den = T.denoise(spp)
        plain.denoise(spp)
        got = T.compare(m, ref, spp, source="denoised", transform="srgb")
        assert same_bits(got, mh.host(np.asarray(den).reshape(H, W, 3), ref, transform="srgb"))
        assert beq(T.read_image(), plain.read_image()) and beq(T.read_denoised(), plain.read_denoised())
        assert T.stats()["rays_per_bounce"] == plain.stats()["rays_per_bounce"]
        T.render(spp + 1, 2)
        plain.render(spp + 1, 2)
        assert beq(T.read_image(), plain.read_image()) and T.stats()["rays_per_bounce"] == plain.stats()["rays_per_bounce"]
        with pt.Metrics(W + 1, H) as other, pytest.raises(pt.PathTracerError, match="size"):
            T.compare(other, np.zeros((H, W + 1, 3), np.float32), spp)
        with pytest.raises(pt.PathTracerError, match="spp"):
            T.compare(m, ref, 0)


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0                                          # little-endian
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)[::-1].copy()     # the bottom row is stored first


def _metrics_line(out):
    lines = [l for l in out.splitlines() if l.startswith("metrics: ")]
    assert len(lines) == 1, out
    got = json.loads(lines[0][len("metrics: "):])
    return {k: np.array(v) if isinstance(v, list) else v for k, v in got.items()}


def test_the_drivers_compare_line_is_the_python_call_on_the_files_it_wrote(gpu_product, tmp_path):
    pt = gpu_product
    exe = os.path.join(ROOT, "mygpuraytracer_amd", "mi355x_pathtrace")
    W, H = 64, 48
    scene = os.path.join(ROOT, "scenes", "cornell.txt")
    base = [exe, scene, "--res", str(W), str(H), "--depth", "4", "--pfm"]
    first = subprocess.run(base + ["--iterations", "8", "--out", str(tmp_path / "ref")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert first.returncode == 0, first.stderr[-2000:]
    ref = [p for p in os.listdir(tmp_path) if p.startswith("ref.") and p.endswith(".pfm")]
    assert len(ref) == 1
    ref = str(tmp_path / ref[0])
    run = subprocess.run(base + ["--iterations", "2", "--denoise", "--out", str(tmp_path / "test"), "--compare", ref, "--compare-denoised",
                                 "--compare-transform", "hdr", "--compare-threshold", "0.05"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = _metrics_line(run.stdout)
    den = [p for p in os.listdir(tmp_path) if p.startswith("test.") and p.endswith(".denoised.pfm")]
    assert len(den) == 1
    a, b = _read_pfm(str(tmp_path / den[0])), _read_pfm(ref)
    with pt.Metrics(W, H) as m:
        want = m.host(a, b, transform="hdr", threshold=0.05)
        assert same_bits(got, want) and 0 < want["ssim"] < 1 and want["exposure"] != 1.0
        plain = subprocess.run(base + ["--iterations", "2", "--out", str(tmp_path / "plain"), "--compare", ref], stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, timeout=120)
        assert plain.returncode == 0, plain.stderr[-2000:]
        frame = [p for p in os.listdir(tmp_path) if p.startswith("plain.") and p.endswith(".pfm")]
        assert same_bits(_metrics_line(plain.stdout), m.host(_read_pfm(str(tmp_path / frame[0])), b))
        files = subprocess.run([exe, "--compare-files", str(tmp_path / frame[0]), ref, "--compare-transform", "srgb"], stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, timeout=120)
        assert files.returncode == 0, files.stderr[-2000:]
        assert same_bits(_metrics_line(files.stdout), m.host(_read_pfm(str(tmp_path / frame[0])), b, transform="srgb"))
