"""The image metrics (include/mi355x_pathtracer.h, "image metrics") restated in numpy, twice from one text: A in float64 (`metrics(..,
np.float64)`: what the real numbers give, to double rounding) and B in float32 (`metrics(.., np.float32)`: every term one IEEE fp32
operation in the kernels' order, the sums in float64 as the kernels add them).  Inputs are float32 (or float16, widened) arrays of
shape (H, W, 3).  Nothing here calls the library but for the eleven window taps, which are data of the plan."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
NONE, SRGB, HDR, SNORM = 0, 1, 2, 3
TRANSFORMS = {"none": NONE, "srgb": SRGB, "hdr": HDR, "snorm": SNORM}
VALID_SSIM, VALID_MSSSIM, VALID_GRAD = 1, 2, 4
WIN, SCALES = 11, 5
# training/ssim.py's window as torch forms it in float32 (the public header says why the floats, not the formula, are the definition)
TAPS = np.array([float.fromhex(h) for h in ("0x1.0d957p-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.10656p-2",
                                            "0x1.b43c3ep-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d957p-10")], np.float32)
WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], np.float32)
C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
X_CAP = 2.0 ** 60


def sanitise(raw, samples, T):
    """np.nan_to_num of raw / samples, the infinities to +-FLT_MAX whatever T is"""
    with np.errstate(all="ignore"):
        s = raw.astype(T) / T(np.float32(samples))
    return np.nan_to_num(s, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX).astype(T)


def srgb_forward(y, T):
    with np.errstate(all="ignore"):
        hi = T(np.float32(1.055)) * np.power(np.maximum(y, T(0)), T(np.float32(1.0 / 2.4))) + T(np.float32(-0.055))
        return np.where(y <= T(np.float32(0.0031308)), T(np.float32(12.92)) * y, hi).astype(T)


def tonemap(x, T):
    """Hable's curve with OIDN's constants (training/color.py), formed in double and, for float32, rounded once each"""
    A, B, C, D, E, F, W = 0.22, 0.30, 0.10, 0.20, 0.01, 0.30, 11.2
    k = lambda v: T(np.float32(v)) if T is np.float32 else T(v)
    a, b, cb, de, df, ef = k(A), k(B), k(C * B), k(D * E), k(D * F), k(E / F)
    white = k(((W * (A * W + C * B) + D * E) / (W * (A * W + B) + D * F)) - E / F)
    with np.errstate(all="ignore"):
        v = np.clip(x * k(1.758141), T(-X_CAP), T(X_CAP))
        e = ((v * (a * v + cb) + de) / (v * (a * v + b) + df)) - ef
        return np.fmin(e / white, T(1)).astype(T)


def transform(s, mode, exposure, T):
    if mode == NONE:
        return s
    if mode == SNORM:
        return s * T(0.5) + T(0.5)
    if mode == HDR:
        with np.errstate(all="ignore"):
            s = tonemap(s * T(np.float32(exposure)), T)
    return np.clip(srgb_forward(s, T), T(-FLT_MAX), T(FLT_MAX))              # an infinite result is held to +-FLT_MAX


def compare_image(sa, sb, threshold, T):
    """apps/utils/image_io.cpp:435-462 as written: (num_errors, max_error)"""
    with np.errstate(all="ignore"):
        err = np.abs(sb - sa)
        rel = err / sb
        err = np.where((sb != 0) & (rel < err), rel, err)
    return int(np.count_nonzero(err > T(np.float32(threshold)))), float(max(0.0, err.max()))


def filter_valid(img, T):
    """(C, H, W) -> (C, H - 10, W - 10): the window along x, then along y, each a left-to-right sum of products"""
    taps = TAPS.astype(T)
    w = img.shape[2] - (WIN - 1)
    acc = np.zeros(img.shape[:2] + (w,), T)
    for k in range(WIN):
        acc = acc + taps[k] * img[:, :, k:k + w]
    h = img.shape[1] - (WIN - 1)
    out = np.zeros((img.shape[0], h, w), T)
    for k in range(WIN):
        out = out + taps[k] * acc[:, k:k + h, :]
    return out


def ssim_maps(x, y, T):
    """planar (3, H, W) -> (cs, l * cs), each (3, H - 10, W - 10)"""
    c1, c2 = (T(np.float32(C1)), T(np.float32(C2))) if T is np.float32 else (T(C1), T(C2))
    with np.errstate(all="ignore"):                      # (samples near FLT_MAX overflow here as they do on the device)
        m1, m2 = filter_valid(x, T), filter_valid(y, T)
        fxx, fyy, fxy = filter_valid(x * x, T), filter_valid(y * y, T), filter_valid(x * y, T)
        m11, m22, m12 = m1 * m1, m2 * m2, m1 * m2
        s1, s2, s12 = fxx - m11, fyy - m22, fxy - m12
        cs = (T(2) * s12 + c2) / ((s1 + s2) + c2)
        full = ((T(2) * m12 + c1) / ((m11 + m22) + c1)) * cs
    return cs, full


def pooled_size(n):
    p = n % 2
    return (n + 2 * p - 2) // 2 + 1


def pool(img, T):
    """avg_pool2d(kernel 2, padding (H % 2, W % 2)) of (C, H, W) as PyTorch defines it: zeros on both sides, a divisor of 4"""
    c, h, w = img.shape
    ph, pw = h % 2, w % 2
    hd, wd = pooled_size(h), pooled_size(w)
    pad = np.zeros((c, 2 * hd + 2, 2 * wd + 2), T)
    pad[:, ph:ph + h, pw:pw + w] = img
    q = [pad[:, dy:dy + 2 * hd:2, dx:dx + 2 * wd:2] for dy in (0, 1) for dx in (0, 1)]
    return (((q[0] + q[1]) + q[2]) + q[3]) * T(0.25)


def mean64(a):
    return float(np.sum(a.astype(np.float64), dtype=np.float64) / a.size)


def metrics(a, b, T=np.float64, transform_mode=NONE, exposure=1.0, threshold=0.01, samples_a=1.0, samples_b=1.0, want_map=False):
    """Every field of ptx_metrics_result as a dict (arrays as numpy arrays); exposure is the one in use (the meter is not restated
    here: tests/display_ref.py has it)."""
    mode = TRANSFORMS[transform_mode] if isinstance(transform_mode, str) else transform_mode
    a, b = np.asarray(a), np.asarray(b)
    h, w = a.shape[:2]
    r = dict(nonfinite_a=int(np.count_nonzero(~np.isfinite(a[..., :3]))), nonfinite_b=int(np.count_nonzero(~np.isfinite(b[..., :3]))),
             exposure=np.float32(exposure if mode == HDR else 1.0), valid=0)
    sa, sb = sanitise(a[..., :3].astype(np.float32), samples_a, T), sanitise(b[..., :3].astype(np.float32), samples_b, T)
    r["num_errors"], r["max_error"] = compare_image(sa, sb, threshold, T)
    ta, tb = transform(sa, mode, exposure, T), transform(sb, mode, exposure, T)
    with np.errstate(all="ignore"):
        d = ta - tb
        ad = np.abs(d)
        r["mse"], r["l1"] = mean64(d * d), mean64(ad)
        r["mape"] = mean64(ad / (np.abs(tb) + T(np.float32(0.01))))
        r["smape"] = mean64(ad / ((np.abs(ta) + np.abs(tb)) + T(np.float32(0.01))))
        r["psnr"] = float(10.0 * np.log10(np.float64(1.0) / np.float64(r["mse"])))
    nan = float("nan")
    r["grad"] = nan
    if w >= 2 and h >= 2:
        gy = (ta[1:, :-1] - ta[:-1, :-1]) - (tb[1:, :-1] - tb[:-1, :-1])
        gx = (ta[:-1, 1:] - ta[:-1, :-1]) - (tb[:-1, 1:] - tb[:-1, :-1])
        r["grad"] = float((np.sum(np.abs(gy).astype(np.float64)) + np.sum(np.abs(gx).astype(np.float64))) / (2 * gy.size))
        r["valid"] |= VALID_GRAD
    r["ssim"] = r["msssim"] = r["l1_msssim"] = nan
    r["ssim_c"], r["msssim_c"], r["mcs"] = np.full(3, nan), np.full(3, nan), np.full((SCALES, 3), nan)
    x, y = np.ascontiguousarray(ta.transpose(2, 0, 1)), np.ascontiguousarray(tb.transpose(2, 0, 1))
    if min(w, h) >= WIN:
        cs, full = ssim_maps(x, y, T)
        r["ssim_c"] = np.array([mean64(full[c]) for c in range(3)])
        r["ssim"] = float(((r["ssim_c"][0] + r["ssim_c"][1]) + r["ssim_c"][2]) / 3.0)
        r["valid"] |= VALID_SSIM
        if want_map:
            r["map"] = (((full[0] + full[1]) + full[2]) / T(3)).astype(T)
        if min(w, h) > (WIN - 1) * 16:
            for s in range(SCALES):
                if s:
                    x, y = pool(x, T), pool(y, T)
                    cs, full = ssim_maps(x, y, T)
                which = cs if s < SCALES - 1 else full
                r["mcs"][s] = [mean64(which[c]) for c in range(3)]
            r["msssim_c"] = np.prod(np.power(np.maximum(r["mcs"], 0.0), WEIGHTS.astype(np.float64)[:, None]), axis=0)
            r["msssim"] = float(((r["msssim_c"][0] + r["msssim_c"][1]) + r["msssim_c"][2]) / 3.0)
            r["l1_msssim"] = 0.16 * r["l1"] + 0.84 * (1.0 - r["msssim"])
            r["valid"] |= VALID_MSSSIM
    for k, bit in (("grad", VALID_GRAD), ("ssim", VALID_SSIM), ("msssim", VALID_MSSSIM)):
        if np.isnan(r[k]):
            r["valid"] &= ~bit                                                 # a set bit means a number
    return r
