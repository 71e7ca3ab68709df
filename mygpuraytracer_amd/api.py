"""ctypes host side over the C ABI of libmi355x_pathtracer.so (include/mi355x_pathtracer.h,
include/mi355x_stream_compaction.h).

Mirrors the reference's interface for the path (nkkk98/MyGPURaytracer):

* ``Scene(path)``                      <->  ``new Scene(sceneFile)``                (src/scene.cpp:10, src/main.cpp:47)
* ``Scene.apply_runcuda_camera()``     <->  first ``runCuda()`` camera recompute    (src/main.cpp:105-123)
* ``Tracer(scene, options)``           <->  ``pathtraceInit(scene)``                (src/pathtrace.cu:101)
* ``Tracer.pathtrace(iter)``           <->  ``pathtrace(pbo, frame, iter)``         (src/pathtrace.cu:433)
* ``Tracer.close()``                   <->  ``pathtraceFree()``                     (src/pathtrace.cu:159)
* ``Tracer.last_loop_ms()``            <->  ``timer().getGpuElapsedTimeForPreviousOperation()``
* ``StreamCompaction.*``               <->  ``StreamCompaction::{CPU,Naive,Efficient,Thrust}::*``

Nothing here computes: every call goes through the library, and there is no CPU fallback.
"""
import ctypes as C
import os
import sys
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libmi355x_pathtracer.so")
# A/B timing of variant builds (tools/ab_*.sh): PTX_AB_LIBRARY names another build of the SAME library to load instead, so that the
# scripts no longer overwrite the in-tree product (an interrupted run used to leave a variant in its place).  Development only, and
# behind a second switch: without PTX_DEV=1 the variable is REFUSED (round 4's one GPU fault came through this door -- a test run
# against a stale variant build), so that neither a test run nor the driver can pick up anything but the in-tree product by accident.
if os.environ.get("PTX_AB_LIBRARY"):
    if os.environ.get("PTX_DEV") != "1":
        raise ImportError("PTX_AB_LIBRARY is set (%s) without PTX_DEV=1: variant builds are loaded for A/B timing only; unset it or "
                          "set PTX_DEV=1" % os.environ["PTX_AB_LIBRARY"])
    LIB_PATH = os.path.abspath(os.environ["PTX_AB_LIBRARY"])

PTX_OK = 0
ABI_VERSION = 5          # include/mi355x_pathtracer.h: PTX_ABI_VERSION
vp = C.c_void_p


class PathTracerError(RuntimeError):
    pass


class Cancelled(PathTracerError):
    """PTX_ERR_CANCELLED: a network denoiser's progress monitor (NN.set_progress) returned a falsy value"""


PTX_ERR_CANCELLED = 6
NN_PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double)      # ptx_nn_progress_fn


class Material(C.Structure):
    _fields_ = [("color", C.c_float * 3), ("specular_exponent", C.c_float), ("specular_color", C.c_float * 3),
                ("hasReflective", C.c_float), ("hasRefractive", C.c_float), ("indexOfRefraction", C.c_float),
                ("emittance", C.c_float)]


class Texture(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("image", C.POINTER(C.c_uint8))]


class Geom(C.Structure):
    _fields_ = [("type", C.c_int32), ("materialid", C.c_int32),
                ("translation", C.c_float * 3), ("rotation", C.c_float * 3), ("scale", C.c_float * 3),
                ("transform", C.c_float * 16), ("inverseTransform", C.c_float * 16), ("invTranspose", C.c_float * 16),
                ("faceSize", C.c_int32), ("faces", C.POINTER(C.c_float)),
                ("kd", Texture), ("ks", Texture), ("bump", Texture), ("ke", Texture)]


class Camera(C.Structure):
    _fields_ = [("resolution", C.c_int32 * 2), ("position", C.c_float * 3), ("lookAt", C.c_float * 3),
                ("view", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3), ("fov", C.c_float * 2),
                ("pixelLength", C.c_float * 2)]


class Options(C.Structure):
    """Runtime form of the #defines of src/pathtrace.cu:36-40 (+ the multi-GPU row-tile split)."""
    _fields_ = [("depth_of_field", C.c_int32), ("cache_first_bounce", C.c_int32), ("sort_by_material", C.c_int32),
                ("antialiasing", C.c_int32), ("bounding_box", C.c_int32),
                ("tile_rows", C.c_int32), ("tile_rank", C.c_int32), ("tile_world", C.c_int32),
                ("device", C.c_int32), ("batch", C.c_int32), ("no_lds_triangles", C.c_int32), ("apps_variant", C.c_int32), ("no_cull", C.c_int32), ("no_bvh", C.c_int32), ("lanes", C.c_int32), ("no_mesh_split", C.c_int32), ("arith", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("bounces", C.c_int32), ("rays_per_bounce", C.c_int64 * 64), ("rays_total", C.c_int64),
                ("loop_ms_total", C.c_double), ("iterations", C.c_int64), ("fenced", C.c_int64),
                ("stored_paths", C.c_int64), ("stored_with_direction", C.c_int64), ("stored_with_normal_code", C.c_int64)]


class DenoiseParams(C.Structure):
    """ptx_denoise_params: the a-trous denoiser's knobs (include/mi355x_pathtracer.h; defaults from ptx_default_denoise_params)."""
    _fields_ = [("passes", C.c_int32), ("demodulate", C.c_int32), ("phi_color", C.c_float), ("phi_normal", C.c_float),
                ("phi_position", C.c_float)]


def _default_params(struct, c_function, int_fields, **kw):
    """a parameter struct filled by the library's ptx_default_* function, then the keyword overrides that are not None"""
    p = struct()
    getattr(load_library(), c_function)(C.byref(p))
    for k, v in kw.items():
        if v is None:
            continue
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, int(v) if k in int_fields else float(v))
    return p


def default_denoise_params(**kw):
    """ptx_default_denoise_params with keyword overrides (passes, demodulate, phi_color, phi_normal, phi_position)."""
    return _default_params(DenoiseParams, "ptx_default_denoise_params", ("passes", "demodulate"), **kw)


class TemporalParams(C.Structure):
    """ptx_temporal_params: temporal reuse in front of the denoiser (include/mi355x_pathtracer.h; defaults from
    ptx_default_temporal_params)."""
    _fields_ = [("max_history", C.c_int32), ("specular_history", C.c_int32), ("normal_cos", C.c_float), ("plane_tolerance", C.c_float)]


def default_temporal_params(**kw):
    """ptx_default_temporal_params with keyword overrides (max_history, specular_history, normal_cos, plane_tolerance)."""
    return _default_params(TemporalParams, "ptx_default_temporal_params", ("max_history", "specular_history"), **kw)


class VarianceParams(C.Structure):
    """ptx_variance_params: variance guidance of the a-trous filter (include/mi355x_pathtracer.h; defaults from
    ptx_default_variance_params)."""
    _fields_ = [("phi_luminance", C.c_float), ("epsilon", C.c_float), ("spatial_radius", C.c_int32), ("prefilter", C.c_int32)]


_DENOISE_KEYS = ("passes", "demodulate", "phi_color", "phi_normal", "phi_position")
_TEMPORAL_KEYS = ("max_history", "specular_history", "normal_cos", "plane_tolerance")
_VARIANCE_KEYS = ("phi_luminance", "epsilon", "spatial_radius", "prefilter")


def default_variance_params(**kw):
    """ptx_default_variance_params with keyword overrides (phi_luminance, epsilon, spatial_radius, prefilter)."""
    return _default_params(VarianceParams, "ptx_default_variance_params", ("spatial_radius", "prefilter"), **kw)


def _split_variance_params(fn, params):
    """keyword arguments of the variance entry points -> (DenoiseParams, TemporalParams, VarianceParams)"""
    for k in params:
        if k not in _DENOISE_KEYS + _TEMPORAL_KEYS + _VARIANCE_KEYS:
            raise TypeError("%s: unknown parameter %r" % (fn, k))
    pick = lambda keys: {k: v for k, v in params.items() if k in keys}
    return (default_denoise_params(**pick(_DENOISE_KEYS)), default_temporal_params(**pick(_TEMPORAL_KEYS)),
            default_variance_params(**pick(_VARIANCE_KEYS)))


class _Owned:
    """An object that owns one native handle: `lib`, the loaded library, and `h`, the handle (None once closed, absent while the create
    call has not succeeded).  _destroy names the library function that frees it."""
    _destroy = None

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Temporal(_Owned):
    """The history of one W x H view sequence on one device (opaque ptx_temporal), for Tracer.denoise_temporal.  It outlives any
    tracer: hand the same handle to a new Tracer after a camera change and the previous view's samples are reused."""
    _destroy = "ptx_temporal_destroy"

    def __init__(self, device, width, height):
        self.lib = load_library()
        h = vp()
        _check(self.lib.ptx_temporal_create(int(device), int(width), int(height), C.byref(h)), "ptx_temporal_create")
        self.h = h
        self.device, self.width, self.height = int(device), int(width), int(height)

    def reset(self):
        """forget all history: the next denoise_temporal is Tracer.denoise bit for bit"""
        _check(self.lib.ptx_temporal_reset(self.h), "ptx_temporal_reset")

    def read(self):
        """The last call's reprojected history h (H, W, 3), its sample count n_h (H, W) and the mix (H, W, 3) the filter took."""
        hh, ww = self.height, self.width
        hist, count, mix = np.zeros((hh, ww, 3), np.float32), np.zeros((hh, ww), np.float32), np.zeros((hh, ww, 3), np.float32)
        _check(self.lib.ptx_temporal_read(self.h, _ptr(hist), _ptr(count), _ptr(mix)), "ptx_temporal_read")
        return dict(history=hist, count=count, mix=mix)


class MomentsParams(C.Structure):
    """ptx_moments_params: the error summary's floor and threshold (include/mi355x_pathtracer.h; defaults from
    ptx_default_moments_params)."""
    _fields_ = [("floor", C.c_float), ("threshold", C.c_float)]


class MomentsSummary(C.Structure):
    """ptx_moments_summary (include/mi355x_pathtracer.h)."""
    _fields_ = [("pixels", C.c_int64), ("pixels_over", C.c_int64), ("samples", C.c_int64), ("mean_rel_se", C.c_double),
                ("rms_rel_se", C.c_double), ("max_rel_se", C.c_double), ("mean_variance", C.c_double), ("batches", C.c_int32),
                ("reserved", C.c_int32)]


def default_moments_params(**kw):
    """ptx_default_moments_params with keyword overrides (floor, threshold)."""
    return _default_params(MomentsParams, "ptx_default_moments_params", (), **kw)


class Moments(_Owned):
    """Per-pixel sample moments by batch means on one device (opaque ptx_moments): add(tracer, samples) whenever `samples` iterations
    are in the tracer's accumulation buffer, then summary() for the frame's error estimate, read() for the per-pixel mean and
    covariance, or Tracer.denoise_measured(moments, spp).  After Tracer.reset_image call reset()."""
    _destroy = "ptx_moments_destroy"

    def __init__(self, device, width, height):
        self.lib = load_library()
        h = vp()
        _check(self.lib.ptx_moments_create(int(device), int(width), int(height), C.byref(h)), "ptx_moments_create")
        self.h = h
        self.device, self.width, self.height = int(device), int(width), int(height)

    def reset(self):
        """forget everything: the next add takes the whole buffer as one batch"""
        _check(self.lib.ptx_moments_reset(self.h), "ptx_moments_reset")

    def add(self, tracer, samples):
        """one batch: what the tracer's accumulation buffer gained since the last add; `samples` = the iterations it holds now
        (enqueued on the tracer's stream)"""
        _check(self.lib.ptx_moments_add(self.h, tracer.h, int(samples)), "ptx_moments_add")

    def add_host(self, rgb_sum, samples):
        """the same from a host frame, (H, W, 3) or (H*W, 3) float32 sums of `samples` samples (synchronous)"""
        rgb = np.ascontiguousarray(rgb_sum, np.float32)
        if rgb.size != self.width * self.height * 3:
            raise PathTracerError("Moments.add_host: the frame must hold %d x %d x 3 floats" % (self.width, self.height))
        _check(self.lib.ptx_moments_add_host(self.h, _ptr(rgb), int(samples)), "ptx_moments_add_host")

    def add_host_tiled(self, rgb_sum, tile_samples):
        """add_host in which every tile of tile_pixels() pixels advances by its own amount (ptx_moments_add_host_tiled): tile_samples[tile]
        = the samples its pixels hold now; a tile whose total did not move keeps its state bit for bit (synchronous)"""
        rgb = np.ascontiguousarray(rgb_sum, np.float32)
        if rgb.size != self.width * self.height * 3:
            raise PathTracerError("Moments.add_host_tiled: the frame must hold %d x %d x 3 floats" % (self.width, self.height))
        ts = np.ascontiguousarray(tile_samples, np.int64).reshape(-1)
        _check(self.lib.ptx_moments_add_host_tiled(self.h, _ptr(rgb), _ptr(ts), len(ts)), "ptx_moments_add_host_tiled")

    def read(self):
        """dict of mean (H, W, 3), cov (H, W, 6: rr, gg, bb, rg, rb, gb of the per-sample covariance, 0 where batches < 2), batches
        (H, W) int32 and samples (int)"""
        hh, ww = self.height, self.width
        mean, cov, b = np.zeros((hh, ww, 3), np.float32), np.zeros((hh, ww, 6), np.float32), np.zeros((hh, ww), np.int32)
        n = C.c_int64(0)
        _check(self.lib.ptx_moments_read(self.h, _ptr(mean), _ptr(cov), _ptr(b), C.byref(n)), "ptx_moments_read")
        return dict(mean=mean, cov=cov, batches=b, samples=int(n.value))

    def read_samples(self):
        """(H, W) int32: the samples every pixel's moments hold (they differ between tiles after add_host_tiled / Adaptive.add)"""
        out = np.zeros((self.height, self.width), np.int32)
        _check(self.lib.ptx_moments_read_samples(self.h, _ptr(out)), "ptx_moments_read_samples")
        return out

    def summary(self, **params):
        """ptx_moments_summarize as a dict; params: floor, threshold"""
        p, out = default_moments_params(**params), MomentsSummary()
        _check(self.lib.ptx_moments_summarize(self.h, C.byref(p), C.byref(out)), "ptx_moments_summarize")
        return {k: getattr(out, k) for k, _ in MomentsSummary._fields_ if k != "reserved"}


class AdaptiveParams(C.Structure):
    """ptx_adaptive_params: when a tile stops (include/mi355x_pathtracer.h; defaults from ptx_default_adaptive_params)."""
    _fields_ = [("target", C.c_float), ("floor", C.c_float), ("min_batches", C.c_int32), ("max_samples", C.c_int32)]


class AdaptiveStatus(C.Structure):
    """ptx_adaptive_status (include/mi355x_pathtracer.h)."""
    _fields_ = [("samples_total", C.c_int64), ("pixels_active", C.c_int64), ("tiles", C.c_int32), ("tiles_active", C.c_int32),
                ("samples_min", C.c_int32), ("samples_max", C.c_int32), ("worst_error", C.c_float), ("rounds", C.c_int32)]


def default_adaptive_params(**kw):
    """ptx_default_adaptive_params with keyword overrides (target, floor, min_batches, max_samples)."""
    return _default_params(AdaptiveParams, "ptx_default_adaptive_params", ("min_batches", "max_samples"), **kw)


def tile_pixels():
    """ptx_tile_pixels: the pixels of one tile of the active-tile mask, tile = (y * W + x) // tile_pixels()"""
    return int(load_library().ptx_tile_pixels())


class Adaptive(_Owned):
    """Adaptive sampling by tiles on one device (opaque ptx_adaptive): render(tracer, moments) traces until every tile's measured error
    is at its target, or step by step add(moments, tracer, k) after every k iterations, select(moments, tracer) for the next mask,
    resolve(tracer) and read() for the frame; Tracer.denoise_adaptive(adaptive, moments) filters it.  Reset it together with the Moments
    it is used with."""
    _destroy = "ptx_adaptive_destroy"

    def __init__(self, device, width, height):
        self.lib = load_library()
        h = vp()
        _check(self.lib.ptx_adaptive_create(int(device), int(width), int(height), C.byref(h)), "ptx_adaptive_create")
        self.h = h
        self.device, self.width, self.height = int(device), int(width), int(height)
        self.num_tiles = int(self.lib.ptx_adaptive_num_tiles(h))

    def reset(self):
        """every tile active with 0 samples, as after create"""
        _check(self.lib.ptx_adaptive_reset(self.h), "ptx_adaptive_reset")

    def add(self, moments, tracer, k):
        """the tracer's last k iterations were rendered under the current mask: counts them and folds them into `moments` tile by tile"""
        _check(self.lib.ptx_adaptive_add(self.h, moments.h, tracer.h, int(k)), "ptx_adaptive_add")

    def select(self, moments, tracer, params=None, **kw):
        """decides which tiles go on and makes that the tracer's mask; returns the status as a dict.  params: an AdaptiveParams, or its
        fields as keywords (target, floor, min_batches, max_samples)"""
        p = params if params is not None else default_adaptive_params(**kw)
        out = AdaptiveStatus()
        _check(self.lib.ptx_adaptive_select(self.h, moments.h, tracer.h, C.byref(p), C.byref(out)), "ptx_adaptive_select")
        return {k: getattr(out, k) for k, _ in AdaptiveStatus._fields_}

    def resolve(self, tracer):
        """the tracer's accumulation buffer over each tile's own sample count, into the handle's frame (enqueued)"""
        _check(self.lib.ptx_adaptive_resolve(self.h, tracer.h), "ptx_adaptive_resolve")

    def read(self):
        """dict of mean (H, W, 3) float32 = the last resolve's frame, samples (H, W) int32, tile_error (tiles) float32, tile_active
        (tiles) bool"""
        hh, ww = self.height, self.width
        mean, spp = np.zeros((hh, ww, 3), np.float32), np.zeros((hh, ww), np.int32)
        err, act = np.zeros(self.num_tiles, np.float32), np.zeros(self.num_tiles, np.uint8)
        _check(self.lib.ptx_adaptive_read(self.h, _ptr(mean), _ptr(spp), _ptr(err), _ptr(act)), "ptx_adaptive_read")
        return dict(mean=mean, samples=spp, tile_error=err, tile_active=act != 0)

    def device_frame_ptr(self):
        return self.lib.ptx_adaptive_device_frame(self.h)

    def render(self, tracer, moments, batch=16, max_iterations=1 << 20, params=None, first_iteration=1, **kw):
        """render `batch` iterations -> add -> select, until no tile is active or max_iterations have been rendered; resolves at the end.
        Returns the list of the rounds' statuses; the last one's tiles_active is 0 unless the cap ended the run.  The handle, `moments`
        and the tracer's image are taken as they are: start from reset ones for a new frame."""
        p = params if params is not None else default_adaptive_params(**kw)
        rounds, done = [], 0
        while done < max_iterations:
            k = min(int(batch), max_iterations - done)
            tracer.render(first_iteration + done, k)
            done += k
            self.add(moments, tracer, k)
            rounds.append(self.select(moments, tracer, params=p))
            if rounds[-1]["tiles_active"] == 0:
                break
        self.resolve(tracer)
        return rounds


class DisplayParams(C.Structure):
    """ptx_display_params: meter, exposure, tone curve, transfer and quantiser of the display transform (include/mi355x_pathtracer.h;
    defaults from ptx_default_display_params)."""
    _fields_ = [("meter", C.c_int), ("exposure", C.c_float), ("key", C.c_float), ("adapt", C.c_float), ("tone", C.c_int),
                ("white", C.c_float), ("transfer", C.c_int), ("quantize", C.c_int), ("dither", C.c_int), ("keep_float", C.c_int)]


class DisplayStatus(C.Structure):
    """ptx_display_status (include/mi355x_pathtracer.h)."""
    _fields_ = [("metered", C.c_float), ("applied", C.c_float), ("log2_mean", C.c_float), ("blocks_used", C.c_int),
                ("blocks_total", C.c_int), ("frames", C.c_int64)]


METER_MANUAL, METER_BLOCKS = 0, 1
TONE_CLAMP, TONE_REINHARD, TONE_ACES = 0, 1, 2
TRANSFER_LINEAR, TRANSFER_SRGB = 0, 1
DISPLAY_IMAGE, DISPLAY_DENOISED = 0, 1
_DISPLAY_NAMES = dict(meter=dict(manual=METER_MANUAL, blocks=METER_BLOCKS), tone=dict(clamp=TONE_CLAMP, reinhard=TONE_REINHARD, aces=TONE_ACES),
                      transfer=dict(linear=TRANSFER_LINEAR, srgb=TRANSFER_SRGB))
_DISPLAY_SOURCES = dict(image=DISPLAY_IMAGE, denoised=DISPLAY_DENOISED)


def default_display_params(**kw):
    """ptx_default_display_params with keyword overrides (meter, exposure, key, adapt, tone, white, transfer, quantize, dither,
    keep_float); meter, tone and transfer take the PTX_* numbers or their names ("manual" / "blocks", "clamp" / "reinhard" / "aces",
    "linear" / "srgb")."""
    kw = {k: _DISPLAY_NAMES[k][v] if k in _DISPLAY_NAMES and isinstance(v, str) else v for k, v in kw.items()}
    return _default_params(DisplayParams, "ptx_default_display_params", ("meter", "tone", "transfer", "quantize", "dither", "keep_float"), **kw)


def debug_display_blocks(width, height):
    """ptx_debug_display_blocks: (row_begin, col_begin) of the meter's block grid, HK + 1 and WK + 1 int32 (empty when there is no block)"""
    hk, wk = C.c_int(), C.c_int()
    rows, cols = np.zeros((int(height) + 8) // 16 + 1, np.int32), np.zeros((int(width) + 8) // 16 + 1, np.int32)
    _check(load_library().ptx_debug_display_blocks(int(width), int(height), C.byref(hk), C.byref(wk), _ptr(rows), _ptr(cols)),
           "ptx_debug_display_blocks")
    if hk.value == 0:
        return rows[:0], cols[:0]
    return rows[:hk.value + 1], cols[:wk.value + 1]


class Display(_Owned):
    """The display transform on one device (opaque ptx_display): automatic exposure from block luminances, tone curve, sRGB transfer,
    8-bit codes.  tracer(T, spp) maps a tracer's frame, device(ptr, samples) any W*H*3 float frame on the device, host(rgb) a numpy
    frame; params are ptx_display_params' fields as keywords.  The adapted exposure lives in the handle: reset() forgets it."""

    _destroy = "ptx_display_destroy"

    def __init__(self, width, height, device=0):
        self.lib = load_library()
        h = vp()
        _check(self.lib.ptx_display_create(int(device), int(width), int(height), C.byref(h)), "ptx_display_create")
        self.h = h
        self.device_ordinal, self.width, self.height = int(device), int(width), int(height)

    def reset(self):
        """forget the adapted exposure: the next metered frame's applied exposure is its metered one"""
        _check(self.lib.ptx_display_reset(self.h), "ptx_display_reset")

    def tracer(self, tracer, spp, source="image", pbo=None, **params):
        """the tracer's accumulation buffer over spp (source "image") or its last denoised frame (source "denoised"), enqueued on the
        tracer's stream; pbo: a device pointer to W*H uchar4, None = the handle's own buffer (read())"""
        p = default_display_params(**params)
        src = _DISPLAY_SOURCES[source] if isinstance(source, str) else int(source)
        _check(self.lib.ptx_display_tracer(self.h, tracer.h, src, int(spp), C.byref(p), vp(pbo) if pbo else None), "ptx_display_tracer")

    def device(self, ptr, samples, stream=0, pbo=None, **params):
        """a W*H*3 float frame at device pointer `ptr`, divided by `samples`, enqueued on `stream` (a hipStream_t as an integer)"""
        p = default_display_params(**params)
        _check(self.lib.ptx_display_device(self.h, vp(ptr), float(samples), C.byref(p), vp(pbo) if pbo else None, vp(stream) if stream else None),
               "ptx_display_device")

    def host(self, rgb, samples=1, **params):
        """a host frame (H, W, 3) or (W*H, 3); returns the codes (H, W, 4) uint8"""
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.size != self.width * self.height * 3:
            raise ValueError("Display.host: the frame has %d floats, the handle's size needs %d" % (rgb.size, self.width * self.height * 3))
        p = default_display_params(**params)
        out = np.zeros((self.height, self.width, 4), np.uint8)
        _check(self.lib.ptx_display_host(self.h, _ptr(rgb), float(samples), C.byref(p), _ptr(out)), "ptx_display_host")
        return out

    def read(self, float_frame=False):
        """the last result's codes (H, W, 4) uint8; with float_frame=True (the last call had keep_float=1) a pair (z (H, W, 3) float32, codes)"""
        out = np.zeros((self.height, self.width, 4), np.uint8)
        if not float_frame:
            _check(self.lib.ptx_display_read(self.h, None, _ptr(out)), "ptx_display_read")
            return out
        z = np.zeros((self.height, self.width, 3), np.float32)
        _check(self.lib.ptx_display_read(self.h, _ptr(z), _ptr(out)), "ptx_display_read")
        return z, out

    def read_float(self):
        """z (H, W, 3) float32 of the last call (it had keep_float=1), wherever that call left its codes"""
        z = np.zeros((self.height, self.width, 3), np.float32)
        _check(self.lib.ptx_display_read(self.h, _ptr(z), None), "ptx_display_read")
        return z

    def blocks(self):
        """(HK, WK) float32: the block luminances of the last metered frame"""
        hk, wk = (self.height + 8) // 16, (self.width + 8) // 16
        out = np.zeros((hk, wk) if hk and wk else (0, 0), np.float32)
        scratch = out if out.size else np.zeros(1, np.float32)
        _check(self.lib.ptx_display_read_blocks(self.h, _ptr(scratch)), "ptx_display_read_blocks")
        return out

    def status(self):
        """ptx_display_get_status as a dict"""
        out = DisplayStatus()
        _check(self.lib.ptx_display_get_status(self.h, C.byref(out)), "ptx_display_get_status")
        return {k: getattr(out, k) for k, _ in DisplayStatus._fields_}


METRICS_NONE, METRICS_SRGB, METRICS_HDR, METRICS_SNORM = 0, 1, 2, 3
METRICS_VALID_SSIM, METRICS_VALID_MSSSIM, METRICS_VALID_GRAD = 1, 2, 4
METRICS_SCALES, METRICS_TAPS = 5, 11
_METRICS_TRANSFORMS = dict(none=METRICS_NONE, srgb=METRICS_SRGB, hdr=METRICS_HDR, snorm=METRICS_SNORM)


class MetricsParams(C.Structure):
    """ptx_metrics_params (include/mi355x_pathtracer.h, "image metrics"; defaults from ptx_default_metrics_params)."""
    _fields_ = [("transform", C.c_int), ("exposure", C.c_float), ("threshold", C.c_float), ("samples_a", C.c_float), ("samples_b", C.c_float), ("pointwise_only", C.c_int)]


class MetricsResult(C.Structure):
    """ptx_metrics_result: a sized struct, struct_size set by the caller."""
    _fields_ = [("struct_size", C.c_size_t), ("mse", C.c_double), ("psnr", C.c_double), ("l1", C.c_double), ("mape", C.c_double),
                ("smape", C.c_double), ("grad", C.c_double), ("l1_msssim", C.c_double), ("ssim", C.c_double), ("msssim", C.c_double),
                ("ssim_c", C.c_double * 3), ("msssim_c", C.c_double * 3), ("mcs", (C.c_double * 3) * METRICS_SCALES), ("max_error", C.c_double),
                ("num_errors", C.c_uint64), ("nonfinite_a", C.c_uint64), ("nonfinite_b", C.c_uint64), ("exposure", C.c_float), ("valid", C.c_int)]


class MetricsPlan(C.Structure):
    """ptx_metrics_plan: scale sizes, window taps and buffer sizes of a W x H handle."""
    _fields_ = [("ssim_valid", C.c_int), ("msssim_valid", C.c_int), ("scales", C.c_int), ("w", C.c_int * METRICS_SCALES), ("h", C.c_int * METRICS_SCALES),
                ("tile_w", C.c_int), ("tile_h", C.c_int), ("blocks", C.c_int * METRICS_SCALES), ("prep_blocks", C.c_int), ("grad_blocks", C.c_int),
                ("level_offset", C.c_size_t * METRICS_SCALES), ("pyramid_floats", C.c_size_t), ("partial_doubles", C.c_size_t),
                ("map_floats", C.c_size_t), ("taps", C.c_float * METRICS_TAPS), ("weights", C.c_float * METRICS_SCALES)]


def default_metrics_params(**kw):
    """ptx_default_metrics_params with keyword overrides (transform, exposure, threshold, samples_a, samples_b, pointwise_only); transform takes the
    PTX_METRICS_* numbers or "none" / "srgb" / "hdr" / "snorm"; exposure None = NaN = metered on b."""
    kw = {k: v for k, v in kw.items() if v is not None}
    if isinstance(kw.get("transform"), str):
        kw["transform"] = _METRICS_TRANSFORMS[kw["transform"]]
    return _default_params(MetricsParams, "ptx_default_metrics_params", ("transform", "pointwise_only"), **kw)


def _struct_value(v):
    if isinstance(v, C.Array):
        return np.array([_struct_value(x) for x in v])
    return v


def _metrics_dict(r):
    return {k: _struct_value(getattr(r, k)) for k, _ in MetricsResult._fields_ if k != "struct_size"}


def debug_metrics_plan(width, height):
    """ptx_debug_metrics_plan as a dict (arrays as numpy arrays).  No device needed."""
    out = MetricsPlan()
    _check(load_library().ptx_debug_metrics_plan(int(width), int(height), C.byref(out)), "ptx_debug_metrics_plan")
    return {k: _struct_value(getattr(out, k)) for k, _ in MetricsPlan._fields_}


def debug_metrics_problem(width, height, a, b, **params):
    """ptx_debug_metrics_problem: raises PathTracerError with what a compare call would refuse of these images (NNImage, or arrays for
    nn_image_of; None: no image) and params for a width x height frame.  No device needed."""
    p = default_metrics_params(**params)
    imgs = [None if x is None else C.byref(x if isinstance(x, NNImage) else nn_image_of(x)) for x in (a, b)]
    _check(load_library().ptx_debug_metrics_problem(int(width), int(height), imgs[0], imgs[1], C.byref(p)), "ptx_debug_metrics_problem")


class Metrics(_Owned):
    """Image metrics on one device (opaque ptx_metrics): MSE, PSNR, L1, MAPE, SMAPE, gradient, compareImage's count and maximum, SSIM and
    MS-SSIM of a test image `a` against a reference image `b` of one W x H, in one call that returns a dict of ptx_metrics_result's
    fields.  host(a, b) takes numpy views (or NNImage descriptors of host memory), device(a, b) NNImage descriptors of device memory,
    Tracer.compare(metrics, reference, spp) a tracer's frame."""

    _destroy = "ptx_metrics_destroy"

    def __init__(self, width, height, device=0):
        self.lib = load_library()
        h = vp()
        _check(self.lib.ptx_metrics_create(int(device), int(width), int(height), C.byref(h)), "ptx_metrics_create")
        self.h = h
        self.device_ordinal, self.width, self.height = int(device), int(width), int(height)

    def _image(self, x):
        if isinstance(x, NNImage):
            return x
        x = np.asarray(x)
        if x.ndim == 2:
            x = x.reshape(self.height, self.width, -1)
        return nn_image_of(x)

    def host(self, a, b, transform="none", exposure=None, threshold=None, samples_a=1, samples_b=1, want_map=False, pointwise_only=0):
        """a, b: float32 / float16 views of shape (H, W, >= 3) with any positive strides ((W*H, 3) is reshaped).  want_map: the dict
        also holds "map", the full-resolution SSIM map (H - 10, W - 10) float32, the mean over channels."""
        p = default_metrics_params(transform=transform, exposure=exposure, threshold=threshold, samples_a=samples_a, samples_b=samples_b,
                                   pointwise_only=int(pointwise_only))
        ia, ib = self._image(a), self._image(b)
        out = MetricsResult(struct_size=C.sizeof(MetricsResult))
        smap = np.zeros((max(self.height - 10, 0), max(self.width - 10, 0)), np.float32) if want_map else None
        _check(self.lib.ptx_metrics_compare_host(self.h, C.byref(ia), C.byref(ib), C.byref(p), C.byref(out), _ptr(smap) if want_map else None),
               "ptx_metrics_compare_host")
        d = _metrics_dict(out)
        if want_map:
            d["map"] = smap
        return d

    def device(self, a, b, transform="none", exposure=None, threshold=None, samples_a=1, samples_b=1, map_ptr=None, stream=0, pointwise_only=0):
        """a, b: NNImage descriptors of device memory (nn_image_of(ptr, format=..)); map_ptr: a device pointer to (H - 10)(W - 10) floats
        or None; compared on `stream` (a hipStream_t as an integer); waits for the result."""
        p = default_metrics_params(transform=transform, exposure=exposure, threshold=threshold, samples_a=samples_a, samples_b=samples_b,
                                   pointwise_only=int(pointwise_only))
        out = MetricsResult(struct_size=C.sizeof(MetricsResult))
        _check(self.lib.ptx_metrics_compare_device(self.h, C.byref(a), C.byref(b), C.byref(p), C.byref(out), vp(map_ptr) if map_ptr else None,
                                                   vp(stream) if stream else None), "ptx_metrics_compare_device")
        return _metrics_dict(out)


NN_LAYERS = 16


class NNParams(C.Structure):
    """ptx_nn_params: the network denoiser's transfer mode and input scale (include/mi355x_pathtracer.h; defaults from
    ptx_default_nn_params: hdr 0, srgb 0, input_scale NaN = automatic)."""
    _fields_ = [("hdr", C.c_int), ("srgb", C.c_int), ("input_scale", C.c_float)]


class NNInfo(C.Structure):
    """ptx_nn_info (include/mi355x_pathtracer.h)."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("padded_width", C.c_int), ("padded_height", C.c_int), ("input_channels", C.c_int),
                ("layers", C.c_int), ("cin", C.c_int * NN_LAYERS), ("cout", C.c_int * NN_LAYERS), ("name", (C.c_char * 16) * NN_LAYERS),
                ("scratch_bytes", C.c_uint64), ("macs", C.c_uint64)]


class NNTile(C.Structure):
    """ptx_nn_tile: the window a tile reads and the rectangle it keeps, in frame coordinates"""
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("out_x", C.c_int), ("out_y", C.c_int), ("out_w", C.c_int), ("out_h", C.c_int)]


class NNTiling(C.Structure):
    """ptx_nn_tiling (include/mi355x_pathtracer.h, "Tiles")"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("tile_width", C.c_int), ("tile_height", C.c_int), ("tiles_x", C.c_int),
                ("tiles_y", C.c_int), ("max_memory_mb", C.c_int), ("scratch_bytes", C.c_uint64), ("macs", C.c_uint64)]


def _nn_tiling_dict(call, what, tiles=True):
    """call(tiling, tiles, cap) -> rc, twice: the plan, then its tiles as dicts in execution order"""
    t = NNTiling()
    _check(call(C.byref(t), None, 0), what)
    out = {k: getattr(t, k) for k, _ in NNTiling._fields_}
    if tiles:
        n = t.tiles_x * t.tiles_y
        arr = (NNTile * n)()
        _check(call(C.byref(t), arr, n), what)
        rows = np.frombuffer(arr, np.int32).reshape(n, len(NNTile._fields_)).copy()
        out["tiles"] = rows if tiles == "array" else [dict(zip((k for k, _ in NNTile._fields_), (int(v) for v in r))) for r in rows]
    return out


def default_nn_params(**kw):
    """ptx_default_nn_params with keyword overrides (hdr, srgb, input_scale)."""
    return _default_params(NNParams, "ptx_default_nn_params", ("hdr", "srgb"), **kw)


def _nn_info_dict(info):
    layers = [(info.name[k].value.decode(), info.cin[k], info.cout[k]) for k in range(info.layers)]
    return dict(width=info.width, height=info.height, padded_width=info.padded_width, padded_height=info.padded_height,
                input_channels=info.input_channels, layers=layers, scratch_bytes=info.scratch_bytes, macs=info.macs)


def _blob_buffer(tza):
    blob = bytes(tza)
    return blob, C.cast(C.c_char_p(blob), vp)


def debug_tza_list(tza):
    """ptx_debug_tza_list: the table of a TZA weight blob (bytes) as a list of (name, dims, layout, type, offset); no device needed.
    A blob the reader refuses raises PathTracerError."""
    L = load_library()
    blob, ptr = _blob_buffer(tza)
    need = C.c_size_t(0)
    _check(L.ptx_debug_tza_list(ptr, len(blob), None, 0, C.byref(need)), "ptx_debug_tza_list")
    buf = C.create_string_buffer(need.value)
    _check(L.ptx_debug_tza_list(ptr, len(blob), buf, need.value, C.byref(need)), "ptx_debug_tza_list")
    out = []
    for line in buf.value.decode().splitlines():
        f = line.split(" ")
        nd = int(f[1])
        out.append((f[0], tuple(int(v) for v in f[2:2 + nd]), f[2 + nd], f[3 + nd], int(f[4 + nd])))
    return out


def debug_nn_plan(tza):
    """ptx_debug_nn_plan: the network plan of a TZA weight blob (input channels, per-layer channel table) as a dict; no device needed.
    A blob that is no such network raises PathTracerError naming the tensor."""
    blob, ptr = _blob_buffer(tza)
    info = NNInfo()
    _check(load_library().ptx_debug_nn_plan(ptr, len(blob), C.byref(info)), "ptx_debug_nn_plan")
    return _nn_info_dict(info)


def debug_nn_tiling(tza, width, height, max_memory_mb=0, tiles=True):
    """ptx_debug_nn_tiling: the tile plan NN(width, height, tza, max_memory_mb=...) would run by, as a dict (ptx_nn_tiling's fields, and
    `tiles`: ptx_nn_tile's fields per tile in execution order; tiles="array": as an (n, 8) int32 array, x y w h out_x out_y out_w out_h;
    tiles=False: left out); no device needed."""
    blob, ptr = _blob_buffer(tza)
    L = load_library()
    return _nn_tiling_dict(lambda t, a, n: L.ptx_debug_nn_tiling(ptr, len(blob), int(width), int(height), int(max_memory_mb), t, a, n),
                           "ptx_debug_nn_tiling", tiles)


NN_FORMAT_FLOAT3, NN_FORMAT_HALF3 = 1, 2
NN_ROLES = {"color": 0, "albedo": 1, "normal": 2}


class NNImage(C.Structure):
    """ptx_nn_image (include/mi355x_pathtracer.h, "images"): ptr, format, and in bytes the offset of pixel (0, 0), the pixel stride
    (0: packed, 12 / 6) and the row stride (0: width * pixel stride).  `keep` holds the array a descriptor was made from."""
    _fields_ = [("ptr", vp), ("format", C.c_int), ("byte_offset", C.c_size_t), ("pixel_stride", C.c_size_t), ("row_stride", C.c_size_t)]
    keep = None


def nn_image_of(array_or_ptr, format=None, byte_offset=0, pixel_stride=0, row_stride=0):
    """An NNImage of a numpy float32 / float16 array view of shape (H, W, >= 3) -- the pointer, offset and strides are the view's own,
    which may be a slice of a float4 / half4 buffer or of padded rows -- or of a raw pointer (an integer; `format` NN_FORMAT_FLOAT3 or
    NN_FORMAT_HALF3, the offset and strides in bytes as given)."""
    if isinstance(array_or_ptr, np.ndarray):
        a = array_or_ptr
        if a.dtype not in (np.float32, np.float16) or a.ndim != 3 or a.shape[2] < 3:
            raise PathTracerError("nn_image_of: an image is a float32 or float16 array of shape (H, W, >= 3)")
        if a.strides[2] != a.itemsize or a.strides[0] <= 0 or a.strides[1] <= 0:
            raise PathTracerError("nn_image_of: a pixel's channels must be consecutive and the strides positive")
        img = NNImage(vp(a.ctypes.data), NN_FORMAT_FLOAT3 if a.dtype == np.float32 else NN_FORMAT_HALF3, 0, a.strides[1], a.strides[0])
        img.keep = a
        return img
    if format not in (NN_FORMAT_FLOAT3, NN_FORMAT_HALF3):
        raise PathTracerError("nn_image_of: a pointer needs format=NN_FORMAT_FLOAT3 or NN_FORMAT_HALF3")
    return NNImage(vp(int(array_or_ptr)), int(format), int(byte_offset), int(pixel_stride), int(row_stride))


def debug_nn_image_problem(width, height, image, is_output=False):
    """ptx_debug_nn_image_problem: raises PathTracerError with what a call would refuse of this image (an NNImage, or an array for
    nn_image_of) for a width x height frame; returns None when there is nothing.  No device needed."""
    img = image if isinstance(image, NNImage) else nn_image_of(image)
    _check(load_library().ptx_debug_nn_image_problem(int(width), int(height), C.byref(img), int(bool(is_output))), "ptx_debug_nn_image_problem")


class NN(_Owned):
    """The network denoiser on one device (opaque ptx_nn): Open Image Denoise's RT filter run from the caller's TZA weights (`tza`:
    bytes, or a path) for one W x H.  host(rgb, albedo, normal) denoises a numpy frame, device(...) a frame on the device,
    Tracer.denoise_nn(nn, spp) a tracer's; params are ptx_nn_params' fields as keywords.  max_memory_mb None: the frame is one tile
    (ptx_nn_create, at most 7680 x 4320); a number: ptx_nn_create_tiled, overlapping tiles whose scratch fits that many MiB (0: no
    limit but the tile cap), frames up to 16384 x 16384, the same bits as one tile."""

    _destroy = "ptx_nn_destroy"

    def __init__(self, width, height, tza, device=0, max_memory_mb=None):
        self.lib = load_library()
        h = vp()
        size = (int(device), int(width), int(height))
        if isinstance(tza, (str, os.PathLike)):
            if max_memory_mb is None:
                _check(self.lib.ptx_nn_create_from_file(*size, os.fsencode(tza), C.byref(h)), "ptx_nn_create_from_file")
            else:
                _check(self.lib.ptx_nn_create_from_file_tiled(*size, os.fsencode(tza), int(max_memory_mb), C.byref(h)), "ptx_nn_create_from_file_tiled")
        else:
            blob, ptr = _blob_buffer(tza)
            if max_memory_mb is None:
                _check(self.lib.ptx_nn_create(*size, ptr, len(blob), C.byref(h)), "ptx_nn_create")
            else:
                _check(self.lib.ptx_nn_create_tiled(*size, ptr, len(blob), int(max_memory_mb), C.byref(h)), "ptx_nn_create_tiled")
        self.h = h
        self.device_ordinal, self.width, self.height = int(device), int(width), int(height)

    def tiling(self, tiles=True):
        """ptx_nn_get_tiling as a dict: ptx_nn_tiling's fields and `tiles`, ptx_nn_tile's fields per tile in execution order"""
        return _nn_tiling_dict(lambda t, a, n: self.lib.ptx_nn_get_tiling(self.h, t, a, n), "ptx_nn_get_tiling", tiles)

    def info(self):
        """ptx_nn_get_info as a dict: sizes, input_channels, layers = [(name, cin, cout)], scratch_bytes, macs"""
        info = NNInfo()
        _check(self.lib.ptx_nn_get_info(self.h, C.byref(info)), "ptx_nn_get_info")
        return _nn_info_dict(info)

    def device(self, rgb_ptr, out_ptr, samples=1, albedo_ptr=None, normal_ptr=None, stream=0, **params):
        """W*H*3 float frames at device pointers, enqueued on `stream` (a hipStream_t as an integer)"""
        p = default_nn_params(**params)
        opt = lambda a: vp(a) if a else None
        _check(self.lib.ptx_nn_denoise_device(self.h, vp(rgb_ptr), float(samples), opt(albedo_ptr), opt(normal_ptr), C.byref(p), vp(out_ptr),
                                              opt(stream)), "ptx_nn_denoise_device")

    def host(self, rgb, albedo=None, normal=None, samples=1, **params):
        """host frames (H, W, 3); returns the denoised (H, W, 3) float32"""
        n = self.width * self.height * 3
        frames = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (rgb, albedo, normal)]
        for a in frames:
            if a is not None and a.size != n:
                raise ValueError("NN.host: a frame has %d floats, the handle's size needs %d" % (a.size, n))
        p = default_nn_params(**params)
        out = np.zeros((self.height, self.width, 3), np.float32)
        _check(self.lib.ptx_nn_denoise_host(self.h, _ptr(frames[0]), float(samples), _opt_ptr(frames[1]), _opt_ptr(frames[2]), C.byref(p), _ptr(out)),
               "ptx_nn_denoise_host")
        return out

    def _images(self, color, output, albedo, normal, role):
        if role not in NN_ROLES:
            raise PathTracerError("NN: role must be one of %s" % ", ".join(map(repr, NN_ROLES)))
        descs = [a if a is None or isinstance(a, NNImage) else nn_image_of(a) for a in (color, albedo, normal, output)]
        return descs, [None if d is None else C.byref(d) for d in descs]

    def images_device(self, color, output, albedo=None, normal=None, samples=1, role="color", stream=0, **params):
        """ptx_nn_denoise_images_device: images on the device as NNImage descriptors (nn_image_of(ptr, format=..)), enqueued on `stream`
        (a hipStream_t as an integer).  role "albedo" / "normal": a 3-input network's image is that guide, as the prefilter takes it."""
        p = default_nn_params(**params)
        _, refs = self._images(color, output, albedo, normal, role)
        _check(self.lib.ptx_nn_denoise_images_device(self.h, refs[0], refs[1], refs[2], refs[3], float(samples), NN_ROLES[role], C.byref(p),
                                                     vp(stream) if stream else None), "ptx_nn_denoise_images_device")

    def images_host(self, color, output, albedo=None, normal=None, samples=1, role="color", **params):
        """ptx_nn_denoise_images_host: numpy float32 / float16 views of shape (H, W, >= 3) with any positive strides (or NNImage
        descriptors of host memory); writes the three channels of every pixel of `output` in place and nothing else.  `output` may be,
        or overlap, an input."""
        p = default_nn_params(**params)
        if isinstance(output, np.ndarray) and not output.flags.writeable:
            raise PathTracerError("NN.images_host: the output array is not writeable")
        keep, refs = self._images(color, output, albedo, normal, role)
        _check(self.lib.ptx_nn_denoise_images_host(self.h, refs[0], refs[1], refs[2], refs[3], float(samples), NN_ROLES[role], C.byref(p)),
               "ptx_nn_denoise_images_host")
        del keep

    def _lightmap(self, color, output):
        descs = [a if isinstance(a, NNImage) else nn_image_of(a) for a in (color, output)]
        return descs, [C.byref(d) for d in descs]

    def lightmap_device(self, color, output, directional=False, input_scale=float("nan"), stream=0):
        """ptx_nn_denoise_lightmap_device: OIDN's RTLightmap filter on a 3-input network, images on the device as NNImage descriptors
        (nn_image_of(ptr, format=..)), enqueued on `stream`.  directional False: the HDR lightmap (input_scale NaN: metered); True: the
        directional one (NaN: 1)."""
        _, refs = self._lightmap(color, output)
        _check(self.lib.ptx_nn_denoise_lightmap_device(self.h, refs[0], refs[1], int(directional), float(input_scale), vp(stream) if stream else None),
               "ptx_nn_denoise_lightmap_device")

    def lightmap_host(self, color, output, directional=False, input_scale=float("nan")):
        """ptx_nn_denoise_lightmap_host: numpy float32 / float16 views of shape (H, W, >= 3), as images_host takes them; writes the
        three channels of every pixel of `output` and nothing else.  `output` may be, or overlap, `color`."""
        if isinstance(output, np.ndarray) and not output.flags.writeable:
            raise PathTracerError("NN.lightmap_host: the output array is not writeable")
        keep, refs = self._lightmap(color, output)
        _check(self.lib.ptx_nn_denoise_lightmap_host(self.h, refs[0], refs[1], int(directional), float(input_scale)), "ptx_nn_denoise_lightmap_host")
        del keep

    def set_progress(self, monitor):
        """ptx_nn_set_progress: `monitor(n)` hears 0, then the finished share of the work after every stage of every tile, last exactly
        1; a falsy return value cancels the call, which raises Cancelled.  None: no monitor.  With a monitor every denoise on the
        handle returns only after it has completed."""
        if monitor is None:
            self._progress = None
            _check(self.lib.ptx_nn_set_progress(self.h, NN_PROGRESS_FN(), None), "ptx_nn_set_progress")
            return

        def call(_user, n):
            return 1 if monitor(n) else 0

        fn = NN_PROGRESS_FN(call)
        _check(self.lib.ptx_nn_set_progress(self.h, fn, None), "ptx_nn_set_progress")
        self._progress = fn                      # kept alive while the handle may call it

    def scale(self):
        """the scale the last denoise's input kernel used (the metered exposure in hdr mode with an automatic scale)"""
        s = C.c_float()
        _check(self.lib.ptx_nn_read_scale(self.h, C.byref(s)), "ptx_nn_read_scale")
        return np.float32(s.value)


def nn_denoise_buffers(tza, rgb, albedo=None, normal=None, samples=1, device=0, max_memory_mb=None, **params):
    """The network denoiser alone on host arrays of one (H, W, 3) frame: a handle for the frame's size from `tza` (bytes or a path;
    max_memory_mb as NN's), one NN.host call.  Returns the denoised (H, W, 3) float32.  Needs a HIP device: there is no CPU path."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise PathTracerError("nn_denoise_buffers: rgb must be (H, W, 3)")
    with NN(rgb.shape[1], rgb.shape[0], tza, device=device, max_memory_mb=max_memory_mb) as nn:
        return nn.host(rgb, albedo, normal, samples=samples, **params)


def kat_nn_conv(src0, weights, bias, src1=None, upsample=False, relu=True, pool=False, f32=False, device=0):
    """ptx_kat_nn_conv: one convolution layer by the production kernel.  src0 (h0, w0, cin0) float16, (h0, w0) = the output's (h, w) or
    half of it when upsample; src1 (h, w, cin1) float16 or None; weights (cout, cin0 + cin1, 3, 3) float32; bias (cout) float32.
    Returns float16 (h, w, cout), (h / 2, w / 2, cout) when pool, or float32 (h, w, 4) when f32."""
    src0 = np.ascontiguousarray(src0, np.float16)
    h, w = (2 * src0.shape[0], 2 * src0.shape[1]) if upsample else src0.shape[:2]
    src1 = None if src1 is None else np.ascontiguousarray(src1, np.float16)
    weights, bias = np.ascontiguousarray(weights, np.float32), np.ascontiguousarray(bias, np.float32)
    cout = weights.shape[0]
    cin1 = 0 if src1 is None else src1.shape[2]
    if weights.shape != (cout, src0.shape[2] + cin1, 3, 3) or bias.shape != (cout,) or (src1 is not None and src1.shape[:2] != (h, w)):
        raise ValueError("kat_nn_conv: shapes do not fit")
    out16 = np.zeros((h // 2, w // 2, cout) if pool else (h, w, cout), np.float16)
    out32 = np.zeros((h, w, 4), np.float32) if f32 else None
    _check(load_library().ptx_kat_nn_conv(int(device), w, h, src0.shape[2], _ptr(src0), int(bool(upsample)), cin1, _opt_ptr(src1), cout,
                                          _ptr(weights), _ptr(bias), int(bool(relu)), int(bool(pool)), None if f32 else _ptr(out16),
                                          _opt_ptr(out32)), "ptx_kat_nn_conv")
    return out32 if f32 else out16


def kat_nn_transfer(rgb, albedo=None, normal=None, hdr=0, srgb=0, scale=1.0, inverse=False, device=0):
    """ptx_kat_nn_transfer on (H, W, 3) float32 frames: forward = the input kernel's nine fp32 values per pixel before the rounding to
    fp16, (H, W, 9); inverse = the output kernel on a network output, (H, W, 3)."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    as3 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).reshape(h, w, 3)
    alb, nrm = as3(albedo), as3(normal)
    out = np.zeros((h, w, 3 if inverse else 9), np.float32)
    _check(load_library().ptx_kat_nn_transfer(int(device), w, h, _ptr(rgb), _opt_ptr(alb), _opt_ptr(nrm), int(hdr), int(srgb), float(scale),
                                              int(bool(inverse)), _ptr(out)), "ptx_kat_nn_transfer")
    return out


NN_AUX_ALBEDO, NN_AUX_NORMAL = 1, 2


class NNPrefilterParams(C.Structure):
    """ptx_nn_prefilter_params (include/mi355x_pathtracer.h; defaults from ptx_default_nn_prefilter_params: srgb 0, input_scale NaN = 1).
    There is no hdr field: a prefilter in hdr mode is refused."""
    _fields_ = [("srgb", C.c_int), ("input_scale", C.c_float)]


class NNPrefilterInfo(C.Structure):
    """ptx_nn_prefilter_info (include/mi355x_pathtracer.h)."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("has_albedo", C.c_int), ("has_normal", C.c_int),
                ("albedo", NNInfo), ("normal", NNInfo), ("scratch_bytes", C.c_uint64), ("runs", C.c_uint64)]


def default_nn_prefilter_params(**kw):
    """ptx_default_nn_prefilter_params with keyword overrides (srgb, input_scale); any other keyword, hdr among them, is refused."""
    for k in kw:
        if k not in ("srgb", "input_scale"):
            raise PathTracerError("ptx_nn_prefilter_params has no field %r (a prefilter takes srgb and input_scale; hdr is refused)" % k)
    return _default_params(NNPrefilterParams, "ptx_default_nn_prefilter_params", ("srgb",), **kw)


def _opt_blob(tza):
    """(keep-alive, pointer, length) of an optional blob"""
    if tza is None:
        return None, None, 0
    blob, ptr = _blob_buffer(tza)
    return blob, ptr, len(blob)


def debug_nn_prefilter_problem(albedo_tza=None, normal_tza=None, **params):
    """ptx_debug_nn_prefilter_problem: raises PathTracerError with what NNPrefilter(.., albedo_tza, normal_tza) or a run with these
    params (srgb, input_scale) would refuse without a device; returns None when there is nothing."""
    p = default_nn_prefilter_params(**params)
    a, b = _opt_blob(albedo_tza), _opt_blob(normal_tza)
    _check(load_library().ptx_debug_nn_prefilter_problem(a[1], a[2], b[1], b[2], C.byref(p)), "ptx_debug_nn_prefilter_problem")


class NNPrefilter(_Owned):
    """The prefilter of the network denoiser's guides on one device (opaque ptx_nn_prefilter; OIDN's cleanAux): a 3-input network for
    the albedo image, one for the normal image, or both (`albedo_tza`, `normal_tza`: bytes or paths, both of one kind), for one W x H.
    host(albedo, normal) cleans numpy images; Tracer.denoise_nn(nn, spp, prefilter=pf) cleans a tracer's guides, once per G-buffer.
    max_memory_mb None: each network runs the frame as one tile; a number: as NN's."""

    _destroy = "ptx_nn_prefilter_destroy"

    def __init__(self, width, height, albedo_tza=None, normal_tza=None, device=0, max_memory_mb=None):
        self.lib = load_library()
        h = vp()
        size = (int(device), int(width), int(height))
        mb = -1 if max_memory_mb is None else int(max_memory_mb)
        given = [t for t in (albedo_tza, normal_tza) if t is not None]
        if given and all(isinstance(t, (str, os.PathLike)) for t in given):
            enc = lambda t: None if t is None else os.fsencode(t)
            _check(self.lib.ptx_nn_prefilter_create_from_files(*size, enc(albedo_tza), enc(normal_tza), mb, C.byref(h)), "ptx_nn_prefilter_create_from_files")
        else:
            a, b = _opt_blob(albedo_tza), _opt_blob(normal_tza)
            _check(self.lib.ptx_nn_prefilter_create(*size, a[1], a[2], b[1], b[2], mb, C.byref(h)), "ptx_nn_prefilter_create")
        self.h = h
        self.device_ordinal, self.width, self.height = int(device), int(width), int(height)
        self.has_albedo, self.has_normal = albedo_tza is not None, normal_tza is not None

    def info(self):
        """ptx_nn_prefilter_get_info as a dict: width, height, albedo / normal (NN.info()'s dict, or None), scratch_bytes, runs"""
        info = NNPrefilterInfo()
        _check(self.lib.ptx_nn_prefilter_get_info(self.h, C.byref(info)), "ptx_nn_prefilter_get_info")
        return dict(width=info.width, height=info.height, albedo=_nn_info_dict(info.albedo) if info.has_albedo else None,
                    normal=_nn_info_dict(info.normal) if info.has_normal else None, scratch_bytes=info.scratch_bytes, runs=info.runs)

    def _result(self, pair):
        return pair[0] if not self.has_normal else pair[1] if not self.has_albedo else pair

    def host(self, albedo=None, normal=None, **params):
        """host images (H, W, 3), each given exactly when the handle has a network for it; returns the clean (H, W, 3) float32 image,
        or the pair (albedo, normal) of a handle with both networks"""
        n = self.width * self.height * 3
        frames = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (albedo, normal)]
        for a in frames:
            if a is not None and a.size != n:
                raise ValueError("NNPrefilter.host: an image has %d floats, the handle's size needs %d" % (a.size, n))
        p = default_nn_prefilter_params(**params)
        outs = [np.zeros((self.height, self.width, 3), np.float32) if has else None for has in (self.has_albedo, self.has_normal)]
        _check(self.lib.ptx_nn_prefilter_run_host(self.h, _opt_ptr(frames[0]), _opt_ptr(frames[1]), C.byref(p), _opt_ptr(outs[0]), _opt_ptr(outs[1])),
               "ptx_nn_prefilter_run_host")
        return self._result(outs)

    def device(self, albedo_ptr=None, normal_ptr=None, albedo_stride=3, normal_stride=3, stream=0, **params):
        """images at device pointers with a stride of 3 or 4 floats per pixel, enqueued on `stream`; read() has the result"""
        p = default_nn_prefilter_params(**params)
        opt = lambda a: vp(a) if a else None
        _check(self.lib.ptx_nn_prefilter_run_device(self.h, opt(albedo_ptr), int(albedo_stride), opt(normal_ptr), int(normal_stride), C.byref(p),
                                                    opt(stream)), "ptx_nn_prefilter_run_device")

    def read(self):
        """the clean images of the last run, as host() returns them"""
        outs = [np.zeros((self.height, self.width, 3), np.float32) if has else None for has in (self.has_albedo, self.has_normal)]
        _check(self.lib.ptx_nn_prefilter_read(self.h, _opt_ptr(outs[0]), _opt_ptr(outs[1])), "ptx_nn_prefilter_read")
        return self._result(outs)

    def invalidate(self):
        """the next Tracer.denoise_nn(.., prefilter=self) runs the networks again"""
        _check(self.lib.ptx_nn_prefilter_invalidate(self.h), "ptx_nn_prefilter_invalidate")


def kat_nn_transfer_aux(image, kind, srgb=0, scale=1.0, inverse=False, device=0):
    """ptx_kat_nn_transfer_aux on an (H, W, 3) float32 image: the prefilter's input kernel (the three fp32 values per pixel before the
    rounding to fp16) or, inverse, its output kernel on a network output; kind NN_AUX_ALBEDO or NN_AUX_NORMAL."""
    image = np.ascontiguousarray(image, np.float32)
    h, w = image.shape[:2]
    out = np.zeros((h, w, 3), np.float32)
    _check(load_library().ptx_kat_nn_transfer_aux(int(device), w, h, int(kind), _ptr(image), int(srgb), float(scale), int(bool(inverse)), _ptr(out)),
           "ptx_kat_nn_transfer_aux")
    return out


def _frame_arrays(fn, rgb, albedo, normal, position, hit):
    """one (H, W) frame as the ptx_denoise_buffers* entry points take it: h, w, rgb (H, W, 3) float32, albedo (or None) / normal /
    position (H*W, 3) float32, hit (H*W) uint8"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise PathTracerError("%s: rgb must be (H, W, 3)" % fn)
    h, w = rgb.shape[:2]
    as3 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).reshape(h * w, 3)
    return h, w, rgb, as3(albedo), as3(normal), as3(position), np.ascontiguousarray(np.asarray(hit).reshape(h * w) != 0, np.uint8)


def _opt_ptr(a):
    return None if a is None else _ptr(a)


def denoise_buffers(rgb, albedo, normal, position, hit, device=0, **params):
    """The a-trous filter alone (ptx_denoise_buffers) on host arrays of one (H, W) frame: rgb = mean radiance, albedo / normal / position
    (..., 3), hit (...) bool.  Returns the filtered mean radiance as (H, W, 3) float32 when rgb is (H, W, 3), else rgb's shape.  Needs a
    HIP device: there is no CPU path."""
    L = load_library()
    h, w, rgb, alb, nrm, pos, hit = _frame_arrays("denoise_buffers", rgb, albedo, normal, position, hit)
    out = np.zeros((h, w, 3), np.float32)
    p = default_denoise_params(**params)
    _check(L.ptx_denoise_buffers(int(device), w, h, _ptr(rgb), _opt_ptr(alb), _ptr(nrm), _ptr(pos), _ptr(hit), C.byref(p), _ptr(out)),
           "ptx_denoise_buffers")
    return out


def denoise_buffers_variance(rgb, albedo, normal, position, hit, ids=None, variance=None, device=0, **params):
    """The variance-guided filter alone (ptx_denoise_buffers_variance) on host arrays of one (H, W) frame, as denoise_buffers: ids
    (H, W, 2) int32 of (material, geom) or None (the spatial estimate then skips its id test), variance (H, W) = v0 or None (the
    spatial estimate).  Returns the filtered mean radiance (H, W, 3) and the last pass's variance (H, W), float32."""
    L = load_library()
    h, w, rgb, alb, nrm, pos, hit = _frame_arrays("denoise_buffers_variance", rgb, albedo, normal, position, hit)
    ids = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(h * w, 2)
    var = None if variance is None else np.ascontiguousarray(variance, np.float32).reshape(h * w)
    out, vout = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    dp, _, vpar = _split_variance_params("denoise_buffers_variance", params)
    _check(L.ptx_denoise_buffers_variance(int(device), w, h, _ptr(rgb), _opt_ptr(alb), _ptr(nrm), _ptr(pos), _ptr(hit), _opt_ptr(ids),
                                          _opt_ptr(var), C.byref(dp), C.byref(vpar), _ptr(out), _ptr(vout)), "ptx_denoise_buffers_variance")
    return out, vout


def _camera_struct(cam, w, h):
    """a Camera, or a mapping with position / view / right / up (3 each) and pl or pixelLength (2), as a Camera of resolution w x h"""
    if isinstance(cam, Camera):
        return cam
    c = Camera()
    c.resolution[0], c.resolution[1] = int(cam.get("W", w)), int(cam.get("H", h))
    for k in ("position", "view", "right", "up"):
        for j in range(3):
            getattr(c, k)[j] = float(cam[k][j])
    pl = cam["pl"] if "pl" in cam else cam["pixelLength"]
    c.pixelLength[0], c.pixelLength[1] = float(pl[0]), float(pl[1])
    return c


def reproject_buffers(rgb, albedo, normal, position, ids, hit, spec, hist=None, hist_camera=None, spp=1, variant=0, scatter=None,
                      batches=0, device=0, **params):
    """The temporal reprojection and mix alone (ptx_kat_reproject) on host arrays of one (H, W) frame, as denoise_buffers: rgb = the
    accumulation of spp samples, albedo / normal / position (H, W, 3), ids (H, W, 2) int32 of (material, geom), hit (H, W), spec = one
    flag per material.  hist_camera (a Camera, or a mapping with position, view, right, up, pl) and hist = dict(hit, normal, position, n,
    D, ids and, when the state carries one, V) are the committed history; hist_camera None = none.  variant 0 / 1 / 2 = the kernel of
    denoise_temporal / denoise_variance / denoise_temporal_measured; 2 takes scatter (H, W, 6) = (rr, gg, bb, rg, rb, gb) and batches.
    params: the temporal parameters.  Returns a dict of float32 arrays nh (H, W, 4), xn (H, W, 4), dd (H, W, 4), mix (H, W, 3),
    hn (H, W, 4) and ids (H, W, 2) int32: the new state's records, the mix and (h, n_h)."""
    L = load_library()
    h, w, rgb, alb, nrm, pos, hit = _frame_arrays("reproject_buffers", rgb, albedo, normal, position, hit)
    f3 = lambda a: np.ascontiguousarray(a, np.float32).reshape(h * w, 3)
    i2 = lambda a: np.ascontiguousarray(a, np.int32).reshape(h * w, 2)
    ids = None if ids is None else i2(ids)
    spec = np.ascontiguousarray(np.asarray(spec).reshape(-1) != 0, np.uint8)
    cam, hh = None, [None] * 7
    if hist_camera is not None:
        cam = _camera_struct(hist_camera, w, h)
        if hist is not None:
            hh = [np.ascontiguousarray(np.asarray(hist["hit"]).reshape(h * w) != 0, np.uint8), f3(hist["normal"]), f3(hist["position"]),
                  np.ascontiguousarray(hist["n"], np.float32).reshape(h * w), f3(hist["D"]),
                  None if hist.get("V") is None else np.ascontiguousarray(hist["V"], np.float32).reshape(h * w), i2(hist["ids"])]
    sc = None if scatter is None else np.ascontiguousarray(scatter, np.float32).reshape(h * w, 6)
    for k in params:
        if k not in _TEMPORAL_KEYS:
            raise TypeError("reproject_buffers: unknown parameter %r" % (k,))
    tp = default_temporal_params(**params)
    out = dict(nh=np.zeros((h, w, 4), np.float32), xn=np.zeros((h, w, 4), np.float32), dd=np.zeros((h, w, 4), np.float32),
               ids=np.zeros((h, w, 2), np.int32), mix=np.zeros((h, w, 3), np.float32), hn=np.zeros((h, w, 4), np.float32))
    _check(L.ptx_kat_reproject(int(device), w, h, int(variant), None if cam is None else C.byref(cam), C.byref(tp), int(spp), _ptr(rgb),
                               _opt_ptr(nrm), _opt_ptr(pos), _opt_ptr(alb), _opt_ptr(ids), _ptr(hit), _ptr(spec) if spec.size else None,
                               int(spec.size), *[_opt_ptr(a) for a in hh], _opt_ptr(sc), int(batches), _ptr(out["nh"]), _ptr(out["xn"]),
                               _ptr(out["dd"]), _ptr(out["ids"]), _ptr(out["mix"]), _ptr(out["hn"])), "ptx_kat_reproject")
    return out


def debug_tile_geoms(camera, boxes6, depth_of_field=False, tile=None):
    """CPU only: the per-tile geom masks of the camera-ray bounce (ptx_debug_tile_geoms) for a ctypes Camera, an (n, 6) array of world
    boxes (lo xyz, hi xyz) and an optional row-tile split (rows, rank, world).  Returns a uint32 array, one word per tile of 256 owned
    pixels."""
    L = load_library()
    b = np.ascontiguousarray(boxes6, np.float32).reshape(-1, 6)
    rows, rank, world = tile if tile else (0, 0, 1)
    cap = (camera.resolution[0] * camera.resolution[1] + 255) // 256 + 1
    out = np.zeros(cap, np.uint32)
    n = L.ptx_debug_tile_geoms(C.byref(camera), len(b), _ptr(b), int(bool(depth_of_field)), rows, rank, world, _ptr(out), cap)
    if n < 0:
        raise PathTracerError("ptx_debug_tile_geoms: bad argument")
    return out[:n]


def debug_cull_boxes(boxes6):
    """CPU only: the device's table of the candidate pre-test (ptx_debug_cull_boxes) for an (n, 6) array of corner boxes: (n, 8) float32,
    centre xyz, 0, half extent xyz, 0."""
    L = load_library()
    b = np.ascontiguousarray(boxes6, np.float32).reshape(-1, 6)
    out = np.zeros((len(b), 8), np.float32)
    if L.ptx_debug_cull_boxes(len(b), _ptr(b), _ptr(out)) < 0:
        raise PathTracerError("ptx_debug_cull_boxes: bad argument")
    return out


def debug_light_bits(materials, geom_material):
    """CPU only: ptx_create's light_bits (ptx_debug_light_bits) for an (n, 11) float32 array of materials (struct Material: colour 3,
    exponent, specular colour 3, reflective, refractive, ior, emittance) and the geoms' material indices: bit g = geom g's material emits."""
    L = load_library()
    m = np.ascontiguousarray(materials, np.float32).reshape(-1, 11)
    gm = np.ascontiguousarray(geom_material, np.int32).reshape(-1)
    out = np.zeros(1, np.uint32)
    if L.ptx_debug_light_bits(len(m), _ptr(m), len(gm), _ptr(gm), _ptr(out)) < 0:
        raise PathTracerError("ptx_debug_light_bits: bad argument")
    return int(out[0])


def debug_cull_objboxes(geom_ints, geom_mats, faces, margin=1.0, no_bvh=0):
    """CPU only: the object-space boxes of a scene's small meshes (ptx_debug_cull_objboxes) for geoms given as Scene.dump() gives them:
    geom_ints (n, 3) = type, material, faces; geom_mats (n, 48) = transform, inverseTransform, invTranspose; faces = a list of (k, 15)
    arrays.  Returns ((n, 16) float32 table as the device reads it, objcull_bits).  margin 0: the boxes without their derived margins;
    no_bvh as the option of that name (every mesh counts as small)."""
    L = load_library()
    gi = np.ascontiguousarray(geom_ints, np.int32).reshape(-1, 3)
    gm = np.ascontiguousarray(geom_mats, np.float32).reshape(-1, 48)
    keep = [np.ascontiguousarray(f, np.float32).reshape(-1, 15) for f in faces]
    geoms = (Geom * max(len(gi), 1))()
    for g in range(len(gi)):
        geoms[g].type, geoms[g].materialid = int(gi[g][0]), int(gi[g][1])
        for name, k in (("transform", 0), ("inverseTransform", 16), ("invTranspose", 32)):
            getattr(geoms[g], name)[:] = gm[g][k:k + 16].tolist()
        geoms[g].faceSize = len(keep[g])
        geoms[g].faces = keep[g].ctypes.data_as(C.POINTER(C.c_float)) if len(keep[g]) else None
    out = np.zeros((len(gi), 16), np.float32)
    bits = np.zeros(1, np.uint32)
    if L.ptx_debug_cull_objboxes(len(gi), geoms, int(no_bvh), float(margin), _ptr(out), _ptr(bits)) < 0:
        raise PathTracerError("ptx_debug_cull_objboxes: bad argument")
    return out, int(bits[0])


def debug_cube_tangents(geom_ints, geom_mats):
    """CPU only: the tangent frames of the cubes' tabulated face normals (ptx_debug_cube_tangents) for geoms given as Scene.dump() gives
    them: geom_ints (n, 3) = type, material, faces; geom_mats (n, 48) = transform, inverseTransform, invTranspose.  Returns an (n, 6, 6)
    float32 array: per geom and side (axis * 2 + (sign > 0)) perp1 xyz, perp2 xyz; zeros for a geom that is not a cube."""
    L = load_library()
    gi = np.ascontiguousarray(geom_ints, np.int32).reshape(-1, 3)
    gm = np.ascontiguousarray(geom_mats, np.float32).reshape(-1, 48)
    geoms = (Geom * max(len(gi), 1))()
    for g in range(len(gi)):
        geoms[g].type, geoms[g].materialid = int(gi[g][0]), int(gi[g][1])
        for name, k in (("transform", 0), ("inverseTransform", 16), ("invTranspose", 32)):
            getattr(geoms[g], name)[:] = gm[g][k:k + 16].tolist()
    out = np.zeros((len(gi), 6, 6), np.float32)
    if L.ptx_debug_cube_tangents(len(gi), geoms, _ptr(out)) < 0:
        raise PathTracerError("ptx_debug_cube_tangents: bad argument")
    return out


WALK_NAMES = ("loop", "skip", "ordered", "wide", "wide_refill")      # PTX_WALK_* of include/mi355x_pathtracer.h


def build_library(force=False):
    """Compiles the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(PKG_DIR, "csrc")])
    return LIB_PATH


_lib = None


class Orbit(C.Structure):
    """ptx_orbit: phi, theta, zoom and the original lookAt of src/main.cpp:18-20"""
    _fields_ = [("phi", C.c_float), ("theta", C.c_float), ("zoom", C.c_float), ("og_look_at", C.c_float * 3)]


def _share_hip_runtime_with_torch():
    """PyTorch's ROCm wheels bundle their own HIP runtime under torch/lib with the same sonames as /opt/rocm's.
    Whichever copy a process loads first serves both libraries, and torch does not find its GPUs through the system
    copy -- so a process that may import torch later (the multi-GPU driver does) loads torch's copy first.
    Without torch installed this does nothing and the library uses /opt/rocm's runtime."""
    import importlib.util
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    hip = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(hip):
        try:
            C.CDLL(hip, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """Loads the native library; raises loudly when it has not been built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    _share_hip_runtime_with_torch()
    if not os.path.exists(LIB_PATH):
        raise PathTracerError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(or make -C mygpuraytracer_amd/csrc). There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    i, f = C.c_int, C.c_float
    # the structs below are allocated HERE and filled by the library: a library of another ABI revision (an older variant build
    # loaded for A/B timing) would overrun them or leave their tail unset -- refused, whatever it is
    if not hasattr(L, "ptx_abi_version"):
        raise PathTracerError("%s predates ptx_abi_version (ABI < %d): rebuild it from this tree" % (LIB_PATH, ABI_VERSION))
    L.ptx_abi_version.restype = i
    L.ptx_sizeof_options.restype = L.ptx_sizeof_stats.restype = C.c_size_t
    if L.ptx_abi_version() != ABI_VERSION or L.ptx_sizeof_options() != C.sizeof(Options) or L.ptx_sizeof_stats() != C.sizeof(Stats):
        raise PathTracerError("%s has ABI %d (options %d B, stats %d B), this module expects %d (%d B, %d B): rebuild the library" % (
            LIB_PATH, L.ptx_abi_version(), L.ptx_sizeof_options(), L.ptx_sizeof_stats(), ABI_VERSION, C.sizeof(Options), C.sizeof(Stats)))
    L.ptx_sizeof_denoise_params.restype = C.c_size_t
    if L.ptx_sizeof_denoise_params() != C.sizeof(DenoiseParams):
        raise PathTracerError("%s has a ptx_denoise_params of %d B, this module expects %d B: rebuild the library" % (
            LIB_PATH, L.ptx_sizeof_denoise_params(), C.sizeof(DenoiseParams)))
    L.ptx_sizeof_variance_params.restype = C.c_size_t
    if L.ptx_sizeof_variance_params() != C.sizeof(VarianceParams):
        raise PathTracerError("%s has a ptx_variance_params of %d B, this module expects %d B: rebuild the library" % (
            LIB_PATH, L.ptx_sizeof_variance_params(), C.sizeof(VarianceParams)))
    L.ptx_sizeof_temporal_params.restype = C.c_size_t
    if L.ptx_sizeof_temporal_params() != C.sizeof(TemporalParams):
        raise PathTracerError("%s has a ptx_temporal_params of %d B, this module expects %d B: rebuild the library" % (
            LIB_PATH, L.ptx_sizeof_temporal_params(), C.sizeof(TemporalParams)))
    L.ptx_last_error.restype = C.c_char_p
    L.ptx_device_count.restype = i
    L.ptx_default_options.argtypes = [C.POINTER(Options)]
    L.ptx_scene_load.restype, L.ptx_scene_load.argtypes = i, [C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.ptx_scene_free.argtypes = [vp]
    L.ptx_scene_num_geoms.restype, L.ptx_scene_num_geoms.argtypes = i, [vp]
    L.ptx_scene_num_materials.restype, L.ptx_scene_num_materials.argtypes = i, [vp]
    L.ptx_scene_geoms.restype, L.ptx_scene_geoms.argtypes = C.POINTER(Geom), [vp]
    L.ptx_scene_materials.restype, L.ptx_scene_materials.argtypes = C.POINTER(Material), [vp]
    L.ptx_scene_camera.restype, L.ptx_scene_camera.argtypes = C.POINTER(Camera), [vp]
    L.ptx_scene_iterations.restype, L.ptx_scene_iterations.argtypes = i, [vp]
    L.ptx_scene_trace_depth.restype, L.ptx_scene_trace_depth.argtypes = i, [vp]
    L.ptx_scene_set_trace_depth.argtypes = [vp, i]
    L.ptx_scene_set_resolution.argtypes = [vp, i, i]
    L.ptx_scene_image_name.restype, L.ptx_scene_image_name.argtypes = C.c_char_p, [vp]
    L.ptx_scene_apply_runcuda_camera.argtypes = [vp]
    L.ptx_orbit_init.argtypes = [vp, C.POINTER(Orbit)]
    L.ptx_orbit_left_drag.argtypes = [C.POINTER(Orbit), C.c_double, C.c_double, i, i]
    L.ptx_orbit_right_drag.argtypes = [C.POINTER(Orbit), C.c_double, i]
    L.ptx_orbit_middle_drag.argtypes = [vp, C.c_double, C.c_double]
    L.ptx_orbit_recenter.argtypes = [vp, C.POINTER(Orbit)]
    L.ptx_orbit_apply.argtypes = [vp, C.POINTER(Orbit)]
    L.ptx_create.restype = i
    L.ptx_create.argtypes = [i, C.POINTER(Geom), i, C.POINTER(Material), C.POINTER(Camera), i, C.POINTER(Options), vp,
                             vp, C.POINTER(vp)]
    L.ptx_create_from_scene.restype = i
    L.ptx_create_from_scene.argtypes = [vp, C.POINTER(Options), vp, vp, C.POINTER(vp)]
    L.ptx_destroy.argtypes = [vp]
    L.ptx_set_camera.restype, L.ptx_set_camera.argtypes = i, [vp, C.POINTER(Camera), i]
    L.ptx_reset_image.restype, L.ptx_reset_image.argtypes = i, [vp]
    L.ptx_iterate.restype, L.ptx_iterate.argtypes = i, [vp, i]
    L.ptx_set_render_ahead.restype, L.ptx_set_render_ahead.argtypes = i, [vp, i]
    L.ptx_render.restype, L.ptx_render.argtypes = i, [vp, i, i]
    L.ptx_render_strided.restype, L.ptx_render_strided.argtypes = i, [vp, i, i, i]
    L.ptx_write_image.restype, L.ptx_write_image.argtypes = i, [vp, vp]
    L.ptx_synchronize.restype, L.ptx_synchronize.argtypes = i, [vp]
    L.ptx_read_image.restype, L.ptx_read_image.argtypes = i, [vp, vp]
    L.ptx_device_image.restype, L.ptx_device_image.argtypes = vp, [vp]
    L.ptx_read_albedo.restype, L.ptx_read_albedo.argtypes = i, [vp, vp]
    L.ptx_write_denoised_pbo.restype, L.ptx_write_denoised_pbo.argtypes = i, [vp, vp, vp]
    L.ptx_write_denoised_pbo_device.restype, L.ptx_write_denoised_pbo_device.argtypes = i, [vp, vp, vp]
    L.ptx_write_pbo.restype, L.ptx_write_pbo.argtypes = i, [vp, i, vp]
    L.ptx_write_pbo_device.restype, L.ptx_write_pbo_device.argtypes = i, [vp, i, vp]
    L.ptx_last_loop_ms.restype, L.ptx_last_loop_ms.argtypes = C.c_double, [vp]
    L.ptx_default_denoise_params.argtypes = [C.POINTER(DenoiseParams)]
    L.ptx_denoise.restype, L.ptx_denoise.argtypes = i, [vp, C.POINTER(DenoiseParams), i]
    L.ptx_read_denoised.restype, L.ptx_read_denoised.argtypes = i, [vp, vp]
    L.ptx_device_denoised.restype, L.ptx_device_denoised.argtypes = vp, [vp]
    L.ptx_write_denoised_pbo_from_device.restype, L.ptx_write_denoised_pbo_from_device.argtypes = i, [vp, vp]
    L.ptx_read_gbuffer.restype, L.ptx_read_gbuffer.argtypes = i, [vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "ptx_set_guide_samples"):     # (absent from the older builds the A/B scripts load through PTX_AB_LIBRARY)
        L.ptx_set_guide_samples.restype, L.ptx_set_guide_samples.argtypes = i, [vp, i, i]
        L.ptx_get_guide_samples.restype, L.ptx_get_guide_samples.argtypes = i, [vp, C.POINTER(i), C.POINTER(i)]
        L.ptx_read_guide_coverage.restype, L.ptx_read_guide_coverage.argtypes = i, [vp, vp]
    if hasattr(L, "ptx_set_guide_bounces"):
        L.ptx_set_guide_bounces.restype, L.ptx_set_guide_bounces.argtypes = i, [vp, i]
        L.ptx_get_guide_bounces.restype, L.ptx_get_guide_bounces.argtypes = i, [vp, C.POINTER(i)]
    L.ptx_denoise_buffers.restype = i
    L.ptx_denoise_buffers.argtypes = [i, i, i, vp, vp, vp, vp, vp, C.POINTER(DenoiseParams), vp]
    L.ptx_default_temporal_params.argtypes = [C.POINTER(TemporalParams)]
    L.ptx_temporal_create.restype, L.ptx_temporal_create.argtypes = i, [i, i, i, C.POINTER(vp)]
    L.ptx_temporal_destroy.restype, L.ptx_temporal_destroy.argtypes = None, [vp]
    L.ptx_temporal_reset.restype, L.ptx_temporal_reset.argtypes = i, [vp]
    L.ptx_denoise_temporal.restype = i
    L.ptx_denoise_temporal.argtypes = [vp, vp, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), i]
    L.ptx_temporal_read.restype, L.ptx_temporal_read.argtypes = i, [vp, vp, vp, vp]
    L.ptx_default_variance_params.argtypes = [C.POINTER(VarianceParams)]
    L.ptx_denoise_variance.restype = i
    L.ptx_denoise_variance.argtypes = [vp, vp, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.POINTER(VarianceParams), i]
    L.ptx_read_variance.restype, L.ptx_read_variance.argtypes = i, [vp, vp, vp]
    L.ptx_denoise_buffers_variance.restype = i
    L.ptx_denoise_buffers_variance.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, vp, C.POINTER(DenoiseParams), C.POINTER(VarianceParams), vp, vp]
    L.ptx_sizeof_moments_params.restype = L.ptx_sizeof_moments_summary.restype = C.c_size_t
    if L.ptx_sizeof_moments_params() != C.sizeof(MomentsParams) or L.ptx_sizeof_moments_summary() != C.sizeof(MomentsSummary):
        raise PathTracerError("ptx_moments_params / ptx_moments_summary layout mismatch")
    L.ptx_default_moments_params.argtypes = [C.POINTER(MomentsParams)]
    L.ptx_moments_create.restype, L.ptx_moments_create.argtypes = i, [i, i, i, C.POINTER(vp)]
    L.ptx_moments_destroy.restype, L.ptx_moments_destroy.argtypes = None, [vp]
    L.ptx_moments_reset.restype, L.ptx_moments_reset.argtypes = i, [vp]
    L.ptx_moments_add.restype, L.ptx_moments_add.argtypes = i, [vp, vp, C.c_int64]
    L.ptx_moments_add_host.restype, L.ptx_moments_add_host.argtypes = i, [vp, vp, C.c_int64]
    L.ptx_moments_read.restype, L.ptx_moments_read.argtypes = i, [vp, vp, vp, vp, C.POINTER(C.c_int64)]
    L.ptx_moments_summarize.restype, L.ptx_moments_summarize.argtypes = i, [vp, C.POINTER(MomentsParams), C.POINTER(MomentsSummary)]
    L.ptx_denoise_measured.restype = i
    L.ptx_denoise_measured.argtypes = [vp, vp, C.POINTER(DenoiseParams), C.POINTER(VarianceParams), i, i]
    L.ptx_denoise_temporal_measured.restype = i
    L.ptx_denoise_temporal_measured.argtypes = [vp, vp, vp, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.POINTER(VarianceParams), i, i]
    L.ptx_moments_add_host_tiled.restype, L.ptx_moments_add_host_tiled.argtypes = i, [vp, vp, vp, i]
    L.ptx_moments_read_samples.restype, L.ptx_moments_read_samples.argtypes = i, [vp, vp]
    L.ptx_tile_pixels.restype, L.ptx_tile_pixels.argtypes = i, []
    L.ptx_num_tiles.restype, L.ptx_num_tiles.argtypes = i, [vp]
    L.ptx_set_active_tiles.restype, L.ptx_set_active_tiles.argtypes = i, [vp, vp, i]
    L.ptx_clear_active_tiles.restype, L.ptx_clear_active_tiles.argtypes = i, [vp]
    L.ptx_sizeof_adaptive_params.restype = L.ptx_sizeof_adaptive_status.restype = C.c_size_t
    if L.ptx_sizeof_adaptive_params() != C.sizeof(AdaptiveParams) or L.ptx_sizeof_adaptive_status() != C.sizeof(AdaptiveStatus):
        raise PathTracerError("%s has adaptive structs of %d and %d B, this module expects %d and %d B: rebuild the library" % (
            LIB_PATH, L.ptx_sizeof_adaptive_params(), L.ptx_sizeof_adaptive_status(), C.sizeof(AdaptiveParams), C.sizeof(AdaptiveStatus)))
    L.ptx_default_adaptive_params.argtypes = [C.POINTER(AdaptiveParams)]
    L.ptx_adaptive_create.restype, L.ptx_adaptive_create.argtypes = i, [i, i, i, C.POINTER(vp)]
    L.ptx_adaptive_destroy.restype, L.ptx_adaptive_destroy.argtypes = None, [vp]
    L.ptx_adaptive_reset.restype, L.ptx_adaptive_reset.argtypes = i, [vp]
    L.ptx_adaptive_num_tiles.restype, L.ptx_adaptive_num_tiles.argtypes = i, [vp]
    L.ptx_adaptive_add.restype, L.ptx_adaptive_add.argtypes = i, [vp, vp, vp, i]
    L.ptx_adaptive_select.restype = i
    L.ptx_adaptive_select.argtypes = [vp, vp, vp, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveStatus)]
    L.ptx_adaptive_resolve.restype, L.ptx_adaptive_resolve.argtypes = i, [vp, vp]
    L.ptx_adaptive_read.restype, L.ptx_adaptive_read.argtypes = i, [vp, vp, vp, vp, vp]
    L.ptx_adaptive_device_frame.restype, L.ptx_adaptive_device_frame.argtypes = vp, [vp]
    L.ptx_denoise_adaptive.restype = i
    L.ptx_denoise_adaptive.argtypes = [vp, vp, vp, C.POINTER(DenoiseParams), C.POINTER(VarianceParams), i]
    L.ptx_sizeof_display_params.restype = L.ptx_sizeof_display_status.restype = C.c_size_t
    if L.ptx_sizeof_display_params() != C.sizeof(DisplayParams) or L.ptx_sizeof_display_status() != C.sizeof(DisplayStatus):
        raise PathTracerError("%s has display structs of %d and %d B, this module expects %d and %d B: rebuild the library" % (
            LIB_PATH, L.ptx_sizeof_display_params(), L.ptx_sizeof_display_status(), C.sizeof(DisplayParams), C.sizeof(DisplayStatus)))
    L.ptx_default_display_params.argtypes = [C.POINTER(DisplayParams)]
    L.ptx_display_create.restype, L.ptx_display_create.argtypes = i, [i, i, i, C.POINTER(vp)]
    L.ptx_display_destroy.restype, L.ptx_display_destroy.argtypes = None, [vp]
    L.ptx_display_reset.restype, L.ptx_display_reset.argtypes = i, [vp]
    L.ptx_display_tracer.restype, L.ptx_display_tracer.argtypes = i, [vp, vp, i, i, C.POINTER(DisplayParams), vp]
    L.ptx_display_device.restype, L.ptx_display_device.argtypes = i, [vp, vp, f, C.POINTER(DisplayParams), vp, vp]
    L.ptx_display_host.restype, L.ptx_display_host.argtypes = i, [vp, vp, f, C.POINTER(DisplayParams), vp]
    L.ptx_display_read.restype, L.ptx_display_read.argtypes = i, [vp, vp, vp]
    L.ptx_display_read_blocks.restype, L.ptx_display_read_blocks.argtypes = i, [vp, vp]
    L.ptx_display_get_status.restype, L.ptx_display_get_status.argtypes = i, [vp, C.POINTER(DisplayStatus)]
    L.ptx_debug_display_blocks.restype, L.ptx_debug_display_blocks.argtypes = i, [i, i, C.POINTER(i), C.POINTER(i), vp, vp]
    # image metrics
    L.ptx_sizeof_metrics_params.restype = L.ptx_sizeof_metrics_result.restype = L.ptx_sizeof_metrics_plan.restype = C.c_size_t
    if (L.ptx_sizeof_metrics_params() != C.sizeof(MetricsParams) or L.ptx_sizeof_metrics_result() != C.sizeof(MetricsResult)
            or L.ptx_sizeof_metrics_plan() != C.sizeof(MetricsPlan)):
        raise PathTracerError("%s has metrics structs of %d, %d and %d B, this module expects %d, %d and %d B: rebuild the library" % (
            LIB_PATH, L.ptx_sizeof_metrics_params(), L.ptx_sizeof_metrics_result(), L.ptx_sizeof_metrics_plan(), C.sizeof(MetricsParams),
            C.sizeof(MetricsResult), C.sizeof(MetricsPlan)))
    L.ptx_default_metrics_params.argtypes = [C.POINTER(MetricsParams)]
    L.ptx_metrics_create.restype, L.ptx_metrics_create.argtypes = i, [i, i, i, C.POINTER(vp)]
    L.ptx_metrics_destroy.restype, L.ptx_metrics_destroy.argtypes = None, [vp]
    L.ptx_metrics_compare_device.restype = i
    L.ptx_metrics_compare_device.argtypes = [vp, C.POINTER(NNImage), C.POINTER(NNImage), C.POINTER(MetricsParams), C.POINTER(MetricsResult), vp, vp]
    L.ptx_metrics_compare_host.restype = i
    L.ptx_metrics_compare_host.argtypes = [vp, C.POINTER(NNImage), C.POINTER(NNImage), C.POINTER(MetricsParams), C.POINTER(MetricsResult), vp]
    L.ptx_metrics_tracer.restype = i
    L.ptx_metrics_tracer.argtypes = [vp, vp, i, i, C.POINTER(NNImage), C.POINTER(MetricsParams), C.POINTER(MetricsResult)]
    L.ptx_debug_metrics_plan.restype, L.ptx_debug_metrics_plan.argtypes = i, [i, i, C.POINTER(MetricsPlan)]
    L.ptx_debug_metrics_problem.restype = i
    L.ptx_debug_metrics_problem.argtypes = [i, i, C.POINTER(NNImage), C.POINTER(NNImage), C.POINTER(MetricsParams)]
    # network denoiser
    L.ptx_sizeof_nn_params.restype = L.ptx_sizeof_nn_info.restype = C.c_size_t
    if L.ptx_sizeof_nn_params() != C.sizeof(NNParams) or L.ptx_sizeof_nn_info() != C.sizeof(NNInfo):
        raise PathTracerError("%s has network denoiser structs of %d and %d B, this module expects %d and %d B: rebuild the library" % (
            LIB_PATH, L.ptx_sizeof_nn_params(), L.ptx_sizeof_nn_info(), C.sizeof(NNParams), C.sizeof(NNInfo)))
    L.ptx_default_nn_params.argtypes = [C.POINTER(NNParams)]
    L.ptx_nn_create.restype, L.ptx_nn_create.argtypes = i, [i, i, i, vp, C.c_size_t, C.POINTER(vp)]
    L.ptx_nn_create_from_file.restype, L.ptx_nn_create_from_file.argtypes = i, [i, i, i, C.c_char_p, C.POINTER(vp)]
    L.ptx_nn_destroy.restype, L.ptx_nn_destroy.argtypes = None, [vp]
    L.ptx_nn_get_info.restype, L.ptx_nn_get_info.argtypes = i, [vp, C.POINTER(NNInfo)]
    L.ptx_nn_denoise_device.restype, L.ptx_nn_denoise_device.argtypes = i, [vp, vp, f, vp, vp, C.POINTER(NNParams), vp, vp]
    L.ptx_nn_denoise_host.restype, L.ptx_nn_denoise_host.argtypes = i, [vp, vp, f, vp, vp, C.POINTER(NNParams), vp]
    L.ptx_nn_read_scale.restype, L.ptx_nn_read_scale.argtypes = i, [vp, C.POINTER(f)]
    L.ptx_denoise_nn.restype, L.ptx_denoise_nn.argtypes = i, [vp, vp, C.POINTER(NNParams), i]
    L.ptx_kat_nn_conv.restype, L.ptx_kat_nn_conv.argtypes = i, [i, i, i, i, vp, i, i, vp, i, vp, vp, i, i, vp, vp]
    L.ptx_kat_nn_transfer.restype, L.ptx_kat_nn_transfer.argtypes = i, [i, i, i, vp, vp, vp, i, i, f, i, vp]
    L.ptx_debug_tza_list.restype, L.ptx_debug_tza_list.argtypes = i, [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ptx_debug_nn_plan.restype, L.ptx_debug_nn_plan.argtypes = i, [vp, C.c_size_t, C.POINTER(NNInfo)]
    L.ptx_sizeof_nn_tile.restype = L.ptx_sizeof_nn_tiling.restype = C.c_size_t
    if L.ptx_sizeof_nn_tile() != C.sizeof(NNTile) or L.ptx_sizeof_nn_tiling() != C.sizeof(NNTiling):
        raise PathTracerError("%s has network tile structs of %d and %d B, this module expects %d and %d B: rebuild the library" % (
            LIB_PATH, L.ptx_sizeof_nn_tile(), L.ptx_sizeof_nn_tiling(), C.sizeof(NNTile), C.sizeof(NNTiling)))
    L.ptx_nn_create_tiled.restype, L.ptx_nn_create_tiled.argtypes = i, [i, i, i, vp, C.c_size_t, i, C.POINTER(vp)]
    L.ptx_nn_create_from_file_tiled.restype, L.ptx_nn_create_from_file_tiled.argtypes = i, [i, i, i, C.c_char_p, i, C.POINTER(vp)]
    L.ptx_nn_get_tiling.restype, L.ptx_nn_get_tiling.argtypes = i, [vp, C.POINTER(NNTiling), C.POINTER(NNTile), i]
    L.ptx_debug_nn_tiling.restype, L.ptx_debug_nn_tiling.argtypes = i, [vp, C.c_size_t, i, i, i, C.POINTER(NNTiling), C.POINTER(NNTile), i]
    L.ptx_sizeof_nn_prefilter_params.restype = L.ptx_sizeof_nn_prefilter_info.restype = C.c_size_t
    if L.ptx_sizeof_nn_prefilter_params() != C.sizeof(NNPrefilterParams) or L.ptx_sizeof_nn_prefilter_info() != C.sizeof(NNPrefilterInfo):
        raise PathTracerError("%s: ptx_nn_prefilter_params / _info are %d / %d bytes in the library, %d / %d here" % (
            LIB_PATH, L.ptx_sizeof_nn_prefilter_params(), L.ptx_sizeof_nn_prefilter_info(), C.sizeof(NNPrefilterParams), C.sizeof(NNPrefilterInfo)))
    pfp = C.POINTER(NNPrefilterParams)
    L.ptx_default_nn_prefilter_params.argtypes = [pfp]
    L.ptx_nn_prefilter_create.restype, L.ptx_nn_prefilter_create.argtypes = i, [i, i, i, vp, C.c_size_t, vp, C.c_size_t, i, C.POINTER(vp)]
    L.ptx_nn_prefilter_create_from_files.restype, L.ptx_nn_prefilter_create_from_files.argtypes = i, [i, i, i, C.c_char_p, C.c_char_p, i, C.POINTER(vp)]
    L.ptx_nn_prefilter_destroy.restype, L.ptx_nn_prefilter_destroy.argtypes = None, [vp]
    L.ptx_nn_prefilter_get_info.restype, L.ptx_nn_prefilter_get_info.argtypes = i, [vp, C.POINTER(NNPrefilterInfo)]
    L.ptx_nn_prefilter_run_device.restype, L.ptx_nn_prefilter_run_device.argtypes = i, [vp, vp, i, vp, i, pfp, vp]
    L.ptx_nn_prefilter_run_host.restype, L.ptx_nn_prefilter_run_host.argtypes = i, [vp, vp, vp, pfp, vp, vp]
    L.ptx_nn_prefilter_device_clean.restype, L.ptx_nn_prefilter_device_clean.argtypes = i, [vp, C.POINTER(vp), C.POINTER(vp)]
    L.ptx_nn_prefilter_read.restype, L.ptx_nn_prefilter_read.argtypes = i, [vp, vp, vp]
    L.ptx_nn_prefilter_invalidate.restype, L.ptx_nn_prefilter_invalidate.argtypes = i, [vp]
    L.ptx_denoise_nn_prefiltered.restype, L.ptx_denoise_nn_prefiltered.argtypes = i, [vp, vp, vp, C.POINTER(NNParams), pfp, i]
    L.ptx_kat_nn_transfer_aux.restype, L.ptx_kat_nn_transfer_aux.argtypes = i, [i, i, i, i, vp, i, f, i, vp]
    L.ptx_debug_nn_prefilter_problem.restype, L.ptx_debug_nn_prefilter_problem.argtypes = i, [vp, C.c_size_t, vp, C.c_size_t, pfp]
    L.ptx_sizeof_nn_image.restype = C.c_size_t
    if L.ptx_sizeof_nn_image() != C.sizeof(NNImage):
        raise PathTracerError("%s: ptx_nn_image is %d bytes in the library, %d here" % (LIB_PATH, L.ptx_sizeof_nn_image(), C.sizeof(NNImage)))
    imp = C.POINTER(NNImage)
    L.ptx_nn_denoise_images_device.restype, L.ptx_nn_denoise_images_device.argtypes = i, [vp, imp, imp, imp, imp, f, i, C.POINTER(NNParams), vp]
    L.ptx_nn_denoise_images_host.restype, L.ptx_nn_denoise_images_host.argtypes = i, [vp, imp, imp, imp, imp, f, i, C.POINTER(NNParams)]
    L.ptx_debug_nn_image_problem.restype, L.ptx_debug_nn_image_problem.argtypes = i, [i, i, imp, i]
    L.ptx_nn_denoise_lightmap_device.restype, L.ptx_nn_denoise_lightmap_device.argtypes = i, [vp, imp, imp, i, f, vp]
    L.ptx_nn_denoise_lightmap_host.restype, L.ptx_nn_denoise_lightmap_host.argtypes = i, [vp, imp, imp, i, f]
    L.ptx_debug_nn_lightmap_constants.restype, L.ptx_debug_nn_lightmap_constants.argtypes = None, [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.ptx_nn_set_progress.restype, L.ptx_nn_set_progress.argtypes = i, [vp, NN_PROGRESS_FN, vp]
    L.ptx_get_stats.restype, L.ptx_get_stats.argtypes = i, [vp, C.POINTER(Stats)]
    L.ptx_get_stats_sized.restype, L.ptx_get_stats_sized.argtypes = i, [vp, vp, C.c_size_t]
    L.ptx_owned_pixels.restype, L.ptx_owned_pixels.argtypes = i, [vp]
    L.ptx_stream.restype, L.ptx_stream.argtypes = vp, [vp]
    L.ptx_set_kernel_timing.restype, L.ptx_set_kernel_timing.argtypes = i, [vp, i]
    L.ptx_get_kernel_times.restype, L.ptx_get_kernel_times.argtypes = i, [vp, vp, vp]
    L.ptx_kat_geom_test.restype, L.ptx_kat_geom_test.argtypes = i, [vp, i, i, vp, vp]
    L.ptx_kat_compute_intersections.restype, L.ptx_kat_compute_intersections.argtypes = i, [vp, i, vp, vp]
    L.ptx_kat_obj_tri_test.restype, L.ptx_kat_obj_tri_test.argtypes = i, [vp, i, i, vp, vp]
    L.ptx_kat_jittered_hemisphere.restype, L.ptx_kat_jittered_hemisphere.argtypes = i, [vp, i, vp, vp, i, vp]
    L.ptx_kat_tile_intersect.restype, L.ptx_kat_tile_intersect.argtypes = i, [vp, i, vp, vp, i]
    L.ptx_kat_shade.restype, L.ptx_kat_shade.argtypes = i, [vp, i, i, vp, vp, vp]
    L.ptx_kat_generate.restype, L.ptx_kat_generate.argtypes = i, [vp, i, vp]
    L.ptx_kat_libm.restype, L.ptx_kat_libm.argtypes = i, [vp, i, vp, vp, vp, vp, vp, vp, vp]
    L.ptx_kat_reproject.restype = i
    L.ptx_kat_reproject.argtypes = [i, i, i, i, C.POINTER(Camera), C.POINTER(TemporalParams), i] + [vp] * 7 + [i] + [vp] * 8 + [i] + [vp] * 6
    if hasattr(L, "ptx_debug_tile_geoms"):
        L.ptx_debug_tile_geoms.restype, L.ptx_debug_tile_geoms.argtypes = i, [vp, i, vp, i, i, i, i, vp, i]
    if hasattr(L, "ptx_debug_cull_boxes"):
        L.ptx_debug_cull_boxes.restype, L.ptx_debug_cull_boxes.argtypes = i, [i, vp, vp]
    if hasattr(L, "ptx_debug_light_bits"):
        L.ptx_debug_light_bits.restype, L.ptx_debug_light_bits.argtypes = i, [i, vp, i, vp, vp]
    if hasattr(L, "ptx_debug_cull_objboxes"):
        L.ptx_debug_cull_objboxes.restype, L.ptx_debug_cull_objboxes.argtypes = i, [i, C.POINTER(Geom), i, C.c_float, vp, vp]
    if hasattr(L, "ptx_debug_cube_tangents"):
        L.ptx_debug_cube_tangents.restype, L.ptx_debug_cube_tangents.argtypes = i, [i, C.POINTER(Geom), vp]
    if hasattr(L, "ptx_debug_mesh_plan"):
        L.ptx_debug_mesh_plan.restype, L.ptx_debug_mesh_plan.argtypes = i, [vp, i, vp]
    if hasattr(L, "ptx_debug_index_plan"):      # (absent from the older builds the A/B scripts load through PTX_AB_LIBRARY)
        L.ptx_debug_index_plan.restype, L.ptx_debug_index_plan.argtypes = i, [vp, vp]
    if hasattr(L, "ptx_kat_fast_exact"):        # (absent from the older builds the A/B scripts load through PTX_AB_LIBRARY)
        L.ptx_kat_fast_exact.restype, L.ptx_kat_fast_exact.argtypes = i, [vp, vp]
    if hasattr(L, "ptx_kat_unit_rsqrt"):
        L.ptx_kat_unit_rsqrt.restype, L.ptx_kat_unit_rsqrt.argtypes = i, [vp, i, C.c_int64, vp]
    L.ptx_debug_set_capture.restype, L.ptx_debug_set_capture.argtypes = i, [vp, i]
    L.ptx_debug_read_stream.restype, L.ptx_debug_read_stream.argtypes = i, [vp, C.POINTER(i), vp, vp, vp, vp, i]
    # several devices behind one handle (csrc/pt_multi.cpp)
    L.ptx_multi_create.restype, L.ptx_multi_create.argtypes = i, [vp, C.POINTER(Options), C.POINTER(C.c_int), i, i, C.POINTER(vp)]
    L.ptx_multi_destroy.argtypes = [vp]
    L.ptx_multi_device_count.restype, L.ptx_multi_device_count.argtypes = i, [vp]
    L.ptx_multi_tracer.restype, L.ptx_multi_tracer.argtypes = vp, [vp, i]
    L.ptx_multi_set_camera.restype, L.ptx_multi_set_camera.argtypes = i, [vp, C.POINTER(Camera), i]
    for n in ("ptx_multi_reset_image", "ptx_multi_synchronize", "ptx_multi_assemble"):
        getattr(L, n).restype, getattr(L, n).argtypes = i, [vp]
    L.ptx_multi_iterate.restype, L.ptx_multi_iterate.argtypes = i, [vp, i]
    L.ptx_multi_set_render_ahead.restype, L.ptx_multi_set_render_ahead.argtypes = i, [vp, i]
    L.ptx_multi_render.restype, L.ptx_multi_render.argtypes = i, [vp, i, i]
    L.ptx_multi_device_image.restype, L.ptx_multi_device_image.argtypes = vp, [vp]
    L.ptx_multi_read_image.restype, L.ptx_multi_read_image.argtypes = i, [vp, vp]
    L.ptx_multi_read_albedo.restype, L.ptx_multi_read_albedo.argtypes = i, [vp, vp]
    L.ptx_multi_get_stats.restype, L.ptx_multi_get_stats.argtypes = i, [vp, C.POINTER(Stats)]
    L.ptx_pin_host_buffer.restype, L.ptx_pin_host_buffer.argtypes = i, [vp, C.c_size_t]
    L.ptx_unpin_host_buffer.restype, L.ptx_unpin_host_buffer.argtypes = i, [vp]
    # stream compaction
    L.sc_cpu_scan.argtypes = [i, vp, vp]
    for n in ("sc_cpu_compact_without_scan", "sc_cpu_compact_with_scan", "sc_efficient_compact", "sc_naive_scan",
              "sc_efficient_scan", "sc_thrust_scan"):
        getattr(L, n).restype, getattr(L, n).argtypes = i, [i, vp, vp]
    L.sc_scan_workspace_bytes.restype, L.sc_scan_workspace_bytes.argtypes = C.c_ulonglong, [i]
    L.sc_scan_device.restype, L.sc_scan_device.argtypes = i, [i, vp, vp, vp, vp]
    L.sc_compact_device.restype, L.sc_compact_device.argtypes = i, [i, vp, vp, vp, vp, vp]
    L.sc_map_to_boolean_device.restype, L.sc_map_to_boolean_device.argtypes = i, [i, vp, vp, vp]
    L.sc_scatter_device.restype, L.sc_scatter_device.argtypes = i, [i, vp, vp, vp, vp, vp]
    L.sc_records_tile_elements.restype, L.sc_records_tile_elements.argtypes = i, []
    L.sc_records_workspace_bytes.restype, L.sc_records_workspace_bytes.argtypes = C.c_ulonglong, [i, i]
    L.sc_sort_records_by_key_device.restype, L.sc_sort_records_by_key_device.argtypes = i, [i, i, i, vp, i, vp, vp, i, vp, vp, i, vp, vp, vp, vp]
    for n in ("sc_partition_records_device", "sc_compact_records_device"):
        getattr(L, n).restype, getattr(L, n).argtypes = i, [i, i, vp, vp, vp, i, vp, vp, vp]
    L.sc_sort_records_by_key.restype, L.sc_sort_records_by_key.argtypes = i, [i, i, i, vp, vp, vp, i, vp, vp, i, vp, vp]
    for n in ("sc_partition_records", "sc_compact_records"):
        getattr(L, n).restype, getattr(L, n).argtypes = i, [i, i, vp, vp, vp, vp]
    L.sc_radix_workspace_bytes.restype, L.sc_radix_workspace_bytes.argtypes = C.c_ulonglong, [i]
    L.sc_radix_map_key.restype, L.sc_radix_map_key.argtypes = C.c_uint, [i, i, C.c_uint]
    L.sc_radix_sort_records_device.restype, L.sc_radix_sort_records_device.argtypes = i, [i, i, i, i, i, vp, i, vp, vp, i, vp, vp, i, vp, vp, vp, vp]
    L.sc_radix_sort_records.restype, L.sc_radix_sort_records.argtypes = i, [i, i, i, i, i, vp, vp, vp, i, vp, vp, i, vp, vp]
    L.sc_last_gpu_ms.restype = f
    L.sc_last_cpu_ms.restype = f
    L.sc_ilog2.restype, L.sc_ilog2.argtypes = i, [i]
    L.sc_ilog2ceil.restype, L.sc_ilog2ceil.argtypes = i, [i]
    _lib = L
    return L


def _check(rc, what):
    if rc == PTX_ERR_CANCELLED:
        raise Cancelled("%s was cancelled (code %d): %s" % (what, rc, load_library().ptx_last_error().decode()))
    if rc != PTX_OK:
        raise PathTracerError("%s failed (code %d): %s" % (what, rc, load_library().ptx_last_error().decode()))


def _ptr(a):
    return a.ctypes.data_as(vp)


def default_options(**kw):
    o = Options()
    load_library().ptx_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


class Scene(_Owned):
    """A loaded scenes/*.txt (class Scene, src/scene.h)."""
    _destroy = "ptx_scene_free"

    def __init__(self, path, base_dir=None, res=None, depth=None):
        self.lib = load_library()
        h = vp()
        _check(self.lib.ptx_scene_load(os.fspath(path).encode(), base_dir.encode() if base_dir else None, C.byref(h)),
               "ptx_scene_load(%s)" % path)
        self.h = h
        if res is not None:
            self.set_resolution(*res)
        if depth is not None:
            self.set_trace_depth(depth)

    @property
    def num_geoms(self):
        return self.lib.ptx_scene_num_geoms(self.h)

    @property
    def num_materials(self):
        return self.lib.ptx_scene_num_materials(self.h)

    @property
    def camera(self):
        return self.lib.ptx_scene_camera(self.h).contents

    @property
    def resolution(self):
        c = self.camera
        return int(c.resolution[0]), int(c.resolution[1])

    @property
    def iterations(self):
        return self.lib.ptx_scene_iterations(self.h)

    @property
    def trace_depth(self):
        return self.lib.ptx_scene_trace_depth(self.h)

    @property
    def image_name(self):
        return self.lib.ptx_scene_image_name(self.h).decode()

    def set_trace_depth(self, d):
        self.lib.ptx_scene_set_trace_depth(self.h, d)

    def set_resolution(self, w, h):
        self.lib.ptx_scene_set_resolution(self.h, w, h)

    def apply_runcuda_camera(self):
        self.lib.ptx_scene_apply_runcuda_camera(self.h)

    # --- the interactive camera of src/main.cpp, driven by a script instead of a mouse ---------------------
    def orbit_init(self):
        """main.cpp:56-70 -> Orbit (phi, theta, zoom, original lookAt)"""
        o = Orbit()
        self.lib.ptx_orbit_init(self.h, C.byref(o))
        return o

    def orbit_events(self, orbit, events):
        """Applies mouse/key events in order, then runCuda's camera recompute (main.cpp:105-123).  events: tuples
        ("left", dx, dy) | ("right", dy) | ("middle", dx, dy) | ("space",) with deltas in window pixels, as the GLFW
        callbacks of main.cpp:166-212 see them.  Hand the result to a tracer with Tracer.set_camera + reset_image."""
        w, h = self.resolution
        for ev in events:
            kind = ev[0]
            if kind == "left":
                self.lib.ptx_orbit_left_drag(C.byref(orbit), float(ev[1]), float(ev[2]), w, h)
            elif kind == "right":
                self.lib.ptx_orbit_right_drag(C.byref(orbit), float(ev[1]), h)
            elif kind == "middle":
                self.lib.ptx_orbit_middle_drag(self.h, float(ev[1]), float(ev[2]))
            elif kind == "space":
                self.lib.ptx_orbit_recenter(self.h, C.byref(orbit))
            else:
                raise PathTracerError("unknown camera event %r" % (ev,))
            # main.cpp applies the recompute on the next frame, i.e. between any two events that set camchanged;
            # the middle drag reads cam.view / cam.right of the recomputed camera, so do the same here
            self.lib.ptx_orbit_apply(self.h, C.byref(orbit))
        return orbit

    def dump(self):
        """POD view of the scene as numpy arrays (same dict layout the CPU checkers use in tests/cpulibs.py)."""
        ng, nm = self.num_geoms, self.num_materials
        geoms = self.lib.ptx_scene_geoms(self.h)
        mats = self.lib.ptx_scene_materials(self.h)
        gints = np.zeros((ng, 3), np.int32)
        trs = np.zeros((ng, 9), np.float32)
        gm = np.zeros((ng, 48), np.float32)
        faces, textures = [], {}
        for i in range(ng):
            g = geoms[i]
            gints[i] = (g.type, g.materialid, g.faceSize)
            trs[i] = list(g.translation) + list(g.rotation) + list(g.scale)
            gm[i] = list(g.transform) + list(g.inverseTransform) + list(g.invTranspose)
            if g.faceSize:
                faces.append(np.ctypeslib.as_array(g.faces, shape=(g.faceSize, 15)).copy())
            else:
                faces.append(np.zeros((0, 15), np.float32))
            for which, t in enumerate((g.kd, g.ks, g.ke, g.bump)):      # checker order: kd, ks, ke, bump
                if t.channels:
                    textures[(i, which)] = np.ctypeslib.as_array(t.image, shape=(t.height, t.width, t.channels)).copy()
        m = np.zeros((nm, 11), np.float32)
        for i in range(nm):
            m[i] = np.frombuffer(bytes(mats[i]), np.float32)
        c = self.camera
        cf = np.array(list(c.position) + list(c.lookAt) + list(c.view) + list(c.up) + list(c.right) + list(c.fov)
                      + list(c.pixelLength), np.float32)
        ci = np.array([c.resolution[0], c.resolution[1], self.iterations, self.trace_depth], np.int32)
        return dict(geom_ints=gints, geom_trs=trs, geom_mats=gm, materials=m, faces=faces, cam_ints=ci, cam_floats=cf,
                    textures=textures)


class MultiTracer(_Owned):
    """The frame split into interleaved row blocks over several devices of one node, one process (opaque ptx_multi; the C/C++
    side of the tile split -- include/mi355x_pathtracer.h "N GPUs of one node").  `devices` may repeat an ordinal."""
    _destroy = "ptx_multi_destroy"

    def __init__(self, scene, devices, tile_rows=8, options=None, **opt_kw):
        self.lib = load_library()
        if self.lib.ptx_device_count() < 1:
            raise PathTracerError("no HIP device is visible; the path tracer has no CPU path")
        self.options = options if options is not None else default_options(**opt_kw)
        devs = (C.c_int * len(devices))(*devices)
        h = vp()
        _check(self.lib.ptx_multi_create(scene.h, C.byref(self.options), devs, len(devices), tile_rows, C.byref(h)), "ptx_multi_create")
        self.h, self.n = h, len(devices)
        self.width, self.height = scene.resolution

    def render(self, iter_first, count):
        _check(self.lib.ptx_multi_render(self.h, iter_first, count), "ptx_multi_render")

    def pathtrace(self, iteration):
        _check(self.lib.ptx_multi_iterate(self.h, iteration), "ptx_multi_iterate")

    def set_render_ahead(self, on=True):
        _check(self.lib.ptx_multi_set_render_ahead(self.h, 1 if on else 0), "ptx_multi_set_render_ahead")

    def synchronize(self):
        _check(self.lib.ptx_multi_synchronize(self.h), "ptx_multi_synchronize")

    def assemble(self):
        _check(self.lib.ptx_multi_assemble(self.h), "ptx_multi_assemble")

    def device_image_ptr(self):
        """ptx_multi_device_image: the assembled frame on the first device, W*H*3 floats (current after assemble())"""
        return self.lib.ptx_multi_device_image(self.h)

    def read_image(self):
        out = np.zeros((self.width * self.height, 3), np.float32)
        _check(self.lib.ptx_multi_read_image(self.h, _ptr(out)), "ptx_multi_read_image")
        return out

    def read_albedo(self):
        out = np.zeros((self.width * self.height, 3), np.float32)
        _check(self.lib.ptx_multi_read_albedo(self.h, _ptr(out)), "ptx_multi_read_albedo")
        return out

    def stats(self):
        s = Stats()
        _check(self.lib.ptx_multi_get_stats(self.h, C.byref(s)), "ptx_multi_get_stats")
        return dict(bounces=s.bounces, rays_per_bounce=[int(s.rays_per_bounce[b]) for b in range(min(s.bounces, 64))],
                    rays_total=int(s.rays_total), loop_ms_total=float(s.loop_ms_total), iterations=int(s.iterations), fenced=int(s.fenced), stored_paths=int(s.stored_paths),
                    stored_with_direction=int(s.stored_with_direction), stored_with_normal_code=int(s.stored_with_normal_code))


class Tracer(_Owned):
    """pathtraceInit / pathtrace / pathtraceFree on one device (opaque ptx_tracer)."""
    _destroy = "ptx_destroy"

    def __init__(self, scene, options=None, external_image_ptr=None, stream_ptr=None, **opt_kw):
        self.lib = load_library()
        if self.lib.ptx_device_count() < 1:
            raise PathTracerError("no HIP device is visible; the path tracer has no CPU path")
        self.options = options if options is not None else default_options(**opt_kw)
        h = vp()
        _check(self.lib.ptx_create_from_scene(scene.h, C.byref(self.options), external_image_ptr, stream_ptr, C.byref(h)),
               "ptx_create")
        self.h = h
        self.width, self.height = scene.resolution
        self.trace_depth = scene.trace_depth
        self.iteration = 0

    @classmethod
    def from_pod(cls, dump, options=None, **opt_kw):
        """pathtraceInit from plain scene arrays instead of a scene file: ptx_create (include/mi355x_pathtracer.h) with the POD
        dict `Scene.dump()` returns (geom_ints [type, material, faces], geom_mats [transform, inverse, invTranspose], materials,
        faces per geom, cam_ints [W, H, iterations, depth], cam_floats, textures {(geom, kd|ks|ke|bump): uint8 HxWxC}) -- the
        way a caller that holds a loaded `Scene` of the reference (src/scene.h:11-32) hands its vectors over."""
        self = cls.__new__(cls)
        self.lib = load_library()
        if self.lib.ptx_device_count() < 1:
            raise PathTracerError("no HIP device is visible; the path tracer has no CPU path")
        self.options = options if options is not None else default_options(**opt_kw)
        ng, nm = len(dump["geom_ints"]), len(dump["materials"])
        geoms = (Geom * max(ng, 1))()
        keep = []                                           # host arrays the structs point into, until ptx_create has uploaded them
        trs = dump.get("geom_trs")
        for i in range(ng):
            g = geoms[i]
            g.type, g.materialid = int(dump["geom_ints"][i][0]), int(dump["geom_ints"][i][1])
            if trs is not None:
                g.translation[:], g.rotation[:], g.scale[:] = [list(map(float, trs[i][k:k + 3])) for k in (0, 3, 6)]
            gm = np.ascontiguousarray(dump["geom_mats"][i], np.float32)
            g.transform[:], g.inverseTransform[:], g.invTranspose[:] = list(gm[:16]), list(gm[16:32]), list(gm[32:48])
            f = np.ascontiguousarray(dump["faces"][i], np.float32).reshape(-1, 15)
            keep.append(f)
            g.faceSize = len(f)
            g.faces = f.ctypes.data_as(C.POINTER(C.c_float)) if len(f) else None
            for which, name in enumerate(("kd", "ks", "ke", "bump")):          # checker order: kd, ks, ke, bump
                img = (dump.get("textures") or {}).get((i, which))
                if img is not None:
                    img = np.ascontiguousarray(img, np.uint8)
                    keep.append(img)
                    t = getattr(g, name)
                    t.height, t.width, t.channels = img.shape
                    t.image = img.ctypes.data_as(C.POINTER(C.c_uint8))
        mats = (Material * max(nm, 1))()
        for i in range(nm):
            C.memmove(C.byref(mats[i]), np.ascontiguousarray(dump["materials"][i], np.float32).ctypes.data, 44)
        cam = Camera()
        ci, cf = dump["cam_ints"], [float(v) for v in dump["cam_floats"]]
        cam.resolution[:] = [int(ci[0]), int(ci[1])]
        cam.position[:], cam.lookAt[:], cam.view[:], cam.up[:], cam.right[:] = cf[0:3], cf[3:6], cf[6:9], cf[9:12], cf[12:15]
        cam.fov[:], cam.pixelLength[:] = cf[15:17], cf[17:19]
        h = vp()
        _check(self.lib.ptx_create(ng, geoms, nm, mats, C.byref(cam), int(ci[3]), C.byref(self.options), None, None, C.byref(h)), "ptx_create")
        self.h = h
        self.width, self.height = int(ci[0]), int(ci[1])
        self.trace_depth = int(ci[3])
        self.iteration = 0
        return self

    # --- the reference's per-frame call -----------------------------------------------------------------
    def pathtrace(self, iteration, read_image=False):
        _check(self.lib.ptx_iterate(self.h, iteration), "ptx_iterate")
        self.iteration = iteration
        return self.read_image() if read_image else None

    def set_render_ahead(self, on=True):
        """ptx_set_render_ahead: iterate() calls that count up are served from batches traced in the background"""
        _check(self.lib.ptx_set_render_ahead(self.h, 1 if on else 0), "ptx_set_render_ahead")

    def render(self, iter_first, count, stride=1):
        """iterations iter_first, iter_first + stride, ... (count of them), no host round trip in between"""
        _check(self.lib.ptx_render_strided(self.h, iter_first, count, stride), "ptx_render_strided")
        self.iteration = iter_first + (count - 1) * stride

    def write_image(self, rgb_sum):
        """uploads an accumulation buffer (what read_image returned earlier): resume from a checkpoint"""
        buf = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
        if buf.size != self.width * self.height * 3:
            raise PathTracerError("write_image: expected %d floats, got %d" % (self.width * self.height * 3, buf.size))
        _check(self.lib.ptx_write_image(self.h, _ptr(buf)), "ptx_write_image")

    CKPT_MAGIC = b"PTXCKPT1"

    def save_checkpoint(self, path, iterations_done):
        """accumulation buffer + the number of iterations in it; same file format as mi355x_pathtrace --checkpoint
        (csrc/pt_image.h: magic, int32 W, H, int64 iterations, W*H*3 float32)"""
        img = self.read_image()
        with open(path, "wb") as f:
            f.write(self.CKPT_MAGIC)
            f.write(np.int32([self.width, self.height]).tobytes())
            f.write(np.int64([iterations_done]).tobytes())
            f.write(np.ascontiguousarray(img, "<f4").tobytes())

    def load_checkpoint(self, path):
        """-> iterations already in the buffer; continue with render(iterations + 1, ...)"""
        with open(path, "rb") as f:
            if f.read(8) != self.CKPT_MAGIC:
                raise PathTracerError("%s is not a checkpoint file" % path)
            w, h = (int(v) for v in np.frombuffer(f.read(8), "<i4"))
            iters = int(np.frombuffer(f.read(8), "<i8")[0])
            if (w, h) != (self.width, self.height):
                raise PathTracerError("checkpoint %s is %dx%d, the tracer is %dx%d" % (path, w, h, self.width, self.height))
            data = np.frombuffer(f.read(), "<f4")
        if data.size != w * h * 3:
            raise PathTracerError("checkpoint %s is truncated" % path)
        self.write_image(data)
        return iters

    def synchronize(self):
        _check(self.lib.ptx_synchronize(self.h), "ptx_synchronize")

    def set_camera(self, scene):
        _check(self.lib.ptx_set_camera(self.h, C.byref(scene.camera), scene.trace_depth), "ptx_set_camera")

    def reset_image(self):
        _check(self.lib.ptx_reset_image(self.h), "ptx_reset_image")

    # --- active tiles (include/mi355x_pathtracer.h: ptx_set_active_tiles) ----------------------------------
    @property
    def num_tiles(self):
        """tiles of tile_pixels() owned pixels, tile = (y * W + x) // tile_pixels()"""
        return int(self.lib.ptx_num_tiles(self.h))

    def set_active_tiles(self, mask):
        """num_tiles flags, nonzero = active: the camera bounce of the other tiles traces nothing, their pixels keep their sums"""
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, np.uint8)
        _check(self.lib.ptx_set_active_tiles(self.h, _ptr(m), len(m)), "ptx_set_active_tiles")

    def clear_active_tiles(self):
        _check(self.lib.ptx_clear_active_tiles(self.h), "ptx_clear_active_tiles")

    def read_image(self):
        out = np.zeros((self.width * self.height, 3), np.float32)
        _check(self.lib.ptx_read_image(self.h, _ptr(out)), "ptx_read_image")
        return out

    def read_albedo(self):
        out = np.zeros((self.width * self.height, 3), np.float32)
        _check(self.lib.ptx_read_albedo(self.h, _ptr(out)), "ptx_read_albedo")
        return out

    def denoised_pbo(self, rgb):
        rgb = np.ascontiguousarray(rgb, np.float32).reshape(self.width * self.height, 3)
        out = np.zeros((self.width * self.height, 4), np.uint8)
        _check(self.lib.ptx_write_denoised_pbo(self.h, _ptr(rgb), _ptr(out)), "ptx_write_denoised_pbo")
        return out

    def denoised_pbo_device(self, rgb, device_pbo):
        """sendToGPU (apps/src/pathtrace.cu:673-685): host frame -> 8-bit preview in a device buffer (address as int)"""
        rgb = np.ascontiguousarray(rgb, np.float32).reshape(self.width * self.height, 3)
        _check(self.lib.ptx_write_denoised_pbo_device(self.h, _ptr(rgb), device_pbo), "ptx_write_denoised_pbo_device")

    # --- denoiser (include/mi355x_pathtracer.h: ptx_denoise ...) ------------------------------------------
    def denoise(self, spp, read=True, passes=None, demodulate=None, phi_color=None, phi_normal=None, phi_position=None):
        """a-trous denoise of the accumulation buffer / spp on the device; returns the (H, W, 3) float32 mean radiance (read=False:
        only enqueues it -- device_denoised_ptr / denoised_pbo_from_device then use it where it is)"""
        p = default_denoise_params(passes=passes, demodulate=demodulate, phi_color=phi_color, phi_normal=phi_normal, phi_position=phi_position)
        _check(self.lib.ptx_denoise(self.h, C.byref(p), int(spp)), "ptx_denoise")
        return self.read_denoised() if read else None

    def denoise_temporal(self, temporal, spp, read=True, passes=None, demodulate=None, phi_color=None, phi_normal=None,
                         phi_position=None, max_history=None, specular_history=None, normal_cos=None, plane_tolerance=None):
        """denoise() with temporal reuse (ptx_denoise_temporal): the previous view's samples in `temporal` (a Temporal) reprojected
        into this view and mixed with the accumulation buffer / spp, then the a-trous filter.  Returns the (H, W, 3) float32 mean
        radiance (read=False: only enqueues it); temporal.read() gives the history and the mix."""
        dp = default_denoise_params(passes=passes, demodulate=demodulate, phi_color=phi_color, phi_normal=phi_normal, phi_position=phi_position)
        tp = default_temporal_params(max_history=max_history, specular_history=specular_history, normal_cos=normal_cos,
                                     plane_tolerance=plane_tolerance)
        _check(self.lib.ptx_denoise_temporal(self.h, temporal.h, C.byref(dp), C.byref(tp), int(spp)), "ptx_denoise_temporal")
        return self.read_denoised() if read else None

    def denoise_variance(self, spp, temporal=None, read=True, **params):
        """denoise() / denoise_temporal() with the variance-guided filter (ptx_denoise_variance): the luminance weight of every pass is
        normalised by a per-pixel estimate of the input's variance instead of phi_color.  temporal: a Temporal or None; params: any
        field of ptx_denoise_params, ptx_temporal_params and ptx_variance_params.  variance() gives the estimate."""
        dp, tp, vpar = _split_variance_params("denoise_variance", params)
        _check(self.lib.ptx_denoise_variance(self.h, None if temporal is None else temporal.h, C.byref(dp), C.byref(tp), C.byref(vpar),
                                             int(spp)), "ptx_denoise_variance")
        return self.read_denoised() if read else None

    def denoise_measured(self, moments, spp, min_batches=None, read=True, temporal=None, **params):
        """denoise_variance() with the variance measured by `moments` (a Moments fed from this tracer's buffer) in place of the spatial
        estimate, on every hit pixel with at least min_batches batches (None: 4); params: any field of ptx_denoise_params and
        ptx_variance_params.  variance() gives the v0 it used.
        temporal: a Temporal: denoise_variance(spp, temporal) whose per-sample variance pools the measured one with the history's
        (ptx_denoise_temporal_measured); params may then name ptx_temporal_params' fields too.  Reset `moments` at every camera step."""
        mb = 0 if min_batches is None else int(min_batches)
        if temporal is not None:
            dp, tp, vpar = _split_variance_params("denoise_measured", params)
            _check(self.lib.ptx_denoise_temporal_measured(self.h, temporal.h, moments.h, C.byref(dp), C.byref(tp), C.byref(vpar), mb,
                                                          int(spp)), "ptx_denoise_temporal_measured")
            return self.read_denoised() if read else None
        for k in params:
            if k not in _DENOISE_KEYS + _VARIANCE_KEYS:
                raise TypeError("denoise_measured: unknown parameter %r" % k)
        dp, _, vpar = _split_variance_params("denoise_measured", params)
        _check(self.lib.ptx_denoise_measured(self.h, moments.h, C.byref(dp), C.byref(vpar), mb, int(spp)), "ptx_denoise_measured")
        return self.read_denoised() if read else None

    def denoise_adaptive(self, adaptive, moments, min_batches=None, read=True, **params):
        """denoise_measured() on an adaptively sampled frame (ptx_denoise_adaptive): the accumulation buffer over every tile's own count
        from `adaptive` (an Adaptive), and the variance `moments` measured with every pixel's own W and B; hit pixels with fewer than
        min_batches batches (None: 4) take the spatial estimate.  params: any field of ptx_denoise_params and ptx_variance_params.
        Includes adaptive.resolve(tracer): adaptive.read()["mean"] is current after it.  variance() gives the v0 it used."""
        for k in params:
            if k not in _DENOISE_KEYS + _VARIANCE_KEYS:
                raise TypeError("denoise_adaptive: unknown parameter %r" % k)
        dp, _, vpar = _split_variance_params("denoise_adaptive", params)
        _check(self.lib.ptx_denoise_adaptive(self.h, adaptive.h, moments.h, C.byref(dp), C.byref(vpar),
                                             0 if min_batches is None else int(min_batches)), "ptx_denoise_adaptive")
        return self.read_denoised() if read else None

    def denoise_nn(self, nn, spp, read=True, prefilter=None, prefilter_params=None, **params):
        """The network denoiser (ptx_denoise_nn) on the accumulation buffer / spp with albedo and normals from the G-buffer in the guide
        mode that is set, `nn` an NN of this tracer's size and device; params: ptx_nn_params' fields (hdr, srgb, input_scale).  Returns the
        (H, W, 3) float32 frame (read=False: only enqueues it); the result is the tracer's denoised frame, as after denoise().
        prefilter: an NNPrefilter of this size and device (ptx_denoise_nn_prefiltered): the main network gets its clean guides, which
        are computed once per G-buffer; prefilter_params: a dict of ptx_nn_prefilter_params' fields (srgb, input_scale)."""
        p = default_nn_params(**params)
        if prefilter is None:
            if prefilter_params is not None:
                raise PathTracerError("denoise_nn: prefilter_params without a prefilter")
            _check(self.lib.ptx_denoise_nn(self.h, nn.h, C.byref(p), int(spp)), "ptx_denoise_nn")
        else:
            pp = default_nn_prefilter_params(**(prefilter_params or {}))
            _check(self.lib.ptx_denoise_nn_prefiltered(self.h, nn.h, prefilter.h, C.byref(p), C.byref(pp), int(spp)), "ptx_denoise_nn_prefiltered")
        return self.read_denoised() if read else None

    def compare(self, metrics, reference, spp, source="image", **params):
        """ptx_metrics_tracer: the accumulation buffer over spp (source "image") or the last denoised frame (source "denoised") against
        `reference`, a host image as Metrics.host takes it, on the tracer's stream; params: transform, exposure, threshold, samples_b.
        Returns Metrics.host's dict.  Nothing of the tracer changes."""
        p = default_metrics_params(**params)
        src = _DISPLAY_SOURCES[source] if isinstance(source, str) else int(source)
        ib = metrics._image(reference)
        out = MetricsResult(struct_size=C.sizeof(MetricsResult))
        _check(self.lib.ptx_metrics_tracer(metrics.h, self.h, src, int(spp), C.byref(ib), C.byref(p), C.byref(out)), "ptx_metrics_tracer")
        return _metrics_dict(out)

    def variance(self):
        """The last denoise_variance's input variance v0 = V / n and the last pass's variance, (H, W) float32 each."""
        vin, vout = np.zeros((self.height, self.width), np.float32), np.zeros((self.height, self.width), np.float32)
        _check(self.lib.ptx_read_variance(self.h, _ptr(vin), _ptr(vout)), "ptx_read_variance")
        return dict(input=vin, output=vout)

    def read_denoised(self):
        out = np.zeros((self.height, self.width, 3), np.float32)
        _check(self.lib.ptx_read_denoised(self.h, _ptr(out)), "ptx_read_denoised")
        return out

    def device_denoised_ptr(self):
        return self.lib.ptx_device_denoised(self.h)

    def denoised_pbo_from_device(self, device_pbo):
        """sendToGPU of the last denoise (still on the device) into a device pbo (address as int); enqueued on the tracer's stream"""
        _check(self.lib.ptx_write_denoised_pbo_from_device(self.h, device_pbo), "ptx_write_denoised_pbo_from_device")

    def gbuffer(self):
        """The denoiser's G-buffer of the current camera: dict of (H, W, ...) arrays position, normal, albedo (float32 x 3), material,
        geom (int32), t (float32), hit (bool)"""
        h, w = self.height, self.width
        pos, nrm, alb = (np.zeros((h, w, 3), np.float32) for _ in range(3))
        ids, t, hit = np.zeros((h, w, 2), np.int32), np.zeros((h, w), np.float32), np.zeros((h, w), np.uint8)
        _check(self.lib.ptx_read_gbuffer(self.h, _ptr(pos), _ptr(nrm), _ptr(alb), _ptr(ids), _ptr(t), _ptr(hit)), "ptx_read_gbuffer")
        return dict(position=pos, normal=nrm, albedo=alb, material=ids[..., 0].copy(), geom=ids[..., 1].copy(), t=t, hit=hit != 0)

    def set_guide_samples(self, count, iter_first=1):
        """count >= 1: the denoiser's guides averaged over the camera rays of iterations iter_first .. iter_first + count - 1, with the
        tracer's own antialiasing jitter and lens (ptx_set_guide_samples); 0: the pixel-centre guides, the default"""
        _check(self.lib.ptx_set_guide_samples(self.h, int(iter_first), int(count)), "ptx_set_guide_samples")

    def guide_samples(self):
        """(count, iter_first) as set_guide_samples left them"""
        first, count = C.c_int(0), C.c_int(0)
        _check(self.lib.ptx_get_guide_samples(self.h, C.byref(first), C.byref(count)), "ptx_get_guide_samples")
        return count.value, first.value

    def set_guide_bounces(self, bounces):
        """bounces >= 1: the denoiser's guide rays followed through mirrors and glass, at most min(bounces, trace depth - 1) times, to
        the surface seen in them (ptx_set_guide_bounces); 0: the first surface, the default"""
        _check(self.lib.ptx_set_guide_bounces(self.h, int(bounces)), "ptx_set_guide_bounces")

    def guide_bounces(self):
        """the value set_guide_bounces left"""
        b = C.c_int()
        _check(self.lib.ptx_get_guide_bounces(self.h, C.byref(b)), "ptx_get_guide_bounces")
        return b.value

    def guide_coverage(self):
        """(H, W) float32: the share of the guide samples that hit a surface (pixel-centre guides: the hit flag)"""
        out = np.zeros((self.height, self.width), np.float32)
        _check(self.lib.ptx_read_guide_coverage(self.h, _ptr(out)), "ptx_read_guide_coverage")
        return out

    def pbo(self, iteration):
        out = np.zeros((self.width * self.height, 4), np.uint8)
        _check(self.lib.ptx_write_pbo(self.h, iteration, _ptr(out)), "ptx_write_pbo")
        return out

    def device_image_ptr(self):
        return self.lib.ptx_device_image(self.h)

    def stream_ptr(self):
        return self.lib.ptx_stream(self.h)

    def last_loop_ms(self):
        return float(self.lib.ptx_last_loop_ms(self.h))

    def set_kernel_timing(self, on):
        _check(self.lib.ptx_set_kernel_timing(self.h, int(bool(on))), "ptx_set_kernel_timing")

    def kernel_times(self):
        """{kernel: (total ms, launches)} since the last call (needs set_kernel_timing(True))."""
        ms = np.zeros(4, np.float64)
        n = np.zeros(4, np.int64)
        _check(self.lib.ptx_get_kernel_times(self.h, _ptr(ms), _ptr(n)), "ptx_get_kernel_times")
        names = ("k_bounce<first>", "k_bounce", "k_mesh", "k_bounce pass2")      # (split mesh search: the first two are then its pass 1)
        return {nm: (float(ms[k]), int(n[k])) for k, nm in enumerate(names)}

    def kat_fast_exact(self):
        """mismatches of the device's guarded core sqrt / 1/sqrt / 1/a against the compiler's IEEE expansions over all 2^32 operands"""
        m = np.zeros(3, np.int64)
        _check(self.lib.ptx_kat_fast_exact(self.h, _ptr(m)), "ptx_kat_fast_exact")
        return m.tolist()

    def kat_unit_rsqrt(self, exponent_reps=64, random_sets=1 << 26):
        """[pt_rsqrt_unit != pt_rsqrt_glm over all 2^32 operands, operands in the window, slab quotients != a / d, sets through the shared reciprocal]"""
        m = np.zeros(4, np.int64)
        _check(self.lib.ptx_kat_unit_rsqrt(self.h, int(exponent_reps), int(random_sets), _ptr(m)), "ptx_kat_unit_rsqrt")
        return m.tolist()

    def owned_pixels(self):
        return self.lib.ptx_owned_pixels(self.h)

    def mesh_plan(self, gi):
        """ptx_debug_mesh_plan (host only): how mesh geom gi is searched -- dict(root, depth, wroot, wneed, bvh_stack, split, frame_walk,
        stack_walk), the walks as WALK_NAMES: what a frame takes for it, and what the single-ray search takes when handed a stack
        (tile_intersect(split=True)); every other entry point searches without a stack: "loop" without a tree, "skip" with one."""
        o = np.zeros(8, np.int32)
        _check(self.lib.ptx_debug_mesh_plan(self.h, int(gi), _ptr(o)), "ptx_debug_mesh_plan")
        d = dict(zip(("root", "depth", "wroot", "wneed", "bvh_stack", "split"), (int(x) for x in o[:6])))
        d["frame_walk"], d["stack_walk"] = WALK_NAMES[int(o[6])], WALK_NAMES[int(o[7])]
        return d

    def index_plan(self):
        """ptx_debug_index_plan (host only): the layout of the local index this tracer's launches use -- dict(loop, n2_log2, words, entries,
        seg_words, bytes_per_path, slots, why); loop = bin-major and written in k_bounce's tile loop, why = 0 or the term of the plan's
        predicate that sent the tracer back to the tail's chunk-compact index."""
        o = np.zeros(8, np.int64)
        _check(self.lib.ptx_debug_index_plan(self.h, _ptr(o)), "ptx_debug_index_plan")
        d = dict(zip(("loop", "n2_log2", "words", "entries", "seg_words", "bytes_per_path", "slots", "why"), (int(x) for x in o)))
        d["loop"] = bool(d["loop"])
        return d

    def stats(self):
        s = Stats()
        _check(self.lib.ptx_get_stats(self.h, C.byref(s)), "ptx_get_stats")
        return dict(bounces=s.bounces, rays_per_bounce=[int(s.rays_per_bounce[b]) for b in range(min(s.bounces, 64))],
                    rays_total=int(s.rays_total), loop_ms_total=float(s.loop_ms_total), iterations=int(s.iterations), fenced=int(s.fenced), stored_paths=int(s.stored_paths),
                    stored_with_direction=int(s.stored_with_direction), stored_with_normal_code=int(s.stored_with_normal_code))

    # --- per-stage entry points used by the parity tests --------------------------------------------------
    def geom_test(self, gi, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((len(rays), 10), np.float32)
        _check(self.lib.ptx_kat_geom_test(self.h, gi, len(rays), _ptr(rays), _ptr(out)), "ptx_kat_geom_test")
        return out

    def obj_tri_test(self, gi, rays):
        """objTriIntersectionTest of the reference (src/intersections.h:284-315, dead code there) on OBJ geom gi: (n, 8) = t, point, normal, outside"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((len(rays), 8), np.float32)
        _check(self.lib.ptx_kat_obj_tri_test(self.h, gi, len(rays), _ptr(rays), _ptr(out)), "ptx_kat_obj_tri_test")
        return out

    def jittered_hemisphere(self, normals, seeds, max_iter=5000):
        """calculateJitteredDirectionHemisphere of the reference (src/interactions.h:46-85, dead code there): (n, 3) normals and (n, 3) int
        (iter, index, depth) -> (n, 3) directions"""
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        seeds = np.ascontiguousarray(seeds, np.int32).reshape(-1, 3)
        out = np.zeros((len(normals), 3), np.float32)
        _check(self.lib.ptx_kat_jittered_hemisphere(self.h, len(normals), _ptr(normals), _ptr(seeds), int(max_iter), _ptr(out)), "ptx_kat_jittered_hemisphere")
        return out

    def compute_intersections(self, paths):
        paths = np.ascontiguousarray(paths)
        assert paths.dtype.itemsize == 44
        out = np.zeros(len(paths), np.dtype([("t", "<f4"), ("normal", "<f4", 3), ("materialId", "<i4"),
                                             ("texcoord", "<f4", 2), ("geomId", "<i4")]))
        _check(self.lib.ptx_kat_compute_intersections(self.h, len(paths), _ptr(paths), _ptr(out)), "ptx_kat_compute_intersections")
        return out

    def tile_intersect(self, paths, split=False):
        """computeIntersections through the production functions (cullMask, primKey / meshKey, decodeKey): ptx_kat_tile_intersect"""
        paths = np.ascontiguousarray(paths)
        assert paths.dtype.itemsize == 44
        out = np.zeros(len(paths), np.dtype([("t", "<f4"), ("normal", "<f4", 3), ("materialId", "<i4"),
                                             ("texcoord", "<f4", 2), ("geomId", "<i4")]))
        _check(self.lib.ptx_kat_tile_intersect(self.h, len(paths), _ptr(paths), _ptr(out), 1 if split else 0), "ptx_kat_tile_intersect")
        return out

    def shade(self, iteration, idx, isects, paths):
        paths = np.array(paths, copy=True)
        isects = np.ascontiguousarray(isects)
        idx = np.ascontiguousarray(idx, np.int32)
        assert paths.dtype.itemsize == 44 and isects.dtype.itemsize == 32
        _check(self.lib.ptx_kat_shade(self.h, iteration, len(paths), _ptr(idx), _ptr(isects), _ptr(paths)), "ptx_kat_shade")
        return paths

    def generate(self, iteration):
        out = np.zeros(self.width * self.height, np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("color", "<f4", 3),
                                                            ("pixelIndex", "<i4"), ("remainingBounces", "<i4")]))
        _check(self.lib.ptx_kat_generate(self.h, iteration, _ptr(out)), "ptx_kat_generate")
        return out

    def libm(self, x, pw, pxy):
        x = np.ascontiguousarray(x, np.float32)
        pw = np.ascontiguousarray(pw, np.float64)
        pxy = np.ascontiguousarray(pxy, np.float32).reshape(-1, 2)
        n = len(x)
        assert len(pw) == n and len(pxy) == n
        s, c, po = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        p5 = np.zeros(n, np.float64)
        _check(self.lib.ptx_kat_libm(self.h, n, _ptr(x), _ptr(s), _ptr(c), _ptr(pw), _ptr(p5), _ptr(pxy), _ptr(po)), "ptx_kat_libm")
        return s, c, p5, po

    def debug_capture(self, bounce):
        _check(self.lib.ptx_debug_set_capture(self.h, bounce), "ptx_debug_set_capture")

    def debug_stream(self):
        cap = self.width * self.height
        pix, idx, mat = (np.zeros(cap, np.int32) for _ in range(3))
        n = C.c_int(0)
        _check(self.lib.ptx_debug_read_stream(self.h, C.byref(n), _ptr(pix), _ptr(idx), _ptr(mat), None, 0), "ptx_debug_read_stream")
        m = n.value
        fields = np.zeros((14, max(m, 1)), np.float32)
        _check(self.lib.ptx_debug_read_stream(self.h, C.byref(n), _ptr(pix), _ptr(idx), _ptr(mat), _ptr(fields), m), "ptx_debug_read_stream")
        names = ("px", "py", "pz", "dx", "dy", "dz", "cr", "cg", "cb", "nx", "ny", "nz", "u", "v")
        out = dict(pix=pix[:m].copy(), idx=idx[:m].copy(), mat=mat[:m].copy())
        for k, nm in enumerate(names):
            out[nm] = fields[k, :m].copy()
        return out


class StreamCompaction:
    """namespace StreamCompaction (stream_compaction/*.cu): host arrays in, host arrays out."""

    def __init__(self):
        self.lib = load_library()

    def _scan(self, fn, a):
        a = np.ascontiguousarray(a, np.int32)
        out = np.zeros_like(a)
        rc = fn(len(a), _ptr(out), _ptr(a))
        if rc:
            _check(rc, fn.__name__)
        return out

    def cpu_scan(self, a):
        a = np.ascontiguousarray(a, np.int32)
        out = np.zeros_like(a)
        self.lib.sc_cpu_scan(len(a), _ptr(out), _ptr(a))
        return out

    def cpu_compact_without_scan(self, a):
        a = np.ascontiguousarray(a, np.int32)
        out = np.zeros_like(a)
        n = self.lib.sc_cpu_compact_without_scan(len(a), _ptr(out), _ptr(a))
        return out[:n].copy()

    def cpu_compact_with_scan(self, a):
        a = np.ascontiguousarray(a, np.int32)
        out = np.zeros_like(a)
        n = self.lib.sc_cpu_compact_with_scan(len(a), _ptr(out), _ptr(a))
        return out[:n].copy()

    def naive_scan(self, a):
        return self._scan(self.lib.sc_naive_scan, a)

    def efficient_scan(self, a):
        return self._scan(self.lib.sc_efficient_scan, a)

    def thrust_scan(self, a):
        return self._scan(self.lib.sc_thrust_scan, a)

    def efficient_compact(self, a):
        a = np.ascontiguousarray(a, np.int32)
        out = np.zeros_like(a)
        n = self.lib.sc_efficient_compact(len(a), _ptr(out), _ptr(a))
        if n < 0:
            raise PathTracerError("sc_efficient_compact failed: %s" % self.lib.ptx_last_error().decode())
        return out[:n].copy()

    # device-pointer forms (addresses as ints, e.g. torch tensor.data_ptr(); stream = a hipStream_t handle or 0)
    def workspace_bytes(self, n):
        return int(self.lib.sc_scan_workspace_bytes(int(n)))

    def scan_device(self, n, d_out, d_in, d_workspace, stream=0):
        _check(self.lib.sc_scan_device(int(n), d_out, d_in, d_workspace, stream), "sc_scan_device")

    def compact_device(self, n, d_out, d_in, d_count, d_workspace, stream=0):
        _check(self.lib.sc_compact_device(int(n), d_out, d_in, d_count, d_workspace, stream), "sc_compact_device")

    # StreamCompaction::Common::kernMapToBoolean / kernScatter (stream_compaction/common.cu:25-49) on device arrays
    def map_to_boolean_device(self, n, d_bools, d_in, stream=0):
        _check(self.lib.sc_map_to_boolean_device(int(n), d_bools, d_in, stream), "sc_map_to_boolean_device")

    def scatter_device(self, n, d_out, d_in, d_bools, d_indices, stream=0):
        _check(self.lib.sc_scatter_device(int(n), d_out, d_in, d_bools, d_indices, stream), "sc_scatter_device")

    # records: thrust::sort_by_key(.., sortByMaterial()) / thrust::stable_partition(.., isTerminate()) of src/pathtrace.cu:518,541
    def records_tile(self):
        return int(self.lib.sc_records_tile_elements())

    def records_workspace_bytes(self, n, nkeys):
        return int(self.lib.sc_records_workspace_bytes(int(n), int(nkeys)))

    def sort_records_by_key_device(self, n, nkeys, descending, d_keys, key_stride_bytes, d_out_a, d_in_a, record_bytes_a,
                                   d_out_b, d_in_b, record_bytes_b, d_perm, d_key_totals, d_workspace, stream=0):
        _check(self.lib.sc_sort_records_by_key_device(int(n), int(nkeys), int(bool(descending)), d_keys, int(key_stride_bytes),
                                                      d_out_a, d_in_a, int(record_bytes_a), d_out_b, d_in_b, int(record_bytes_b),
                                                      d_perm, d_key_totals, d_workspace, stream), "sc_sort_records_by_key_device")

    def partition_records_device(self, n, record_bytes, d_out, d_in, d_flags, flag_stride_bytes, d_count, d_workspace, stream=0):
        _check(self.lib.sc_partition_records_device(int(n), int(record_bytes), d_out, d_in, d_flags, int(flag_stride_bytes), d_count,
                                                    d_workspace, stream), "sc_partition_records_device")

    def compact_records_device(self, n, record_bytes, d_out, d_in, d_flags, flag_stride_bytes, d_count, d_workspace, stream=0):
        _check(self.lib.sc_compact_records_device(int(n), int(record_bytes), d_out, d_in, d_flags, int(flag_stride_bytes), d_count,
                                                  d_workspace, stream), "sc_compact_records_device")

    @staticmethod
    def _records(a, n):
        """a C-contiguous array of n records (any dtype, structured ones included) and the bytes of one record"""
        a = np.ascontiguousarray(a)
        if a.ndim < 1 or len(a) != n:
            raise PathTracerError("records: every array needs one row per key (%d), got shape %r" % (n, a.shape))
        return a, (a.nbytes // n if n else a.dtype.itemsize * int(np.prod(a.shape[1:], dtype=np.int64)))

    def sort_records_by_key(self, keys, *arrays, nkeys, descending=False):
        """Stable sort of one or two host record arrays by int keys in [0, nkeys) (clamped), ascending or descending.
        Returns (the permuted arrays as a list, perm = source index of every output row, totals = rows per mapped key)."""
        keys = np.ascontiguousarray(keys, np.int32)
        if not 1 <= len(arrays) <= 2:
            raise PathTracerError("sort_records_by_key: one or two record arrays, got %d" % len(arrays))
        n = len(keys)
        recs = [self._records(a, n) for a in arrays]
        outs = [np.empty_like(a) for a, _ in recs]
        perm = np.empty(n, np.int32)
        totals = np.zeros(max(int(nkeys), 0), np.int32)
        b = (_ptr(outs[1]), _ptr(recs[1][0]), recs[1][1]) if len(recs) == 2 else (None, None, 0)
        _check(self.lib.sc_sort_records_by_key(n, int(nkeys), int(bool(descending)), _ptr(keys), _ptr(outs[0]), _ptr(recs[0][0]), recs[0][1],
                                               b[0], b[1], b[2], _ptr(perm), _ptr(totals)), "sc_sort_records_by_key")
        return outs, perm, totals

    def _split_records(self, fn, what, records, flags):
        flags = np.ascontiguousarray(flags, np.int32)
        a, rb = self._records(records, len(flags))
        out = np.empty_like(a)
        count = C.c_int(0)
        _check(fn(len(flags), rb, _ptr(out), _ptr(a), _ptr(flags), C.byref(count)), what)
        return out, int(count.value)

    def partition_records(self, records, flags):
        """Rows with flag != 0 first, then those with flag == 0, both in order: (the partitioned array, the partition point)."""
        return self._split_records(self.lib.sc_partition_records, "sc_partition_records", records, flags)

    def compact_records(self, records, flags):
        """The rows with flag != 0, in order."""
        out, count = self._split_records(self.lib.sc_compact_records, "sc_compact_records", records, flags)
        return out[:count].copy()

    # records by full 32-bit keys: thrust::sort_by_key for keys of any value (an 8-bit LSD radix sort; the records move once)
    KEY_INT32, KEY_UINT32, KEY_FLOAT32 = 0, 1, 2

    def radix_workspace_bytes(self, n):
        return int(self.lib.sc_radix_workspace_bytes(int(n)))

    def radix_map_key(self, key_type, descending, bits):
        """the order-preserving map of 32 key bits to the unsigned value the sort compares"""
        return int(self.lib.sc_radix_map_key(int(key_type), int(bool(descending)), int(bits) & 0xffffffff))

    def radix_sort_records_device(self, n, key_type, descending, begin_bit, end_bit, d_keys, key_stride_bytes, d_out_a, d_in_a, record_bytes_a,
                                  d_out_b, d_in_b, record_bytes_b, d_perm, d_keys_out, d_workspace, stream=0):
        _check(self.lib.sc_radix_sort_records_device(int(n), int(key_type), int(bool(descending)), int(begin_bit), int(end_bit), d_keys,
                                                     int(key_stride_bytes), d_out_a, d_in_a, int(record_bytes_a), d_out_b, d_in_b, int(record_bytes_b),
                                                     d_perm, d_keys_out, d_workspace, stream), "sc_radix_sort_records_device")

    def radix_sort_records(self, keys, *arrays, key_type=None, descending=False, begin_bit=0, end_bit=32):
        """Stable sort of one or two host record arrays by bits [begin_bit, end_bit) of 32-bit keys: int32, uint32 or float32 (taken
        from keys.dtype when key_type is None; floats in the total order -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN).
        Returns (the permuted arrays as a list, perm = source index of every output row, keys_out = the keys in output order)."""
        keys = np.ascontiguousarray(keys)
        if key_type is None:
            types = {np.dtype(np.int32): self.KEY_INT32, np.dtype(np.uint32): self.KEY_UINT32, np.dtype(np.float32): self.KEY_FLOAT32}
            if keys.dtype not in types:
                raise PathTracerError("radix_sort_records: keys are int32, uint32 or float32, got %s" % keys.dtype)
            key_type = types[keys.dtype]
        if keys.dtype.itemsize != 4 or keys.ndim != 1:
            raise PathTracerError("radix_sort_records: keys are one 32-bit word per row, got %s %r" % (keys.dtype, keys.shape))
        if not 1 <= len(arrays) <= 2:
            raise PathTracerError("radix_sort_records: one or two record arrays, got %d" % len(arrays))
        n = len(keys)
        recs = [self._records(a, n) for a in arrays]
        outs = [np.empty_like(a) for a, _ in recs]
        perm, keys_out = np.empty(n, np.int32), np.empty_like(keys)
        b = (_ptr(outs[1]), _ptr(recs[1][0]), recs[1][1]) if len(recs) == 2 else (None, None, 0)
        _check(self.lib.sc_radix_sort_records(n, int(key_type), int(bool(descending)), int(begin_bit), int(end_bit), _ptr(keys), _ptr(outs[0]),
                                              _ptr(recs[0][0]), recs[0][1], b[0], b[1], b[2], _ptr(perm), _ptr(keys_out)), "sc_radix_sort_records")
        return outs, perm, keys_out

    def last_gpu_ms(self):
        return float(self.lib.sc_last_gpu_ms())

    def last_cpu_ms(self):
        return float(self.lib.sc_last_cpu_ms())
