"""mygpuraytracer_amd -- MI355X-native Monte-Carlo path tracer.

Drop-in for the ``pathtraceInit / pathtrace(iter) / pathtraceFree`` path and the ``scenes/*.txt`` loader of
nkkk98/MyGPURaytracer.  The compute path is hand-written HIP for gfx950 in ``csrc/`` behind the C ABI declared in
``include/mi355x_pathtracer.h`` and ``include/mi355x_stream_compaction.h``; this package is the thin Python host
side over that ABI (ctypes), used by the tests, ``bench.py`` and the multi-GPU driver.

There is no CPU fallback: importing works anywhere (so that CPU-only tooling can inspect the ABI), but creating a
tracer without the built library or without a HIP device raises.
"""
from .api import (  # noqa: F401
    LIB_PATH,
    PathTracerError,
    Cancelled,
    Options,
    DenoiseParams,
    TemporalParams,
    VarianceParams,
    MomentsParams,
    MomentsSummary,
    AdaptiveParams,
    AdaptiveStatus,
    Adaptive,
    DisplayParams,
    DisplayStatus,
    Display,
    default_display_params,
    NNParams,
    NNInfo,
    NN,
    default_nn_params,
    nn_denoise_buffers,
    debug_tza_list,
    debug_nn_plan,
    debug_nn_tiling,
    NNTile,
    NNTiling,
    kat_nn_conv,
    kat_nn_transfer,
    NNPrefilter,
    NNPrefilterParams,
    NNPrefilterInfo,
    NN_AUX_ALBEDO,
    NN_AUX_NORMAL,
    default_nn_prefilter_params,
    debug_nn_prefilter_problem,
    kat_nn_transfer_aux,
    NNImage,
    NN_FORMAT_FLOAT3,
    NN_FORMAT_HALF3,
    nn_image_of,
    debug_nn_image_problem,
    Scene,
    Tracer,
    Temporal,
    Moments,
    MultiTracer,
    StreamCompaction,
    build_library,
    default_denoise_params,
    default_temporal_params,
    default_variance_params,
    default_moments_params,
    default_adaptive_params,
    tile_pixels,
    denoise_buffers,
    denoise_buffers_variance,
    reproject_buffers,
    load_library,
)

__all__ = ["LIB_PATH", "PathTracerError", "Cancelled", "Options", "DenoiseParams", "TemporalParams", "VarianceParams", "MomentsParams", "MomentsSummary", "AdaptiveParams", "AdaptiveStatus", "Adaptive", "DisplayParams", "DisplayStatus", "Display", "default_display_params", "NNParams", "NNInfo", "NN", "default_nn_params", "nn_denoise_buffers", "debug_tza_list", "debug_nn_plan", "kat_nn_conv", "kat_nn_transfer", "NNPrefilter", "NNPrefilterParams", "NNPrefilterInfo", "NN_AUX_ALBEDO", "NN_AUX_NORMAL", "default_nn_prefilter_params", "debug_nn_prefilter_problem", "kat_nn_transfer_aux", "NNImage", "NN_FORMAT_FLOAT3", "NN_FORMAT_HALF3", "nn_image_of", "debug_nn_image_problem", "Scene", "Tracer", "Temporal", "Moments", "MultiTracer",
           "StreamCompaction", "build_library", "default_denoise_params", "default_temporal_params", "default_variance_params", "default_moments_params", "default_adaptive_params", "tile_pixels", "denoise_buffers",
           "denoise_buffers_variance", "reproject_buffers", "load_library"]
