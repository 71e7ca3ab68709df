// pt_nn.h -- internal interface of the network denoiser (pt_nn.hip: ptx_nn_* of include/mi355x_pathtracer.h) towards the tracer
// (pt_post.hip: ptx_denoise_nn, which needs the tracer's accumulation buffer, G-buffer, denoised frame and stream).  Not part of the C
// ABI; include/mi355x_pathtracer.h has the public side and the definition of the arithmetic.
//
// Device state of a handle:
//   per layer: the weights as fp16 in the convolution's fragment order (pack_weights) and the padded fp32 bias, written once at create
//   d_scratch: the activations of one tile (pt_nn_tiles.h: the whole frame, or the tile buffer of a handle made under a memory limit;
//              a smaller tile uses a prefix of each tensor), channels-last fp16, planned once at create: the network's input and the three pooled skips each in a
//              place of their own, every other tensor in one of two arenas that the layers write in turn (a layer reads one arena and
//              writes the other); dec_conv0's fp32 output, four floats per pixel, is the last tenant of the second arena
//   d_scale  : the scale the last input kernel used, written by it and read by the output kernel
//   meter    : a display handle for the block meter (hdr with automatic scale), made by the first call that needs it
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_handle.h"
#include "pt_tza.h"
#include "pt_nn_tiles.h"

struct ptx_display;

struct PtNnLayerDev {
    int cin0 = 0, cin1 = 0, cout = 0;             // the blob's counts
    int c0p = 0, c1p = 0, coutp = 0;              // padded to 16, the two sources separately
    int level = 0, src0 = -2, src1 = -2;
    bool relu = true, pool = false, upsample = false;
    DevBuf<uint16_t> w;                           // fp16 bits, fragment order
    DevBuf<float> b;
    size_t out_offset = 0;                        // of its output in d_scratch (bytes)
};

struct ptx_nn : PtHandle {
    int wp = 0, hp = 0, ic = 0;                   // the padded tile buffer (one tile: the padded frame), the network's input channels
    PtNnTiling tiling;                            // the frame's tiles (pt_nn_tiles.h); one tile unless made by ptx_nn_create_tiled
    PtNnLayerDev L[PT_NN_LAYERS];
    char names[PT_NN_LAYERS][16] = {};
    DevBuf<uint8_t> d_scratch;
    size_t in_offset = 0;
    uint64_t macs = 0;                            // summed over the tiles
    DevBuf<float> d_scale;
    ptx_display *meter = nullptr;
    DevBuf<float> d_stage[4];                     // ptx_nn_denoise_host's rgb, albedo, normal, result (first use)
    ~ptx_nn();
};

// NULL when the parameters are usable, else what is wrong with them (the ptx_last_error message)
const char *pt_nn_params_problem(const ptx_nn_params &p, float samples);

// One denoise on `st`: rgb = W*H*3 floats on the handle's device, divided by `samples`; alb / nrm with a stride of 3 or 4 floats per
// pixel (the tracer's G-buffer records are float4), NULL exactly when the network does not take them (the caller has checked).  Makes
// st wait for the handle's last work, enqueues the meter on the whole frame where the scale is automatic, then for every tile in
// row-major order the input kernel on its window, the sixteen convolutions and the output kernel on the rectangle it keeps, records the
// handle's event.  The caller has checked p and set the device, and with more than one tile that out_rgb overlaps no input.
int pt_nn_enqueue(ptx_nn *n, hipStream_t st, const float *rgb, float samples, const float *alb, int alb_stride, const float *nrm, int nrm_stride,
                  const ptx_nn_params &p, float *out_rgb);
