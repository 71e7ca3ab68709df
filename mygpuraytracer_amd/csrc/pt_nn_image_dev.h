// pt_nn_image_dev.h -- what the units whose kernels read and write described images share (pt_nn_image.hip: the RT filter's images;
// pt_nn_lightmap.hip: the lightmap filter's): the view as a kernel sees it, its loads and stores, and the host functions of
// pt_nn_image.hip that both use -- the gather for the meter, the in-place copy-out, the staging of host images.  One text for both
// units; pt_nn_image.hip's code object is what it was with these lines in the unit itself.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_nn.h"
#include "pt_nn_image.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// a view on the device.  wide: loads a pixel at once (see pt_nn_image.hip); pair: half stores as 4 + 2 bytes
struct Img {
    uint8_t *base;                            // NULL: no image
    size_t ps, rs;
    int half, wide, pair;
};

__device__ __forceinline__ void load3(const Img &im, size_t x, size_t y, float v[3]) {
    const uint8_t *p = im.base + y * im.rs + x * im.ps;
    if (!im.half) {
        if (im.wide) {
            const float4 r = *reinterpret_cast<const float4 *>(p);
            v[0] = r.x; v[1] = r.y; v[2] = r.z;
        } else {
            const float *f = reinterpret_cast<const float *>(p);
            v[0] = f[0]; v[1] = f[1]; v[2] = f[2];
        }
    } else {
        if (im.wide) {
            const half4 r = *reinterpret_cast<const half4 *>(p);
            v[0] = (float)r[0]; v[1] = (float)r[1]; v[2] = (float)r[2];
        } else {
            const _Float16 *f = reinterpret_cast<const _Float16 *>(p);
            v[0] = (float)f[0]; v[1] = (float)f[1]; v[2] = (float)f[2];
        }
    }
}

__device__ __forceinline__ _Float16 to_half(float v) { return (_Float16)(v > 65504.f ? 65504.f : v); }

__device__ __forceinline__ void store3(const Img &im, size_t x, size_t y, const float v[3]) {
    uint8_t *p = im.base + y * im.rs + x * im.ps;
    if (!im.half) {
        float *f = reinterpret_cast<float *>(p);
        f[0] = v[0]; f[1] = v[1]; f[2] = v[2];
    } else if (im.pair) {
        half2v lo;
        lo[0] = to_half(v[0]); lo[1] = to_half(v[1]);
        *reinterpret_cast<half2v *>(p) = lo;
        reinterpret_cast<_Float16 *>(p)[2] = to_half(v[2]);
    } else {
        _Float16 *f = reinterpret_cast<_Float16 *>(p);
        f[0] = to_half(v[0]); f[1] = to_half(v[1]); f[2] = to_half(v[2]);
    }
}

inline Img device_image(const PtNnImageView &v) {
    Img im;
    im.base = reinterpret_cast<uint8_t *>(v.base);
    im.ps = v.pixel_stride; im.rs = v.row_stride;
    im.half = v.format == PTX_NN_FORMAT_HALF3;
    const size_t pixel = im.half ? 8 : 16;    // of four channels
    im.wide = v.base && v.pixel_stride == pixel && v.base % pixel == 0 && v.row_stride % pixel == 0;
    im.pair = im.half && v.base % 4 == 0 && v.pixel_stride % 4 == 0 && v.row_stride % 4 == 0;
    return im;
}

inline PtNnImageView packed_view(const float *p, int width) {
    PtNnImageView v;
    v.base = (uintptr_t)p; v.format = PTX_NN_FORMAT_FLOAT3; v.pixel_stride = 12; v.row_stride = 12 * (size_t)width;
    return v;
}

inline bool is_packed_float(const PtNnImageView &v, int width) {
    return v.format == PTX_NN_FORMAT_FLOAT3 && v.pixel_stride == 12 && v.row_stride == 12 * (size_t)width;
}

}  // namespace

// ---- pt_nn_image.hip's, for the other image unit -----------------------------------------------------------------------------------------
// k_nn_image_gather on st: the three channels of every pixel of `img` as floats into packed, W*H*3
int pt_nn_image_gather_enqueue(hipStream_t st, int w, int h, const PtNnImageView &img, float *packed);
// k_nn_image_copy on st: packed, W*H*3 floats, through `img`
int pt_nn_image_copy_enqueue(hipStream_t st, int w, int h, const float *packed, const PtNnImageView &img);
// The output's interval meets an input's and the handle has more than one tile: the tiles write the temporary (the public header, "in
// place").  The same for host views and for their staged copies, which meet the same way.
bool pt_nn_image_staged(const ptx_nn *n, const PtNnImageView v[4]);
// A *_host call on checked views of host memory: waits for the handle's last work, reports 0 to a progress monitor, stages the images'
// intervals up as ptx_nn_denoise_images_host describes, runs enqueue(ctx, n, the device views) on the default stream, waits, and
// brings the output's interval back -- or, where enqueue does not return PTX_OK, nothing.  The device is set.
int pt_nn_image_host_call(const char *fn, ptx_nn *n, const PtNnImageView v[4], int (*enqueue)(void *ctx, ptx_nn *n, const PtNnImageView d[4]), void *ctx);
