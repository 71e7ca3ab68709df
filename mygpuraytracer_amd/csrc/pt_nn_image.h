// pt_nn_image.h -- host only, no hip* call: the arithmetic of the network denoiser's image descriptors (ptx_nn_image of
// include/mi355x_pathtracer.h, "images"; pt_nn_image.hip runs by it, tests/nn_image_check.cpp holds it under the sanitizers and
// tests/nn_image_ref.py restates it).  A descriptor with its defaults filled in is a view; a view has a byte interval; two intervals
// meet or do not.  All of it in size_t / uintptr_t: 16384 x 16384 pixels of 16 bytes are 2^32 bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "../../include/mi355x_pathtracer.h"

// bytes per channel; 0: no such format
inline size_t pt_nn_image_channel(int format) { return format == PTX_NN_FORMAT_FLOAT3 ? 4 : format == PTX_NN_FORMAT_HALF3 ? 2 : 0; }

struct PtNnImageView {
    uintptr_t base = 0;                       // of channel 0 of pixel (0, 0): ptr + byte_offset; 0: no image
    size_t pixel_stride = 0, row_stride = 0;  // bytes, the defaults filled in
    int format = 0;
    size_t channel() const { return pt_nn_image_channel(format); }
    uintptr_t at(size_t x, size_t y, size_t c) const { return base + y * row_stride + x * pixel_stride + c * channel(); }
};

// The view of a descriptor for a width x height frame, or what is refused of it ("" when nothing): the rules of the public header, in
// its order.  The caller has checked img.ptr and width, height >= 1.
inline std::string pt_nn_image_view(int width, int height, const ptx_nn_image &img, PtNnImageView &v) {
    (void)height;
    const size_t size = pt_nn_image_channel(img.format);
    if (!size) return "unknown format " + std::to_string(img.format) + " (PTX_NN_FORMAT_FLOAT3 = 1, PTX_NN_FORMAT_HALF3 = 2)";
    v.format = img.format;
    v.base = (uintptr_t)img.ptr + img.byte_offset;
    v.pixel_stride = img.pixel_stride ? img.pixel_stride : 3 * size;
    if (v.pixel_stride < 3 * size)
        return "a pixel stride of " + std::to_string(v.pixel_stride) + " bytes is below the pixel's size of " + std::to_string(3 * size);
    v.row_stride = img.row_stride ? img.row_stride : (size_t)width * v.pixel_stride;
    if (v.row_stride < (size_t)width * v.pixel_stride)
        return "a row stride of " + std::to_string(v.row_stride) + " bytes is below width * pixel stride = " + std::to_string((size_t)width * v.pixel_stride);
    if (v.row_stride % v.pixel_stride)
        return "a row stride of " + std::to_string(v.row_stride) + " bytes is not a multiple of the pixel stride of " + std::to_string(v.pixel_stride);
    const char *what = v.base % size ? "ptr + byte_offset" : v.pixel_stride % size ? "the pixel stride" : v.row_stride % size ? "the row stride" : nullptr;
    if (what) return std::string(what) + " is not a multiple of the channel size of " + std::to_string(size) + " bytes (the device needs aligned channels)";
    return "";
}

// [lo, hi): the first channel byte of pixel (0, 0) to the last channel byte of pixel (width - 1, height - 1), + 1
inline void pt_nn_image_interval(const PtNnImageView &v, int width, int height, uintptr_t &lo, uintptr_t &hi) {
    lo = v.base;
    hi = v.at((size_t)width - 1, (size_t)height - 1, 2) + v.channel();
}

// two intervals share a byte
inline bool pt_nn_intervals_meet(uintptr_t alo, uintptr_t ahi, uintptr_t blo, uintptr_t bhi) { return alo < bhi && blo < ahi; }
