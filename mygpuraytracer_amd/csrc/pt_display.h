// pt_display.h -- internal interface of the display transform (pt_display.hip: ptx_display_* of include/mi355x_pathtracer.h) towards
// the tracer (pt_post.hip: ptx_display_tracer, which needs the tracer's accumulation buffer, denoised frame and stream).
// Not part of the C ABI; include/mi355x_pathtracer.h has the public side and the definition of the rule.
//
// Device state of a handle:
//   d_blocks[i * WK + j] = L_ij, the mean luminance of block (i, j) of the last metered frame (HK * WK floats)
//   d_begin              = where the blocks begin: i*H/HK for i = 0 .. HK, then j*W/WK for j = 0 .. WK (written once, at create)
//   d_state              = one PtDisplayState, written by k_display_meter alone and read by k_display_map, so that metering and
//                          mapping enqueue back to back and the host never waits for an exposure
//   d_codes              = W*H uchar4, the handle's own result buffer (used when the caller passes no buffer of its own)
//   d_float              = W*H*3 floats of z, allocated by the first call that asks for keep_float
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_denoise.h"

// what k_display_meter leaves on the device (ptx_display_status is read from it)
struct PtDisplayState {
    double log2_applied;                  // the adapted exposure's logarithm, carried in double from frame to frame
    float metered, applied, log2_mean;
    int32_t blocks_used, blocks_total;
    int32_t reserved;
    long long frames;                     // metered frames since create / reset
};

struct ptx_display : PtHandle {
    int hk = 0, wk = 0;                   // the block grid: (h + 8) / 16 x (w + 8) / 16
    DevBuf<float> d_blocks;
    DevBuf<int32_t> d_begin;              // hk + 1 row boundaries, then wk + 1 column boundaries
    DevBuf<PtDisplayState> d_state;
    DevBuf<uchar4> d_codes;
    DevBuf<float> d_float;                // first keep_float call
    DevBuf<float> d_stage;                // W*H*3: ptx_display_host's upload (first use)
    bool fresh = true;                    // the next metered frame is the first after create / reset: applied = metered
    bool metered = false;                 // d_blocks and d_state hold a frame's (since create / reset)
    bool codes_own = false;               // the last call's codes are in d_codes (else in the caller's buffer, or there was no call)
    bool float_valid = false;             // the last call stored z in d_float
};

// the block grid of a W x H frame (0 x 0 below 8 pixels either way), and where its rows and columns begin: hk + 1 / wk + 1 entries,
// NULLs allowed
inline void pt_display_grid(int w, int h, int *hk, int *wk) { *hk = (h + 8) / 16; *wk = (w + 8) / 16; }
void pt_display_begins(int w, int h, int hk, int wk, int32_t *row_begin, int32_t *col_begin);

// NULL when the parameters are usable, else what is wrong with them (the ptx_last_error message)
const char *pt_display_params_problem(const ptx_display_params &p, float samples);

// One display call on `st`: rgb = W*H*3 floats on the handle's device, divided by `samples`.  Makes st wait for the handle's last
// work, enqueues the meter (p.meter == PTX_METER_BLOCKS) and the map, records the handle's event.  Codes go to device_uchar4, or to
// the handle's own buffer when that is NULL.  The caller has checked p (pt_display_params_problem) and set the device.
int pt_display_enqueue(ptx_display *d, hipStream_t st, const float *rgb, float samples, const ptx_display_params &p, void *device_uchar4);

// The block meter alone on `st` (k_display_blocks, k_display_meter at adapt 1): d_state's `metered` is then this frame's.  For a handle
// that its caller owns and orders itself (pt_nn.hip's automatic scale): no wait, no event, none of the handle's flags.
int pt_display_meter_enqueue(ptx_display *d, hipStream_t st, const float *rgb, float samples, float key);
