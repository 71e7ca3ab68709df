// pt_adaptive.h -- internal interface between the adaptive-sampling handle (pt_adaptive.hip: its state, its kernels, create / reset /
// read) and the tracer (pt_post.hip: ptx_adaptive_add / _select / _resolve and ptx_denoise_adaptive, which need the tracer's
// accumulation buffer, stream and tile mask; the mask itself is set by pt_engine.hip).  Not part of the C ABI; include/mi355x_pathtracer.h has the public side and the definitions.
//
// State per tile of ptx_tile_pixels() pixels, tile = (y * W + x) / ptx_tile_pixels():
//   samples[tile] int32  iterations its pixels hold        batches[tile] int32  adds it took part in
//   active[tile]  uint8  1 = rendered under the mask       err[tile]     float  e_T of the last select (0: no estimate yet)
//   nest[tile]    int32  its pixels with B >= 2 at the last select (0: no estimate)
//   kt[tile]      float2 (k, W') of the last add, the table k_moments_add_tiled reads
// and one W*H*3 frame of mean radiance (ptx_adaptive_resolve).  d_status holds the last select's ptx_adaptive_status, h_status (pinned)
// the copy the host reads it from together with the flags: one transfer.
#pragma once
#include "pt_denoise.h"

struct ptx_adaptive : PtHandle {
    int ntiles = 0;
    DevBuf<int32_t> d_samples, d_batches, d_nest;
    DevBuf<float> d_err;
    DevBuf<float2> d_kt;
    DevBuf<uint8_t> d_out;                // [sizeof(ptx_adaptive_status) | active: ntiles bytes], contiguous for the one read
    uint8_t *h_out = nullptr;             // its pinned host copy
    DevBuf<float> d_frame;                // W*H*3
    std::vector<uint8_t> h_active;        // the flags as the last select left them (all 1 after create / reset)
    std::vector<int32_t> h_samples, h_k;  // the host's mirror of samples, and the last add's k per tile
    int rounds = 0;
    ~ptx_adaptive() { if (h_out) (void)hipHostFree(h_out); }
    uint8_t *d_active() const { return d_out + sizeof(ptx_adaptive_status); }
};

// The tracer's active-tile mask (ptx_set_active_tiles): keep[tile] = flags[tile] != 0, eff[tile] = keep[tile] ? base[tile] : 0 -- the
// table the camera bounce reads while a mask is set.  flags may be keep itself.
hipError_t pt_tile_mask_enqueue(hipStream_t st, int ntiles, const uint8_t *flags, uint8_t *keep, const uint32_t *base, uint32_t *eff);
const char *pt_adaptive_params_problem(const ptx_adaptive_params &p);
// Active tiles: samples += k, batches += 1, kt = (k, samples); the others: kt = (0, samples).
hipError_t pt_adaptive_advance_enqueue(hipStream_t st, const ptx_adaptive &a, int k);
// One workgroup per tile: e_T from the moments state, the decision into active, then one workgroup that reduces the status.
hipError_t pt_adaptive_select_enqueue(hipStream_t st, const ptx_adaptive &a, const PtMomentsState &s, const ptx_adaptive_params &p, int rounds);
// frame[p] = acc[p] / samples[tile(p)], 0 where the tile has no sample
hipError_t pt_adaptive_resolve_enqueue(hipStream_t st, const ptx_adaptive &a, const float *acc);
// pt_moments_prep_enqueue on a frame of unequal counts: c = float4(acc / s (demodulated on hit pixels), v) with s = samples[tile(p)] > 0
// on every tile, v = max(g^T C g, 0) / s on hit pixels with B >= min_batches (>= 2), -1 on the other hit pixels
// (pt_variance_spatial_enqueue fills those in), 0 on miss pixels; and frame[p] = acc[p] / s, the resolve.  Every tile with the same
// count: pt_moments_prep_enqueue's bits.
hipError_t pt_adaptive_prep_enqueue(hipStream_t st, const ptx_adaptive &a, const float *acc, const float4 *nh, const float4 *alb, int demod,
                                    const PtMomentsState &s, int min_batches, float4 *c);
