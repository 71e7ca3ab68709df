// pt_metrics.h -- the image metrics' host side (ptx_metrics_* of include/mi355x_pathtracer.h, "image metrics"; pt_metrics.hip runs by
// it).  First the arithmetic that needs no device and calls no hip* function: the scale geometry of the MS-SSIM pyramid, the window
// taps, the constants of the tone curve and the buffer sizes (pt_metrics_plan; tests/metrics_plan_check.cpp holds it under the
// sanitizers, ptx_debug_metrics_plan hands it out).  Then the handle.  Not part of the C ABI.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mi355x_pathtracer.h"

constexpr int PT_METRICS_MAX_SIDE = 16384;
constexpr int PT_METRICS_WIN = PTX_METRICS_TAPS, PT_METRICS_APRON = PT_METRICS_WIN - 1;
constexpr int PT_METRICS_TW = 32, PT_METRICS_TH = 16;       // k_metrics_ssim's output tile
constexpr int PT_METRICS_NT = 256;                          // every kernel's workgroup
// what one call reduces: a sum (or, MAXERR, a maximum) of doubles per job.  A job's partials are consecutive.
enum { PT_METRICS_JOB_SE = 0, PT_METRICS_JOB_AE, PT_METRICS_JOB_MAPE, PT_METRICS_JOB_SMAPE, PT_METRICS_JOB_NFA, PT_METRICS_JOB_NFB,
       PT_METRICS_JOB_NERR, PT_METRICS_JOB_MAXERR, PT_METRICS_JOB_GRAD, PT_METRICS_JOB_SSIM, /* + channel: l cs at full resolution */
       PT_METRICS_JOB_MCS = PT_METRICS_JOB_SSIM + 3, /* + 3 * scale + channel: MS-SSIM's five (none without it) */
       PT_METRICS_JOBS = PT_METRICS_JOB_MCS + 3 * PTX_METRICS_SCALES };
constexpr int PT_METRICS_POINT_JOBS = PT_METRICS_JOB_MAXERR + 1;

// The window of training/ssim.py as torch forms it in float32 -- exp(-k^2 / 4.5) for k = -5 .. 5 over its sum -- tabulated to the bit
// (tests/test_metrics_cpu.py forms it again with torch): ssim.py widens these very floats when it runs in double, so a float64
// restatement agrees with it only on them, and numpy's float32 sum of the same eleven terms already differs in the last place.
constexpr float PT_METRICS_TAPS_F[PT_METRICS_WIN] = {0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                                     0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f};
constexpr float PT_METRICS_WEIGHTS_F[PTX_METRICS_SCALES] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};

// The tone curve's constants (training/color.py:181-194), each formed in double as Python forms it and rounded once
struct PtMetricsTone {
    float a, b, cb, de, df, ef, scale, inv_white_div;      // inv_white_div: e(11.2), the divisor
};
inline PtMetricsTone pt_metrics_tone() {
    const double A = 0.22, B = 0.30, C = 0.10, D = 0.20, E = 0.01, F = 0.30, W = 11.2;
    PtMetricsTone t;
    t.a = (float)A; t.b = (float)B; t.cb = (float)(C * B); t.de = (float)(D * E); t.df = (float)(D * F); t.ef = (float)(E / F);
    t.scale = (float)1.758141;
    t.inv_white_div = (float)(((W * (A * W + C * B) + D * E) / (W * (A * W + B) + D * F)) - E / F);
    return t;
}
inline float pt_metrics_c1() { return (float)((0.01 * 1.0) * (0.01 * 1.0)); }
inline float pt_metrics_c2() { return (float)((0.03 * 1.0) * (0.03 * 1.0)); }

// avg_pool2d(kernel 2, padding n % 2): floor((n + 2 p - 2) / 2) + 1
inline int pt_metrics_pooled(int n) { const int p = n % 2; return (n + 2 * p - 2) / 2 + 1; }

inline size_t pt_metrics_ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// false: no such frame (a side below 1 or above PT_METRICS_MAX_SIDE)
inline bool pt_metrics_plan(int w, int h, ptx_metrics_plan *out) {
    if (w < 1 || h < 1 || w > PT_METRICS_MAX_SIDE || h > PT_METRICS_MAX_SIDE || !out) return false;
    ptx_metrics_plan p = ptx_metrics_plan();
    const int smaller = w < h ? w : h;
    p.ssim_valid = smaller >= PT_METRICS_WIN;
    p.msssim_valid = smaller > PT_METRICS_APRON * 16;
    p.scales = p.msssim_valid ? PTX_METRICS_SCALES : 1;
    p.tile_w = PT_METRICS_TW; p.tile_h = PT_METRICS_TH;
    size_t floats = 0, partials = 0;
    for (int s = 0; s < PTX_METRICS_SCALES; s++) {
        p.w[s] = s ? pt_metrics_pooled(p.w[s - 1]) : w;
        p.h[s] = s ? pt_metrics_pooled(p.h[s - 1]) : h;
        p.level_offset[s] = floats;
        if (s < p.scales) floats += 3 * (size_t)p.w[s] * (size_t)p.h[s];
        const bool runs = s < p.scales && p.ssim_valid && p.w[s] >= PT_METRICS_WIN && p.h[s] >= PT_METRICS_WIN;
        p.blocks[s] = runs ? (int)(pt_metrics_ceil_div((size_t)p.w[s] - PT_METRICS_APRON, PT_METRICS_TW) *
                                   pt_metrics_ceil_div((size_t)p.h[s] - PT_METRICS_APRON, PT_METRICS_TH)) : 0;
        partials += 3 * (size_t)p.blocks[s] * (p.msssim_valid ? (s == 0 ? 2 : 1) : 1);
    }
    p.pyramid_floats = floats;
    p.prep_blocks = (int)pt_metrics_ceil_div((size_t)w * (size_t)h, PT_METRICS_NT);
    p.grad_blocks = w >= 2 && h >= 2 ? (int)pt_metrics_ceil_div(((size_t)w - 1) * ((size_t)h - 1), PT_METRICS_NT) : 0;
    p.partial_doubles = partials + (size_t)PT_METRICS_POINT_JOBS * (size_t)p.prep_blocks + (size_t)p.grad_blocks;
    p.map_floats = p.ssim_valid ? ((size_t)w - PT_METRICS_APRON) * ((size_t)h - PT_METRICS_APRON) : 0;
    for (int k = 0; k < PT_METRICS_WIN; k++) p.taps[k] = PT_METRICS_TAPS_F[k];
    for (int s = 0; s < PTX_METRICS_SCALES; s++) p.weights[s] = PT_METRICS_WEIGHTS_F[s];
    *out = p;
    return true;
}

// where each job's partials begin and how many it has: prep's eight, grad, full-resolution SSIM by channel, then scale by scale and
// channel by channel
inline void pt_metrics_jobs(const ptx_metrics_plan &p, size_t off[PT_METRICS_JOBS], unsigned cnt[PT_METRICS_JOBS]) {
    size_t at = 0;
    for (int j = 0; j < PT_METRICS_JOBS; j++) {
        const int s = j >= PT_METRICS_JOB_MCS ? (j - PT_METRICS_JOB_MCS) / 3 : 0;
        cnt[j] = j < PT_METRICS_POINT_JOBS ? (unsigned)p.prep_blocks : j == PT_METRICS_JOB_GRAD ? (unsigned)p.grad_blocks :
                 j < PT_METRICS_JOB_MCS ? (unsigned)p.blocks[0] : p.msssim_valid ? (unsigned)p.blocks[s] : 0u;
        off[j] = at;
        at += cnt[j];
    }
}

// NULL when the parameters are usable, else what is wrong with them
inline const char *pt_metrics_params_problem(const ptx_metrics_params &p) {
    if (p.transform < PTX_METRICS_NONE || p.transform > PTX_METRICS_SNORM)
        return "ptx_metrics_params.transform must be PTX_METRICS_NONE, _SRGB, _HDR or _SNORM";
    if (!isnan(p.exposure) && (!(p.exposure > 0.f) || isinf(p.exposure))) return "ptx_metrics_params.exposure must be finite and positive, or NaN (metered on b)";
    if (!(p.threshold >= 0.f) || isinf(p.threshold)) return "ptx_metrics_params.threshold must be finite and >= 0";
    if (!(p.samples_a > 0.f) || isinf(p.samples_a) || !(p.samples_b > 0.f) || isinf(p.samples_b))
        return "ptx_metrics_params.samples_a and samples_b must be finite and positive";
    if (p.pointwise_only != 0 && p.pointwise_only != 1) return "ptx_metrics_params.pointwise_only must be 0 or 1";
    return nullptr;
}

// ---- the handle (pt_metrics.hip; pt_post.hip's ptx_metrics_tracer) ---------------------------------------------------------------------
#include "pt_handle.h"
#include "pt_nn_image.h"

struct ptx_display;

struct ptx_metrics : PtHandle {
    ptx_metrics_plan plan = ptx_metrics_plan();
    DevBuf<float> d_x, d_y;               // the planar pyramids of t(a) and t(b): [level][channel][y][x]
    DevBuf<double> d_part;                // plan.partial_doubles
    DevBuf<double> d_res;                 // PT_METRICS_JOBS sums, then the exposure used
    DevBuf<float> d_map;                  // the host call's map (first need)
    DevBuf<float> d_gather;               // b as packed floats for the meter (first need)
    DevBuf<uint8_t> d_stage[2];           // the host calls' staged intervals of a and b (grown on need)
    ptx_display *meter = nullptr;         // the automatic exposure's block meter (first need); ordered by this handle
    ~ptx_metrics();
};

// One comparison on st of checked views on the handle's device, the device set: waits for the handle's last work, enqueues, records
// the handle's event, waits for it and fills *out (as far as out->struct_size).  d_map: NULL, or the map on the device.
int pt_metrics_compare(ptx_metrics *m, hipStream_t st, const PtNnImageView &a, const PtNnImageView &b, const ptx_metrics_params &p,
                       ptx_metrics_result *out, float *d_map);
// A checked view of host memory -> its interval staged in d_stage[which], the view on the device in *dev.  Waits for the handle first.
int pt_metrics_stage(ptx_metrics *m, int which, const PtNnImageView &host, PtNnImageView *dev);
// What the compare calls refuse without a device, in order: the params, out, NULL images, unknown formats, each descriptor.  va, vb:
// the views (a NULL `a` is skipped when a_given is false: ptx_metrics_tracer brings its own).
int pt_metrics_problem(const char *fn, int w, int h, const ptx_nn_image *a, bool a_given, const ptx_nn_image *b, const ptx_metrics_params &p,
                       PtNnImageView *va, PtNnImageView *vb);
