// pt_metrics.hip -- image metrics on the device (ptx_metrics_* of include/mi355x_pathtracer.h, "image metrics"): two described images
// -> MSE / PSNR / L1 / MAPE / SMAPE / gradient, compareImage's count and maximum, SSIM and MS-SSIM, in one call.  The rule is defined in
// the public header and restated by tests/metrics_ref.py; geometry, taps, constants and buffer sizes are pt_metrics.h's.
// ptx_metrics_tracer is pt_post.hip's: it needs the tracer's buffers and stream.
//
// Kernels (fp32 terms, one IEEE operation per step: -ffp-contract=off; fp64 sums; a workgroup of 256 everywhere; no atomics, no scratch):
//   k_metrics_prep   : one thread per pixel.  Both images through their descriptors (pt_nn_image_dev.h), the divisor, the sanitiser,
//       compareImage on the sanitised values, the transform, the planar level 0 of both pyramids (three coalesced 4-byte stores each), the
//       four pointwise terms.  A thread adds its three channels in double, a wave its lanes by shuffles of fixed shape, thread 0 the four
//       waves from LDS in wave order: eight partials per workgroup (four sums, three counts held as doubles, one maximum).
//   k_metrics_grad   : one thread per pixel (i, j) of the (H - 1) x (W - 1) interior corner grid, six terms from level 0; one partial.
//   k_metrics_pool   : avg_pool2d(2, padding n % 2) of the three planes of both pyramids' level s - 1 into level s: (((a + b) + c) + d) * 0.25f
//       with zeros outside, one thread per output.
//   k_metrics_ssim<CS, FULL> : the hot one.  A workgroup owns a 32 x 16 tile of the map.  Channel by channel it stages the tile plus its
//       10-pixel apron of X and Y in LDS (42 x 26 floats each, zeros beyond the image), filters x, y, xx, yy, xy along x into 26 x 32 x 5
//       floats of LDS (thread = one row position, eleven taps left to right), then along y (thread = two map pixels), forms cs and l cs and
//       adds them in double: one partial per channel for cs (CS: scales 0 .. 3 of MS-SSIM) and / or for l cs (FULL: SSIM at full
//       resolution, MS-SSIM's last scale).  25.4 KiB of LDS.  The map, where asked for, is ((v0 + v1) + v2) / 3 of the channels' l cs.
//   k_metrics_finish : one workgroup per job (pt_metrics.h): thread t adds partials t, t + 256, ... in that order, then a tree of fixed
//       shape in LDS; the maximum likewise.  Thread 0 stores the job's double.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <limits>
#include <string>

#include "pt_metrics.h"
#include "pt_nn_image_dev.h"
#include "pt_nn_transfer.h"
#include "pt_display.h"

namespace {

constexpr int NT = PT_METRICS_NT, WAVE = 64, NWAVES = NT / WAVE;
constexpr int TW = PT_METRICS_TW, TH = PT_METRICS_TH, WIN = PT_METRICS_WIN, APRON = PT_METRICS_APRON;
constexpr int AW = TW + APRON, AH = TH + APRON;
constexpr float X_CAP = 0x1p60f;          // the tone curve's argument is held to +-2^60 (the public header)

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = WAVE / 2; off > 0; off >>= 1) v = v + __shfl_down(v, off, WAVE);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int off = WAVE / 2; off > 0; off >>= 1) { const double o = __shfl_down(v, off, WAVE); v = v < o ? o : v; }
    return v;
}

__device__ __forceinline__ bool nonfinite(float r) { return r != r || fabsf(r) > FLT_MAX; }
// np.nan_to_num of r / samples
__device__ __forceinline__ float sanitise(float r, float samples) {
    const float s = r / samples;
    return s != s ? 0.f : s > FLT_MAX ? FLT_MAX : s < -FLT_MAX ? -FLT_MAX : s;
}

__device__ __forceinline__ float hable(float v, const PtMetricsTone &t) {
    return ((v * (t.a * v + t.cb) + t.de) / (v * (t.a * v + t.b) + t.df)) - t.ef;
}

// (the last step: 12.92 * -FLT_MAX, or the curve at one of its two poles below 0, would be an infinity, and two of them a NaN in every sum)
__device__ __forceinline__ float held(float t) { return t > FLT_MAX ? FLT_MAX : t < -FLT_MAX ? -FLT_MAX : t; }

__device__ __forceinline__ float transform(float s, int mode, float exposure, const PtMetricsTone &t) {
    if (mode == PTX_METRICS_NONE) return s;
    if (mode == PTX_METRICS_SNORM) return s * 0.5f + 0.5f;
    if (mode == PTX_METRICS_HDR) {
        float v = (s * exposure) * t.scale;
        v = v > X_CAP ? X_CAP : v < -X_CAP ? -X_CAP : v;
        s = fminf(hable(v, t) / t.inv_white_div, 1.f);
    }
    return held(pt_nn_transfer::transfer_forward(s, pt_nn_transfer::MODE_SRGB, 1.f));
}

struct PrepArgs {
    Img a, b;
    int w, h;
    float samples_a, samples_b;
    int mode;
    float exposure;
    const float *exposure_ptr;            // NULL: `exposure`
    float threshold;
    PtMetricsTone tone;
    float *x0, *y0;                       // level 0, planar
    double *part;                         // eight jobs of nblk partials each
    unsigned nblk;
    double *exposure_out;
};

__global__ __launch_bounds__(NT) void k_metrics_prep(PrepArgs a) {
    __shared__ double s_w[PT_METRICS_POINT_JOBS][NWAVES];
    const int tid = threadIdx.x;
    const size_t n = (size_t)a.w * a.h, p = (size_t)blockIdx.x * NT + tid;
    const float E = a.exposure_ptr ? *a.exposure_ptr : a.exposure;
    if (p == 0) *a.exposure_out = (double)E;
    double v[PT_METRICS_POINT_JOBS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < n) {
        const size_t y = p / a.w, x = p - y * a.w;
        float ra[3], rb[3];
        load3(a.a, x, y, ra);
        load3(a.b, x, y, rb);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float sa = sanitise(ra[c], a.samples_a), sb = sanitise(rb[c], a.samples_b);
            // compareImage (apps/utils/image_io.cpp:449-455), std::min and std::max as written there
            float err = fabsf(sb - sa);
            if (sb != 0.f) { const float rel = err / sb; err = rel < err ? rel : err; }
            const double e = (double)err;
            v[PT_METRICS_JOB_MAXERR] = v[PT_METRICS_JOB_MAXERR] < e ? e : v[PT_METRICS_JOB_MAXERR];
            v[PT_METRICS_JOB_NERR] += err > a.threshold ? 1.0 : 0.0;
            v[PT_METRICS_JOB_NFA] += nonfinite(ra[c]) ? 1.0 : 0.0;
            v[PT_METRICS_JOB_NFB] += nonfinite(rb[c]) ? 1.0 : 0.0;
            const float ta = transform(sa, a.mode, E, a.tone), tb = transform(sb, a.mode, E, a.tone);
            a.x0[(size_t)c * n + p] = ta;
            a.y0[(size_t)c * n + p] = tb;
            const float d = ta - tb, ad = fabsf(d);
            v[PT_METRICS_JOB_SE] = v[PT_METRICS_JOB_SE] + (double)(d * d);
            v[PT_METRICS_JOB_AE] = v[PT_METRICS_JOB_AE] + (double)ad;
            v[PT_METRICS_JOB_MAPE] = v[PT_METRICS_JOB_MAPE] + (double)(ad / (fabsf(tb) + 0.01f));
            v[PT_METRICS_JOB_SMAPE] = v[PT_METRICS_JOB_SMAPE] + (double)(ad / ((fabsf(ta) + fabsf(tb)) + 0.01f));
        }
    }
#pragma unroll
    for (int j = 0; j < PT_METRICS_POINT_JOBS; j++) {
        const double r = j == PT_METRICS_JOB_MAXERR ? wave_max(v[j]) : wave_sum(v[j]);
        if ((tid & (WAVE - 1)) == 0) s_w[j][tid / WAVE] = r;
    }
    __syncthreads();
    if (tid < PT_METRICS_POINT_JOBS) {
        const double *w = s_w[tid];
        double r;
        if (tid == PT_METRICS_JOB_MAXERR) { r = w[0]; for (int k = 1; k < NWAVES; k++) r = r < w[k] ? w[k] : r; }
        else r = ((w[0] + w[1]) + w[2]) + w[3];
        a.part[(size_t)tid * a.nblk + blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(NT) void k_metrics_grad(int w, int h, const float *__restrict__ x0, const float *__restrict__ y0, double *__restrict__ part) {
    __shared__ double s_w[NWAVES];
    const int tid = threadIdx.x;
    const size_t gw = (size_t)w - 1, n = gw * ((size_t)h - 1), p = (size_t)blockIdx.x * NT + tid, plane = (size_t)w * h;
    double v = 0.0;
    if (p < n) {
        const size_t i = p / gw, j = p - i * gw, at = i * w + j;
        for (int c = 0; c < 3; c++) {
            const float *X = x0 + c * plane + at, *Y = y0 + c * plane + at;
            const float dy = (X[w] - X[0]) - (Y[w] - Y[0]), dx = (X[1] - X[0]) - (Y[1] - Y[0]);
            v = v + (double)fabsf(dy);
            v = v + (double)fabsf(dx);
        }
    }
    v = wave_sum(v);
    if ((tid & (WAVE - 1)) == 0) s_w[tid / WAVE] = v;
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// blockIdx.y: 0 = X's pyramid, 1 = Y's
__global__ __launch_bounds__(NT) void k_metrics_pool(int ws, int hs, int wd, int hd, const float *__restrict__ xs, float *__restrict__ xd,
                                                     const float *__restrict__ ys, float *__restrict__ yd) {
    const float *src = blockIdx.y ? ys : xs;
    float *dst = blockIdx.y ? yd : xd;
    const size_t pd = (size_t)wd * hd, idx = (size_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= 3 * pd) return;
    const size_t c = idx / pd, r = idx - c * pd, i = r / wd, j = r - i * wd;
    const long long y0 = 2 * (long long)i - hs % 2, x0 = 2 * (long long)j - ws % 2;
    const float *plane = src + c * (size_t)ws * hs;
    float q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long y = y0 + (k >> 1), x = x0 + (k & 1);
        q[k] = y >= 0 && y < hs && x >= 0 && x < ws ? plane[(size_t)y * ws + (size_t)x] : 0.f;
    }
    dst[idx] = (((q[0] + q[1]) + q[2]) + q[3]) * 0.25f;
}

struct SsimArgs {
    const float *x, *y;                   // one level, planar
    int w, h;
    float c1, c2;
    float taps[WIN];
    double *part_cs, *part_full;          // three jobs of nblk partials each
    unsigned nblk;
    float *map;                           // NULL: none
};

template <bool CS, bool FULL>
__global__ __launch_bounds__(NT) void k_metrics_ssim(SsimArgs a) {
    __shared__ float s_x[AH][AW], s_y[AH][AW];
    __shared__ float s_f[5][AH][TW];
    __shared__ double s_w[2][NWAVES];
    const int tid = threadIdx.x, lx = tid % TW, ly = tid / TW;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int mw = a.w - APRON, mh = a.h - APRON;
    const unsigned blk = blockIdx.y * gridDim.x + blockIdx.x;
    const size_t plane = (size_t)a.w * a.h;
    float mapv[2] = {0.f, 0.f};
    for (int c = 0; c < 3; c++) {
        const float *px = a.x + c * plane, *py = a.y + c * plane;
        for (int i = tid; i < AH * AW; i += NT) {
            const int r = i / AW, q = i - r * AW, gy = ty0 + r, gx = tx0 + q;
            const bool in = gy < a.h && gx < a.w;
            s_x[r][q] = in ? px[(size_t)gy * a.w + gx] : 0.f;
            s_y[r][q] = in ? py[(size_t)gy * a.w + gx] : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < AH * TW; i += NT) {
            const int r = i / TW, q = i - r * TW;
            float fx = 0.f, fy = 0.f, fxx = 0.f, fyy = 0.f, fxy = 0.f;
#pragma unroll
            for (int k = 0; k < WIN; k++) {
                const float x = s_x[r][q + k], y = s_y[r][q + k], t = a.taps[k];
                fx = fx + t * x; fy = fy + t * y;
                fxx = fxx + t * (x * x); fyy = fyy + t * (y * y); fxy = fxy + t * (x * y);
            }
            s_f[0][r][q] = fx; s_f[1][r][q] = fy; s_f[2][r][q] = fxx; s_f[3][r][q] = fyy; s_f[4][r][q] = fxy;
        }
        __syncthreads();
        double dcs = 0.0, dfull = 0.0;
#pragma unroll
        for (int o = 0; o < 2; o++) {
            const int oy = ly + o * (TH / 2);
            float m1 = 0.f, m2 = 0.f, fxx = 0.f, fyy = 0.f, fxy = 0.f;
#pragma unroll
            for (int k = 0; k < WIN; k++) {
                const float t = a.taps[k];
                m1 = m1 + t * s_f[0][oy + k][lx]; m2 = m2 + t * s_f[1][oy + k][lx];
                fxx = fxx + t * s_f[2][oy + k][lx]; fyy = fyy + t * s_f[3][oy + k][lx]; fxy = fxy + t * s_f[4][oy + k][lx];
            }
            const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
            const float s1 = fxx - m11, s2 = fyy - m22, s12 = fxy - m12;
            const float cs = (2.f * s12 + a.c2) / ((s1 + s2) + a.c2);
            const float full = ((2.f * m12 + a.c1) / ((m11 + m22) + a.c1)) * cs;
            if (tx0 + lx < mw && ty0 + oy < mh) {
                if (CS) dcs = dcs + (double)cs;
                if (FULL) { dfull = dfull + (double)full; mapv[o] = c ? mapv[o] + full : full; }
            }
        }
        if (CS) { dcs = wave_sum(dcs); if ((tid & (WAVE - 1)) == 0) s_w[0][tid / WAVE] = dcs; }
        if (FULL) { dfull = wave_sum(dfull); if ((tid & (WAVE - 1)) == 0) s_w[1][tid / WAVE] = dfull; }
        __syncthreads();                   // also: every read of s_x, s_y, s_f precedes the next channel's staging
        if (tid == 0) {
            if (CS) a.part_cs[(size_t)c * a.nblk + blk] = ((s_w[0][0] + s_w[0][1]) + s_w[0][2]) + s_w[0][3];
            if (FULL) a.part_full[(size_t)c * a.nblk + blk] = ((s_w[1][0] + s_w[1][1]) + s_w[1][2]) + s_w[1][3];
        }
        __syncthreads();                   // s_w is read before the next channel writes it
    }
    if (FULL && a.map) {
#pragma unroll
        for (int o = 0; o < 2; o++) {
            const int ox = tx0 + lx, oy = ty0 + ly + o * (TH / 2);
            if (ox < mw && oy < mh) a.map[(size_t)oy * mw + ox] = mapv[o] / 3.f;
        }
    }
}

struct FinishArgs {
    unsigned long long off[PT_METRICS_JOBS];
    unsigned cnt[PT_METRICS_JOBS];
};

__global__ __launch_bounds__(NT) void k_metrics_finish(FinishArgs a, const double *__restrict__ part, double *__restrict__ res) {
    __shared__ double s[NT];
    const int tid = threadIdx.x, j = blockIdx.x;
    const bool is_max = j == PT_METRICS_JOB_MAXERR;
    const double *p = part + a.off[j];
    double v = 0.0;
    for (unsigned k = tid; k < a.cnt[j]; k += NT) { const double q = p[k]; v = is_max ? (v < q ? q : v) : v + q; }
    s[tid] = v;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) { const double q = s[tid + h]; s[tid] = is_max ? (s[tid] < q ? q : s[tid]) : s[tid] + q; }
        __syncthreads();
    }
    if (tid == 0) res[j] = s[0];
}

int alloc_metrics(ptx_metrics *m) {
    if (!pt_metrics_plan(m->w, m->h, &m->plan)) return pt_fail(PTX_ERR_INVALID, "ptx_metrics_create: bad frame size");
    PT_HC(hipSetDevice(m->device));
    PT_HC(m->d_x.alloc(m->plan.pyramid_floats));
    PT_HC(m->d_y.alloc(m->plan.pyramid_floats));
    PT_HC(m->d_part.alloc(m->plan.partial_doubles));
    PT_HC(m->d_res.alloc(PT_METRICS_JOBS + 1));
    PT_HC(m->ev.create(hipEventDisableTiming));
    return PTX_OK;
}

template <class T> hipError_t grow(DevBuf<T> &b, size_t count) {
    if (b.p && b.n >= count) return hipSuccess;
    if (b.p) { const hipError_t e = hipFree(b.p); b.p = nullptr; b.n = 0; if (e != hipSuccess) return e; }
    return b.alloc(count);
}

template <bool CS, bool FULL> void launch_ssim(hipStream_t st, const ptx_metrics_plan &pl, int s, const SsimArgs &a) {
    const dim3 grid((unsigned)pt_metrics_ceil_div((size_t)pl.w[s] - APRON, TW), (unsigned)pt_metrics_ceil_div((size_t)pl.h[s] - APRON, TH));
    hipLaunchKernelGGL((k_metrics_ssim<CS, FULL>), grid, dim3(NT), 0, st, a);
}

bool given(const ptx_nn_image *img) { return img && img->ptr; }

const double NaN = std::numeric_limits<double>::quiet_NaN();

}  // namespace

ptx_metrics::~ptx_metrics() { ptx_display_destroy(meter); }

int pt_metrics_problem(const char *fn_, int w, int h, const ptx_nn_image *a, bool a_given, const ptx_nn_image *b, const ptx_metrics_params &p,
                       PtNnImageView *va, PtNnImageView *vb) {
    const std::string fn = fn_;
    if (const char *why = pt_metrics_params_problem(p)) return pt_fail(PTX_ERR_INVALID, fn + ": " + why);
    const ptx_nn_image *const img[2] = {a, b};
    PtNnImageView *const v[2] = {va, vb};
    const char *const name[2] = {"a (the test image)", "b (the reference image)"};
    for (int k = a_given ? 0 : 1; k < 2; k++)
        if (!given(img[k])) return pt_fail(PTX_ERR_INVALID, fn + ": image " + name[k] + " is NULL");
    if (w < 1 || h < 1 || w > PT_METRICS_MAX_SIDE || h > PT_METRICS_MAX_SIDE) return pt_fail(PTX_ERR_INVALID, fn + ": bad frame size");
    for (int k = a_given ? 0 : 1; k < 2; k++) {
        const std::string why = pt_nn_image_view(w, h, *img[k], *v[k]);
        if (!why.empty()) return pt_fail(PTX_ERR_INVALID, fn + ": image " + name[k] + ": " + why);
    }
    return PTX_OK;
}

int pt_metrics_stage(ptx_metrics *m, int which, const PtNnImageView &host, PtNnImageView *dev) {
    uintptr_t lo, hi;
    pt_nn_image_interval(host, m->w, m->h, lo, hi);
    const size_t lead = lo % 16;                          // the interval keeps its place on the 16-byte grid: the same loads either side
    PT_HC(m->wait_host());
    PT_HC(grow(m->d_stage[which], lead + (size_t)(hi - lo)));
    PT_HC(hipMemcpy(m->d_stage[which].p + lead, reinterpret_cast<const void *>(lo), (size_t)(hi - lo), hipMemcpyHostToDevice));
    *dev = host;
    dev->base = (uintptr_t)(m->d_stage[which].p + lead) + (host.base - lo);
    return PTX_OK;
}

int pt_metrics_compare(ptx_metrics *m, hipStream_t st, const PtNnImageView &va, const PtNnImageView &vb, const ptx_metrics_params &p,
                       ptx_metrics_result *out, float *d_map) {
    const ptx_metrics_plan &pl = m->plan;
    const bool with_ssim = pl.ssim_valid && !p.pointwise_only, with_msssim = pl.msssim_valid && !p.pointwise_only;
    const bool automatic = p.transform == PTX_METRICS_HDR && isnan(p.exposure);
    if (automatic && !m->meter)
        if (const int rc = ptx_display_create(m->device, m->w, m->h, &m->meter)) return rc;
    const bool gather = automatic && !is_packed_float(vb, m->w);
    PT_HC(m->wait_stream(st));
    if (gather && !m->d_gather) PT_HC(m->d_gather.alloc(3 * (size_t)m->w * m->h));

    size_t off[PT_METRICS_JOBS];
    FinishArgs fa;
    pt_metrics_jobs(pl, off, fa.cnt);
    for (int j = 0; j < PT_METRICS_JOBS; j++) fa.off[j] = off[j];

    PrepArgs pa;
    pa.a = device_image(va); pa.b = device_image(vb);
    pa.w = m->w; pa.h = m->h;
    pa.samples_a = p.samples_a; pa.samples_b = p.samples_b;
    pa.mode = p.transform;
    pa.exposure = p.transform == PTX_METRICS_HDR ? p.exposure : 1.f;
    pa.exposure_ptr = nullptr;
    if (automatic) {
        const float *rgb = reinterpret_cast<const float *>(vb.base);
        if (gather) {
            if (const int rc = pt_nn_image_gather_enqueue(st, m->w, m->h, vb, m->d_gather)) return rc;
            rgb = m->d_gather;
        }
        if (const int rc = pt_display_meter_enqueue(m->meter, st, rgb, p.samples_b, 0.18f)) return rc;
        pa.exposure_ptr = &m->meter->d_state.p->metered;
    }
    pa.threshold = p.threshold;
    pa.tone = pt_metrics_tone();
    pa.x0 = m->d_x; pa.y0 = m->d_y;
    pa.part = m->d_part.p + off[0];
    pa.nblk = (unsigned)pl.prep_blocks;
    pa.exposure_out = m->d_res.p + PT_METRICS_JOBS;
    hipLaunchKernelGGL(k_metrics_prep, dim3((unsigned)pl.prep_blocks), dim3(NT), 0, st, pa);
    PT_HC(hipGetLastError());
    if (pl.grad_blocks) {
        hipLaunchKernelGGL(k_metrics_grad, dim3((unsigned)pl.grad_blocks), dim3(NT), 0, st, m->w, m->h, (const float *)m->d_x, (const float *)m->d_y,
                           m->d_part.p + off[PT_METRICS_JOB_GRAD]);
        PT_HC(hipGetLastError());
    }
    for (int s = 0; s < pl.scales && with_ssim; s++) {
        float *xs = m->d_x.p + pl.level_offset[s], *ys = m->d_y.p + pl.level_offset[s];
        if (s) {
            const size_t n = 3 * (size_t)pl.w[s] * pl.h[s];
            hipLaunchKernelGGL(k_metrics_pool, dim3((unsigned)pt_metrics_ceil_div(n, NT), 2), dim3(NT), 0, st, pl.w[s - 1], pl.h[s - 1], pl.w[s], pl.h[s],
                               (const float *)(m->d_x.p + pl.level_offset[s - 1]), xs, (const float *)(m->d_y.p + pl.level_offset[s - 1]), ys);
            PT_HC(hipGetLastError());
        }
        SsimArgs sa;
        sa.x = xs; sa.y = ys; sa.w = pl.w[s]; sa.h = pl.h[s];
        sa.c1 = pt_metrics_c1(); sa.c2 = pt_metrics_c2();
        for (int k = 0; k < WIN; k++) sa.taps[k] = pl.taps[k];
        sa.nblk = (unsigned)pl.blocks[s];
        sa.map = s == 0 ? d_map : nullptr;
        sa.part_cs = sa.part_full = m->d_part.p + off[PT_METRICS_JOB_MCS + 3 * s];
        if (s == 0) sa.part_full = m->d_part.p + off[PT_METRICS_JOB_SSIM];
        if (!pl.msssim_valid) launch_ssim<false, true>(st, pl, s, sa);                 // SSIM alone
        else if (s == 0) launch_ssim<true, true>(st, pl, s, sa);                       // MS-SSIM's first scale and SSIM
        else if (s < PTX_METRICS_SCALES - 1) launch_ssim<true, false>(st, pl, s, sa);
        else launch_ssim<false, true>(st, pl, s, sa);
        PT_HC(hipGetLastError());
    }
    hipLaunchKernelGGL(k_metrics_finish, dim3(PT_METRICS_JOBS), dim3(NT), 0, st, fa, (const double *)m->d_part, m->d_res.p);
    PT_HC(hipGetLastError());
    PT_HC(m->record(st));
    PT_HC(hipEventSynchronize(m->ev));
    double r[PT_METRICS_JOBS + 1];
    PT_HC(hipMemcpy(r, m->d_res, sizeof r, hipMemcpyDeviceToHost));

    ptx_metrics_result o = ptx_metrics_result();
    const double n = 3.0 * (double)m->w * (double)m->h;
    o.mse = r[PT_METRICS_JOB_SE] / n;
    o.psnr = 10.0 * log10(1.0 / o.mse);
    o.l1 = r[PT_METRICS_JOB_AE] / n;
    o.mape = r[PT_METRICS_JOB_MAPE] / n;
    o.smape = r[PT_METRICS_JOB_SMAPE] / n;
    o.nonfinite_a = (uint64_t)r[PT_METRICS_JOB_NFA];
    o.nonfinite_b = (uint64_t)r[PT_METRICS_JOB_NFB];
    o.num_errors = (uint64_t)r[PT_METRICS_JOB_NERR];
    o.max_error = r[PT_METRICS_JOB_MAXERR];
    o.exposure = (float)r[PT_METRICS_JOBS];
    o.grad = NaN;
    if (pl.grad_blocks) {
        o.grad = r[PT_METRICS_JOB_GRAD] / (6.0 * ((double)m->w - 1.0) * ((double)m->h - 1.0));
        if (!isnan(o.grad)) o.valid |= PTX_METRICS_VALID_GRAD;
    }
    o.ssim = o.msssim = o.l1_msssim = NaN;
    for (int c = 0; c < 3; c++) {
        o.ssim_c[c] = o.msssim_c[c] = NaN;
        for (int s = 0; s < PTX_METRICS_SCALES; s++) o.mcs[s][c] = NaN;
    }
    if (with_ssim) {
        const double count = ((double)m->w - APRON) * ((double)m->h - APRON);
        for (int c = 0; c < 3; c++) o.ssim_c[c] = r[PT_METRICS_JOB_SSIM + c] / count;
        o.ssim = ((o.ssim_c[0] + o.ssim_c[1]) + o.ssim_c[2]) / 3.0;
        if (!isnan(o.ssim)) o.valid |= PTX_METRICS_VALID_SSIM;                  // (values near FLT_MAX: their squares are inf - inf in the window)
    }
    if (with_msssim) {
        for (int c = 0; c < 3; c++) {
            double prod = 1.0;
            for (int s = 0; s < PTX_METRICS_SCALES; s++) {
                o.mcs[s][c] = r[PT_METRICS_JOB_MCS + 3 * s + c] / (((double)pl.w[s] - APRON) * ((double)pl.h[s] - APRON));
                prod = prod * pow(o.mcs[s][c] > 0.0 ? o.mcs[s][c] : 0.0, (double)pl.weights[s]);
            }
            o.msssim_c[c] = prod;
        }
        o.msssim = ((o.msssim_c[0] + o.msssim_c[1]) + o.msssim_c[2]) / 3.0;
        o.l1_msssim = 0.16 * o.l1 + 0.84 * (1.0 - o.msssim);
        if (!isnan(o.msssim)) o.valid |= PTX_METRICS_VALID_MSSSIM;
    }
    o.struct_size = out->struct_size;
    memcpy(out, &o, std::min(out->struct_size, sizeof o));
    return PTX_OK;
}

namespace {

// what every compare call checks before a device call; p: the params in use
int call_problem(const char *fn, ptx_metrics *m, const ptx_metrics_params *params, ptx_metrics_params &p, const ptx_metrics_result *out) {
    if (params) p = *params;
    else ptx_default_metrics_params(&p);
    if (const char *why = pt_metrics_params_problem(p)) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": " + why);
    if (!m || !out) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": null metrics handle or result");
    if (out->struct_size < sizeof(size_t))
        return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": ptx_metrics_result.struct_size is not set (the caller's sizeof(ptx_metrics_result))");
    return PTX_OK;
}

}  // namespace

extern "C" {

void ptx_default_metrics_params(ptx_metrics_params *p) {
    if (!p) return;
    p->transform = PTX_METRICS_NONE;
    p->exposure = std::numeric_limits<float>::quiet_NaN();
    p->threshold = 0.01f;
    p->samples_a = p->samples_b = 1.f;
    p->pointwise_only = 0;
}

size_t ptx_sizeof_metrics_params(void) { return sizeof(ptx_metrics_params); }
size_t ptx_sizeof_metrics_result(void) { return sizeof(ptx_metrics_result); }
size_t ptx_sizeof_metrics_plan(void) { return sizeof(ptx_metrics_plan); }

int ptx_debug_metrics_plan(int w, int h, ptx_metrics_plan *out) {
    if (!pt_metrics_plan(w, h, out)) return pt_fail(PTX_ERR_INVALID, "ptx_debug_metrics_plan: bad frame size (1 .. 16384 either way) or NULL plan");
    return PTX_OK;
}

int ptx_debug_metrics_problem(int width, int height, const ptx_nn_image *a, const ptx_nn_image *b, const ptx_metrics_params *params) {
    ptx_metrics_params p;
    if (params) p = *params;
    else ptx_default_metrics_params(&p);
    PtNnImageView va, vb;
    return pt_metrics_problem("ptx_debug_metrics_problem", width, height, a, true, b, p, &va, &vb);
}

int ptx_metrics_create(int device, int width, int height, ptx_metrics **out) {
    if (width > PT_METRICS_MAX_SIDE || height > PT_METRICS_MAX_SIDE) width = height = 0;       // refused as a bad frame size, in the one order
    return pt_handle_create("ptx_metrics_create", "the metrics handle", device, width, height, (long long)PT_METRICS_MAX_SIDE * PT_METRICS_MAX_SIDE,
                            out, alloc_metrics);
}

void ptx_metrics_destroy(ptx_metrics *m) { pt_handle_destroy(m); }

int ptx_metrics_compare_device(ptx_metrics *m, const ptx_nn_image *a, const ptx_nn_image *b, const ptx_metrics_params *params,
                               ptx_metrics_result *out, float *device_map_or_null, void *stream) {
    ptx_metrics_params p;
    if (const int rc = call_problem("ptx_metrics_compare_device", m, params, p, out)) return rc;
    PtNnImageView va, vb;
    if (const int rc = pt_metrics_problem("ptx_metrics_compare_device", m->w, m->h, a, true, b, p, &va, &vb)) return rc;
    if (device_map_or_null && (!m->plan.ssim_valid || p.pointwise_only))
        return pt_fail(PTX_ERR_INVALID, "ptx_metrics_compare_device: no SSIM map below 11 pixels either way or with pointwise_only");
    PT_HC(hipSetDevice(m->device));
    return pt_metrics_compare(m, (hipStream_t)stream, va, vb, p, out, device_map_or_null);
}

int ptx_metrics_compare_host(ptx_metrics *m, const ptx_nn_image *a, const ptx_nn_image *b, const ptx_metrics_params *params,
                             ptx_metrics_result *out, float *host_map_or_null) {
    ptx_metrics_params p;
    if (const int rc = call_problem("ptx_metrics_compare_host", m, params, p, out)) return rc;
    PtNnImageView va, vb, da, db;
    if (const int rc = pt_metrics_problem("ptx_metrics_compare_host", m->w, m->h, a, true, b, p, &va, &vb)) return rc;
    if (host_map_or_null && (!m->plan.ssim_valid || p.pointwise_only))
        return pt_fail(PTX_ERR_INVALID, "ptx_metrics_compare_host: no SSIM map below 11 pixels either way or with pointwise_only");
    PT_HC(hipSetDevice(m->device));
    if (const int rc = pt_metrics_stage(m, 0, va, &da)) return rc;
    if (const int rc = pt_metrics_stage(m, 1, vb, &db)) return rc;
    if (host_map_or_null && !m->d_map) PT_HC(m->d_map.alloc(m->plan.map_floats));
    if (const int rc = pt_metrics_compare(m, nullptr, da, db, p, out, host_map_or_null ? m->d_map.p : nullptr)) return rc;
    if (host_map_or_null) PT_HC(hipMemcpy(host_map_or_null, m->d_map, sizeof(float) * m->plan.map_floats, hipMemcpyDeviceToHost));
    return PTX_OK;
}

}  // extern "C"
