// pt_nn.hip -- the network denoiser (ptx_nn_* of include/mi355x_pathtracer.h): Open Image Denoise's RT filter, a U-Net of sixteen
// 3 x 3 convolutions, run from a caller's TZA weight blob on the matrix cores.  ptx_denoise_nn is pt_post.hip's: it needs the tracer's
// buffers and stream.  The blob and the plan are pt_tza.h's, the memory model and the tiles of a handle made under a memory limit
// pt_nn_tiles.h's (both host only); the state's layout is in pt_nn.h; the arithmetic is defined in the public header and restated by
// tests/unet_ref.py, the tile rule by tests/nn_tiles_ref.py.  The per-tile loop (pt_nn_run_tiles) takes its two end stages from the
// caller: k_nn_input / k_nn_output here, the prefilter's two kernels in pt_nn_aux.hip, which runs this unit's networks on its guides.
//
// Kernels (the unit has optimisation flags of its own, see the Makefile; -ffp-contract=off stays, the transfer functions are restated):
//   k_nn_input  : one thread per pixel of a tile's padded window (one tile: the padded frame; the window's origin in the frame and the
//       frame's row stride are launch arguments): colour / albedo / normal sanitised and transferred into the network's
//       input, 16 fp16 channels per pixel (two 16-byte stores), zeros right of and below the window.  The scale is a launch argument or
//       read from the meter's state record on the device; thread 0 leaves the one it used in d_scale.
//   k_nn_conv<NCO> : one convolution as an implicit GEMM on v_mfma_f32_16x16x32_f16, M = Cout, N = pixels, K = 9 Cin.  A workgroup of
//       256 (4 waves) computes a tile of TILE x TILE = 16 x 16 output pixels for NCO blocks of 16 output channels (NCO = 1 .. 8, the
//       grid's z takes further groups above 128 channels); wave v owns rows 4 v .. 4 v + 3, each row the 16 columns of one MFMA.  The
//       input channels go by in chunks of 32: the chunk's 18 x 18 halo tile is staged in LDS (16-byte loads; zeros outside the tensor
//       and beyond its padded channels), then for each of the 9 taps a lane reads one 16-byte fragment per row from LDS -- its 8
//       consecutive k are 8 consecutive channels of one tap -- and one 16-byte weight fragment per channel block from global memory
//       (pre-packed in fragment order, the same 1 KiB line for the four waves).  The weights are the A operand (row = output channel)
//       and the pixels the B operand (column = pixel), so a lane ends with four consecutive output channels of one pixel: bias, ReLU,
//       one rounding to fp16 and an 8-byte store.  Sources: one tensor; or two, read directly -- the first upsampled 2 x (nearest) and
//       the second the skip, each with its own padded channel block, so no upsampled or concatenated tensor exists.  Pooled form: the
//       2 x 2 maximum is taken in registers (rows of one lane, then the neighbour column by a shuffle) and only the pooled tensor is
//       written.  dec_conv0's form writes its fp32 sums, four floats per pixel.
//   k_nn_output : one thread per pixel of the rectangle a tile keeps (one tile: the image): dec_conv0's three fp32 channels sanitised,
//       the inverse transfer, 1 / scale, written to the rectangle's place in the frame.
// No atomics; every sum has one order, which does not depend on where a pixel lies: the same bits on every run, and a tiled run
// (pt_nn_tiles.h) gives the bits of a one-tile run.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "pt_nn.h"
#include "pt_nn_transfer.h"
#include "pt_display.h"

namespace {

using namespace pt_nn_transfer;              // the transfer functions and their constants (shared with pt_nn_aux.hip)

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256, TILE = 16, HALO = TILE + 2, CHUNK = 32;
constexpr int MAX_NCO = 8;

struct InputArgs {
    int w, h, wp, hp;                         // the window and its padded size
    int x0, y0, W;                            // the window's origin in the frame, the frame's row stride in pixels
    const float *rgb, *alb, *nrm;
    int alb_stride, nrm_stride;
    float samples, scale;
    const float *scale_ptr;                   // NULL: `scale`
    float *scale_out;
    int mode, hdr;
    float norm;
    uint16_t *out;                            // [hp][wp][16] fp16
    float *raw;                               // NULL, or [h][w][9] fp32 before the rounding (ptx_kat_nn_transfer)
};

__global__ __launch_bounds__(NT) void k_nn_input(InputArgs a) {
    const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
    const float s = a.scale_ptr ? *a.scale_ptr : a.scale;
    if (idx == 0) *a.scale_out = s;
    if (idx >= (size_t)a.wp * a.hp) return;
    const int y = (int)(idx / a.wp), x = (int)(idx - (size_t)y * a.wp);
    float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool inside = x < a.w && y < a.h;
    const size_t p = ((size_t)a.y0 + y) * a.W + a.x0 + x;
    if (inside) {
        for (int c = 0; c < 3; c++)
            v[c] = transfer_forward(sanitise((a.rgb[3 * p + c] / a.samples) * s, 0.f, a.hdr ? FLT_MAX : 1.f), a.mode, a.norm);
        if (a.alb) for (int c = 0; c < 3; c++) v[3 + c] = sanitise(a.alb[(size_t)a.alb_stride * p + c], 0.f, 1.f);
        if (a.nrm) for (int c = 0; c < 3; c++) v[6 + c] = sanitise(a.nrm[(size_t)a.nrm_stride * p + c], -1.f, 1.f) * 0.5f + 0.5f;
        if (a.raw) for (int c = 0; c < 9; c++) a.raw[9 * ((size_t)y * a.w + x) + c] = v[c];
    }
    half8 lo, hi = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 8; c++) lo[c] = (_Float16)v[c];
    hi[0] = (_Float16)v[8];
    half8 *o = reinterpret_cast<half8 *>(a.out) + 2 * idx;
    o[0] = lo; o[1] = hi;
}

struct OutputArgs {
    int w, h, wp;                             // the rectangle kept; the tile's padded width
    int ix, iy;                               // where the rectangle begins in the tile's output
    int ox, oy, W;                            // ... and in the frame; the frame's row stride in pixels
    const float *net;                         // [hp][wp][4] fp32
    const float *scale;
    int mode, hdr;
    float xmax;
    float *out;                               // [H][W][3]
};

__global__ __launch_bounds__(NT) void k_nn_output(OutputArgs a) {
    const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= (size_t)a.w * a.h) return;
    const int y = (int)(idx / a.w), x = (int)(idx - (size_t)y * a.w);
    const float s = *a.scale, inv = s != 0.f ? 1.f / s : 0.f;
    const float4 n = reinterpret_cast<const float4 *>(a.net)[((size_t)a.iy + y) * a.wp + a.ix + x];
    const size_t p = ((size_t)a.oy + y) * a.W + a.ox + x;
    const float in[3] = {n.x, n.y, n.z};
    for (int c = 0; c < 3; c++) {
        float v = transfer_inverse(sanitise(in[c], 0.f, FLT_MAX), a.mode, a.xmax);
        if (!a.hdr) v = fminf(v, 1.f);
        a.out[3 * p + c] = v * inv;
    }
}

// ---- the convolution ------------------------------------------------------------------------------------------------------------------
struct ConvArgs {
    const uint16_t *src0, *src1;              // fp16 bits; src1 NULL: one source
    const uint16_t *w;                        // fragment order, see pack_weights
    const float *bias;                        // padded to the groups' channel blocks
    uint16_t *out;                            // fp16, [H][W][coutp], or [H/2][W/2][coutp] when pool
    float *out32;                             // not NULL: [H][W][4] fp32 instead (channels 0 .. 3)
    int W, H;                                 // of the convolution's output, before the pool
    int c0p, c1p, coutp, nchunks;
    int upsample, pool, relu;
};

template <int NCO>
__global__ __launch_bounds__(NT) void k_nn_conv(ConvArgs a) {
    __shared__ __attribute__((aligned(16))) _Float16 s_tile[HALO * HALO * CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE, group = blockIdx.z;
    const int cinp = a.c0p + a.c1p;
    const int W0 = a.upsample ? a.W >> 1 : a.W;
    f32x4 acc[NCO][4];
#pragma unroll
    for (int cb = 0; cb < NCO; cb++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[cb][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    const half8 *wfrag = reinterpret_cast<const half8 *>(a.w) + (size_t)group * a.nchunks * 9 * NCO * 64 + lane;

    for (int chunk = 0; chunk < a.nchunks; chunk++) {
        __syncthreads();                                             // the last chunk's reads are done
        for (int i = tid; i < HALO * HALO * (CHUNK / 8); i += NT) {
            const int pix = i >> 2, q = i & 3;
            const int py = pix / HALO, px = pix - py * HALO;
            const int gy = ty0 + py - 1, gx = tx0 + px - 1, c = chunk * CHUNK + q * 8;
            half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && c < cinp) {
                if (c < a.c0p) {
                    const size_t p = a.upsample ? (size_t)(gy >> 1) * W0 + (gx >> 1) : (size_t)gy * a.W + gx;
                    v = *reinterpret_cast<const half8 *>(a.src0 + p * a.c0p + c);
                } else {
                    v = *reinterpret_cast<const half8 *>(a.src1 + ((size_t)gy * a.W + gx) * a.c1p + (c - a.c0p));
                }
            }
            *reinterpret_cast<half8 *>(&s_tile[i * 8]) = v;
        }
        __syncthreads();
        const half8 *wc = wfrag + (size_t)chunk * 9 * NCO * 64;
#pragma unroll
        for (int ky = 0; ky < 3; ky++)
#pragma unroll
            for (int kx = 0; kx < 3; kx++) {
                half8 b[4];
#pragma unroll
                for (int r = 0; r < 4; r++)
                    b[r] = *reinterpret_cast<const half8 *>(&s_tile[((wave * 4 + r + ky) * HALO + col + kx) * CHUNK + g * 8]);
#pragma unroll
                for (int cb = 0; cb < NCO; cb++) {
                    const half8 w = wc[((ky * 3 + kx) * NCO + cb) * 64];
#pragma unroll
                    for (int r = 0; r < 4; r++) acc[cb][r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, b[r], acc[cb][r], 0, 0, 0);
                }
            }
    }

    // a lane holds output channels co .. co + 3 of pixel (row, col) in acc[cb][r]
    const int x = tx0 + col;
#pragma unroll
    for (int cb = 0; cb < NCO; cb++) {
        const int co = (group * NCO + cb) * 16 + g * 4;
        const float4 bias = *reinterpret_cast<const float4 *>(a.bias + co);
        f32x4 v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            v[r] = f32x4{acc[cb][r][0] + bias.x, acc[cb][r][1] + bias.y, acc[cb][r][2] + bias.z, acc[cb][r][3] + bias.w};
            if (a.relu)
                for (int j = 0; j < 4; j++) v[r][j] = fmaxf(v[r][j], 0.f);
        }
        if (a.pool) {
#pragma unroll
            for (int rp = 0; rp < 2; rp++) {
                const int y = ty0 + wave * 4 + 2 * rp;
                half4 o;
                for (int j = 0; j < 4; j++) {
                    float m = fmaxf(v[2 * rp][j], v[2 * rp + 1][j]);
                    m = fmaxf(m, __shfl_xor(m, 1, 64));
                    o[j] = (_Float16)m;
                }
                if (!(col & 1) && x < a.W && y < a.H && co < a.coutp)
                    *reinterpret_cast<half4 *>(a.out + ((size_t)(y >> 1) * (a.W >> 1) + (x >> 1)) * a.coutp + co) = o;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int y = ty0 + wave * 4 + r;
                if (x >= a.W || y >= a.H || co >= a.coutp) continue;
                const size_t p = (size_t)y * a.W + x;
                if (a.out32) {
                    if (co == 0) *reinterpret_cast<float4 *>(a.out32 + 4 * p) = float4{v[r][0], v[r][1], v[r][2], v[r][3]};
                } else {
                    half4 o;
                    for (int j = 0; j < 4; j++) o[j] = (_Float16)v[r][j];
                    *reinterpret_cast<half4 *>(a.out + p * a.coutp + co) = o;
                }
            }
        }
    }
}

int pad16(int c) { return (c + 15) / 16 * 16; }

// How a layer of `cout` channels is split: `groups` launches in z of `nco` blocks of 16 channels each
void split_cout(int cout, int *groups, int *nco) {
    const int blocks = pad16(cout) / 16;
    *groups = (blocks + MAX_NCO - 1) / MAX_NCO;
    *nco = (blocks + *groups - 1) / *groups;
}

uint16_t half_bits(float f) {
    const _Float16 h = (_Float16)f;               // round to nearest even
    uint16_t b; memcpy(&b, &h, 2);
    return b;
}

// The weights in the order the kernel's lanes read them: [group][chunk][tap][cb][lane][j], the A fragment of the MFMA: lane l, element
// j = weight[co = (group * nco + cb) * 16 + (l & 15)][k = chunk * 32 + 8 (l >> 4) + j][tap].  k runs over the PADDED input channels:
// the first source's c0p, then the second's; a padded channel, like one beyond the last chunk's end, has weight 0.  get(co, ci, tap)
// reads the blob's [cout][cin0 + cin1][3][3].
template <class Get>
void pack_weights(int cin0, int cin1, int cout, Get get, const float *bias, std::vector<uint16_t> &w, std::vector<float> &b) {
    const int c0p = pad16(cin0), c1p = cin1 ? pad16(cin1) : 0, cinp = c0p + c1p, nchunks = (cinp + CHUNK - 1) / CHUNK;
    int groups, nco;
    split_cout(cout, &groups, &nco);
    w.assign((size_t)groups * nchunks * 9 * nco * 64 * 8, 0);
    b.assign((size_t)groups * nco * 16, 0.f);
    for (int co = 0; co < cout; co++) b[(size_t)co] = bias[co];
    size_t at = 0;
    for (int grp = 0; grp < groups; grp++)
        for (int chunk = 0; chunk < nchunks; chunk++)
            for (int tap = 0; tap < 9; tap++)
                for (int cb = 0; cb < nco; cb++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int j = 0; j < 8; j++, at++) {
                            const int co = (grp * nco + cb) * 16 + (lane & 15), cp = chunk * CHUNK + 8 * (lane >> 4) + j;
                            if (co >= cout || cp >= cinp) continue;
                            int ci = -1;
                            if (cp < c0p) { if (cp < cin0) ci = cp; }
                            else if (cp - c0p < cin1) ci = cin0 + cp - c0p;
                            if (ci >= 0) w[at] = half_bits(get(co, ci, tap));
                        }
}

template <int NCO> void launch_conv_n(hipStream_t st, dim3 grid, const ConvArgs &a) { hipLaunchKernelGGL(k_nn_conv<NCO>, grid, dim3(NT), 0, st, a); }

int launch_conv(hipStream_t st, const ConvArgs &a, int cout) {
    int groups, nco;
    split_cout(cout, &groups, &nco);
    const dim3 grid((unsigned)((a.W + TILE - 1) / TILE), (unsigned)((a.H + TILE - 1) / TILE), (unsigned)groups);
    switch (nco) {
    case 1: launch_conv_n<1>(st, grid, a); break;
    case 2: launch_conv_n<2>(st, grid, a); break;
    case 3: launch_conv_n<3>(st, grid, a); break;
    case 4: launch_conv_n<4>(st, grid, a); break;
    case 5: launch_conv_n<5>(st, grid, a); break;
    case 6: launch_conv_n<6>(st, grid, a); break;
    case 7: launch_conv_n<7>(st, grid, a); break;
    default: launch_conv_n<8>(st, grid, a); break;
    }
    PT_HC(hipGetLastError());
    return PTX_OK;
}

thread_local const PtNnPlan *tl_plan = nullptr;      // ptx_nn_create's plan, for alloc_nn (pt_handle_create hands over the handle alone)
thread_local int tl_max_memory_mb = 0;               // ... and ptx_nn_create_tiled's limit
thread_local uint8_t *tl_scratch = nullptr;          // ... and pt_nn_create_shared's scratch (NULL: the handle allocates its own)

int alloc_nn(ptx_nn *n) {
    const PtNnPlan &plan = *tl_plan;
    n->tiling = pt_nn_tiling(plan, n->w, n->h, tl_max_memory_mb);
    n->wp = n->tiling.tile_width; n->hp = n->tiling.tile_height; n->ic = plan.ic;
    PT_HC(hipSetDevice(n->device));
    const PtNnScratch scratch = pt_nn_scratch(plan, n->wp, n->hp);
    n->macs = pt_nn_tiling_macs(plan, n->tiling);
    for (int i = 0; i < PT_NN_LAYERS; i++) {
        const PtNnLayer &P = plan.layers[i];
        PtNnLayerDev &L = n->L[i];
        L.cin0 = P.cin0; L.cin1 = P.cin1; L.cout = P.cout;
        L.c0p = pad16(P.cin0); L.c1p = P.cin1 ? pad16(P.cin1) : 0; L.coutp = pad16(P.cout);
        L.level = P.level; L.src0 = P.src0; L.src1 = P.src1; L.relu = P.relu; L.pool = P.pool; L.upsample = P.upsample;
        snprintf(n->names[i], sizeof n->names[i], "%s", P.name);
        L.out_offset = scratch.out_offset[i];
        const PtTzaTensor *wt = P.weight;
        const int cin = P.cin0 + P.cin1;
        std::vector<uint16_t> w;
        std::vector<float> b, bias((size_t)P.cout);
        for (int co = 0; co < P.cout; co++) bias[(size_t)co] = P.bias->at((uint64_t)co);
        pack_weights(P.cin0, P.cin1, P.cout, [&](int co, int ci, int tap) { return wt->at(((uint64_t)co * cin + ci) * 9 + tap); }, bias.data(), w, b);
        PT_HC(L.w.upload(w));
        PT_HC(L.b.upload(b));
    }
    n->in_offset = scratch.in_offset;
    n->scratch_bytes = scratch.total;
    if (tl_scratch) n->scratch = tl_scratch;
    else {
        PT_HC(n->d_scratch.alloc(scratch.total));
        n->scratch = n->d_scratch;
    }
    PT_HC(n->d_scale.alloc(1));
    PT_HC(n->d_scale.zero());
    PT_HC(n->ev.create(hipEventDisableTiming));
    return PTX_OK;
}

void fill_info(const PtNnPlan &plan, ptx_nn_info *o) {
    *o = ptx_nn_info();
    o->input_channels = plan.ic;
    o->layers = PT_NN_LAYERS;
    for (int i = 0; i < PT_NN_LAYERS; i++) {
        o->cin[i] = plan.layers[i].cin0 + plan.layers[i].cin1;
        o->cout[i] = plan.layers[i].cout;
        snprintf(o->name[i], sizeof o->name[i], "%s", plan.layers[i].name);
    }
}

int mode_of(const ptx_nn_params &p) { return p.hdr ? MODE_PU : p.srgb ? MODE_LINEAR : MODE_SRGB; }

int launch_input(hipStream_t st, const InputArgs &a) {
    const size_t n = (size_t)a.wp * a.hp;
    hipLaunchKernelGGL(k_nn_input, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, a);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

int launch_output(hipStream_t st, const OutputArgs &a) {
    const size_t n = (size_t)a.w * a.h;
    hipLaunchKernelGGL(k_nn_output, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, a);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

int device_problem(const char *fn, int device) {
    if (device < 0) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": device ordinal out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return pt_fail(PTX_ERR_NODEVICE, "no HIP device available; the network denoiser has no CPU path");
    }
    if (device >= ndev) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": device ordinal out of range");
    return PTX_OK;
}

int read_file(const char *fn, const char *path, std::vector<uint8_t> &blob) {
    if (!path) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": path is NULL");
    FILE *f = fopen(path, "rb");
    if (!f) return pt_fail(PTX_ERR_IO, std::string(fn) + ": cannot open " + path);
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + got);
    fclose(f);
    return PTX_OK;
}

// What ptx_nn_create_tiled refuses without a device, before pt_handle_create's own checks: the blob, the limit, a frame above the cap
int tiled_problem(const char *fn, const void *tza, size_t bytes, int width, int height, int max_memory_mb, PtNnPlan &plan) {
    std::string err;
    if (!pt_nn_plan(tza, bytes, plan, err)) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": " + err);
    if (max_memory_mb < 0) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": max_memory_mb must be >= 0 (0: no memory limit)");
    if (width > PTX_NN_MAX_FRAME || height > PTX_NN_MAX_FRAME)
        return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": bad frame size (a tiled frame is at most 16384 x 16384)");
    return PTX_OK;
}

void fill_tiling(const PtNnTiling &t, size_t scratch_bytes, uint64_t macs, ptx_nn_tiling *o, ptx_nn_tile *tiles, int cap) {
    *o = ptx_nn_tiling();
    o->width = t.width; o->height = t.height; o->tile_width = t.tile_width; o->tile_height = t.tile_height;
    o->tiles_x = t.tiles_x; o->tiles_y = t.tiles_y; o->max_memory_mb = t.max_memory_mb;
    o->scratch_bytes = scratch_bytes; o->macs = macs;
    for (int k = 0; tiles && k < cap && k < t.count(); k++) tiles[k] = pt_nn_tile_at(t, k);
}

// the byte ranges [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

ptx_nn::~ptx_nn() { if (meter) ptx_display_destroy(meter); }

const char *pt_nn_params_problem(const ptx_nn_params &p, float samples) {
    if (p.hdr != 0 && p.hdr != 1) return "ptx_nn_params.hdr must be 0 or 1";
    if (p.srgb != 0 && p.srgb != 1) return "ptx_nn_params.srgb must be 0 or 1";
    if (!isnan(p.input_scale) && (!(p.input_scale >= 0.f) || isinf(p.input_scale))) return "ptx_nn_params.input_scale must be NaN (automatic) or finite and >= 0";
    if (!(samples > 0.f) || isinf(samples)) return "the network denoiser's divisor (samples) must be finite and positive";
    return nullptr;
}

// the sixteen convolutions of one wp x hp tile in the handle's scratch; ev: NULL, or sixteen events, one recorded behind each layer
static int run_layers(ptx_nn *n, hipStream_t st, int wp, int hp, OwnedEvent *ev = nullptr) {
    uint8_t *base = n->scratch;
    for (int i = 0; i < PT_NN_LAYERS; i++) {
        const PtNnLayerDev &L = n->L[i];
        auto tensor = [&](int src) { return reinterpret_cast<const uint16_t *>(base + (src == -1 ? n->in_offset : n->L[src].out_offset)); };
        ConvArgs a;
        a.src0 = tensor(L.src0); a.src1 = L.src1 == -2 ? nullptr : tensor(L.src1);
        a.w = L.w; a.bias = L.b;
        const bool last = i == PT_NN_LAYERS - 1;
        a.out = last ? nullptr : reinterpret_cast<uint16_t *>(base + L.out_offset);
        a.out32 = last ? reinterpret_cast<float *>(base + L.out_offset) : nullptr;
        a.W = wp >> L.level; a.H = hp >> L.level;
        a.c0p = L.c0p; a.c1p = L.c1p; a.coutp = L.coutp; a.nchunks = (L.c0p + L.c1p + CHUNK - 1) / CHUNK;
        a.upsample = L.upsample; a.pool = L.pool; a.relu = L.relu;
        if (const int rc = launch_conv(st, a, L.cout)) return rc;
        if (ev) PT_HC(hipEventRecord(ev[i], st));
    }
    return PTX_OK;
}

static_assert(PT_NN_TILE_UNITS == PT_NN_LAYERS + 2, "a tile's units: input, the layers, output");

// a cancel: nothing further is enqueued, and the call returns after what is in flight on st
static int cancelled(ptx_nn *n, hipStream_t st) {
    const double at = n->progress.done >= n->progress.total ? 1.0 : (double)n->progress.done / (double)n->progress.total;
    PT_HC(hipStreamSynchronize(st));
    return pt_fail(PTX_ERR_CANCELLED, "the network denoiser's progress monitor cancelled the call at n = " + std::to_string(at));
}

// the markers of two tiles' stages and, last, of the copy-out
static int progress_events(ptx_nn *n) {
    while (n->progress_ev.size() < 2 * PT_NN_TILE_UNITS + 1) {
        OwnedEvent e;
        PT_HC(e.create(hipEventDisableTiming));
        n->progress_ev.push_back(std::move(e));
    }
    return PTX_OK;
}

int pt_nn_progress_begin(const char *fn, ptx_nn *n, bool copy_out, bool *mine) {
    *mine = false;
    if (!n->progress.fn || n->progress.running) return PTX_OK;
    if (!n->progress.begin(n->tiling.count(), copy_out))
        return pt_fail(PTX_ERR_CANCELLED, std::string(fn) + ": the progress monitor cancelled the call at n = 0, before anything was enqueued");
    *mine = true;
    return PTX_OK;
}

int pt_nn_progress_frame_unit(ptx_nn *n, hipStream_t st) {
    if (!n->progress.running) return PTX_OK;
    if (const int rc = progress_events(n)) return rc;
    OwnedEvent &e = n->progress_ev[2 * PT_NN_TILE_UNITS];
    PT_HC(hipEventRecord(e, st));
    PT_HC(hipEventSynchronize(e));
    return n->progress.unit() ? PTX_OK : cancelled(n, st);
}

int pt_nn_progress_end(ptx_nn *n, bool mine, int rc) {
    if (mine) n->progress.end();
    return rc;
}

// the tile loop of a call under a monitor: a marker behind every stage, the reports one tile behind the enqueue (pt_nn_progress.h)
static int run_tiles_reporting(ptx_nn *n, hipStream_t st, const PtNnStages &stages) {
    if (const int rc = progress_events(n)) return rc;
    uint8_t *base = n->scratch;
    uint16_t *net_in = reinterpret_cast<uint16_t *>(base + n->in_offset);
    const float *net_out = reinterpret_cast<const float *>(base + n->L[PT_NN_LAYERS - 1].out_offset);
    auto enqueue = [&](int k) {
        const ptx_nn_tile T = pt_nn_tile_at(n->tiling, k);
        const int wp = pad16(T.w), hp = pad16(T.h);
        OwnedEvent *ev = &n->progress_ev[(size_t)(k & 1) * PT_NN_TILE_UNITS];
        if (const int rc = stages.input(stages.ctx, st, T, wp, hp, net_in)) return rc;
        PT_HC(hipEventRecord(ev[0], st));
        if (const int rc = run_layers(n, st, wp, hp, ev + 1)) return rc;
        if (const int rc = stages.output(stages.ctx, st, T, wp, net_out)) return rc;
        PT_HC(hipEventRecord(ev[PT_NN_TILE_UNITS - 1], st));
        return (int)PTX_OK;
    };
    auto wait = [&](int k, int s) {
        PT_HC(hipEventSynchronize(n->progress_ev[(size_t)(k & 1) * PT_NN_TILE_UNITS + s]));
        return (int)PTX_OK;
    };
    const int rc = pt_nn_progress_tiles(n->progress, n->tiling.count(), enqueue, wait);
    return rc == PTX_ERR_CANCELLED ? cancelled(n, st) : rc;
}

// every tile in the handle's one scratch, a smaller tile in a prefix of each tensor
int pt_nn_run_tiles(ptx_nn *n, hipStream_t st, const PtNnStages &stages) {
    if (n->progress.running) return run_tiles_reporting(n, st, stages);
    uint8_t *base = n->scratch;
    uint16_t *net_in = reinterpret_cast<uint16_t *>(base + n->in_offset);
    const float *net_out = reinterpret_cast<const float *>(base + n->L[PT_NN_LAYERS - 1].out_offset);
    for (int k = 0; k < n->tiling.count(); k++) {
        const ptx_nn_tile T = pt_nn_tile_at(n->tiling, k);
        const int wp = pad16(T.w), hp = pad16(T.h);
        if (const int rc = stages.input(stages.ctx, st, T, wp, hp, net_in)) return rc;
        if (const int rc = run_layers(n, st, wp, hp)) return rc;
        if (const int rc = stages.output(stages.ctx, st, T, wp, net_out)) return rc;
    }
    return PTX_OK;
}

int pt_nn_enqueue(ptx_nn *n, hipStream_t st, const float *rgb, float samples, const float *alb, int alb_stride, const float *nrm, int nrm_stride,
                  const ptx_nn_params &p, float *out_rgb) {
    const bool automatic = isnan(p.input_scale) && p.hdr;
    if (automatic && !n->meter)
        if (const int rc = ptx_display_create(n->device, n->w, n->h, &n->meter)) {
            if (rc == PTX_ERR_INVALID && (n->w > PTX_NN_MAX_WIDTH || n->h > PTX_NN_MAX_HEIGHT))
                return pt_fail(rc, "the network denoiser's automatic hdr scale is refused at " + std::to_string(n->w) + " x " + std::to_string(n->h) +
                                       ": the display handle that meters the frame refuses this size (give ptx_nn_params.input_scale)");
            return rc;
        }
    PT_HC(n->wait_stream(st));
    struct Ends { InputArgs ia; OutputArgs oa; } e;
    InputArgs &ia = e.ia;
    ia.W = n->w;
    ia.rgb = rgb; ia.alb = alb; ia.nrm = nrm; ia.alb_stride = alb_stride; ia.nrm_stride = nrm_stride;
    ia.samples = samples; ia.scale = isnan(p.input_scale) ? 1.f : p.input_scale;
    ia.scale_ptr = nullptr;
    if (automatic) {
        if (const int rc = pt_display_meter_enqueue(n->meter, st, rgb, samples, 0.18f)) return rc;
        ia.scale_ptr = &n->meter->d_state.p->metered;
    }
    ia.scale_out = n->d_scale;
    ia.mode = mode_of(p); ia.hdr = p.hdr; ia.norm = pu_norm();
    ia.raw = nullptr;
    OutputArgs &oa = e.oa;
    oa.W = n->w;
    oa.scale = n->d_scale; oa.mode = mode_of(p); oa.hdr = p.hdr; oa.xmax = pu_xmax();
    oa.out = out_rgb;
    // the scale is the frame's, the same for each tile
    PtNnStages stages;
    stages.ctx = &e;
    stages.input = [](void *ctx, hipStream_t s, const ptx_nn_tile &T, int wp, int hp, uint16_t *net_in) {
        InputArgs a = static_cast<Ends *>(ctx)->ia;
        a.w = T.w; a.h = T.h; a.wp = wp; a.hp = hp; a.x0 = T.x; a.y0 = T.y; a.out = net_in;
        return launch_input(s, a);
    };
    stages.output = [](void *ctx, hipStream_t s, const ptx_nn_tile &T, int wp, const float *net_out) {
        OutputArgs a = static_cast<Ends *>(ctx)->oa;
        a.w = T.out_w; a.h = T.out_h; a.wp = wp; a.net = net_out;
        a.ix = T.out_x - T.x; a.iy = T.out_y - T.y; a.ox = T.out_x; a.oy = T.out_y;
        return launch_output(s, a);
    };
    if (const int rc = pt_nn_run_tiles(n, st, stages)) return rc;
    PT_HC(n->record(st));
    return PTX_OK;
}

int pt_nn_device_problem(const char *fn, int device) { return device_problem(fn, device); }
int pt_nn_read_file(const char *fn, const char *path, std::vector<uint8_t> &blob) { return read_file(fn, path, blob); }

// max_memory_mb < 0: one tile covers the frame (ptx_nn_create's rule and cap); else ptx_nn_create_tiled's
int pt_nn_blob_problem(const char *fn, const void *tza, size_t bytes, int width, int height, int max_memory_mb, PtNnPlan &plan) {
    if (max_memory_mb >= 0) return tiled_problem(fn, tza, bytes, width, height, max_memory_mb, plan);
    std::string err;
    if (!pt_nn_plan(tza, bytes, plan, err)) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": " + err);
    if (width > PTX_NN_MAX_WIDTH || height > PTX_NN_MAX_HEIGHT)
        return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": bad frame size (one tile covers the frame; at most 7680 x 4320)");
    return PTX_OK;
}

int pt_nn_create_shared(const char *fn, int device, int width, int height, const PtNnPlan &plan, int max_memory_mb, uint8_t *scratch, ptx_nn **out) {
    const bool one = max_memory_mb < 0;
    tl_plan = &plan; tl_max_memory_mb = one ? 0 : max_memory_mb; tl_scratch = scratch;
    const long long cap = one ? (long long)PTX_NN_MAX_WIDTH * PTX_NN_MAX_HEIGHT : (long long)PTX_NN_MAX_FRAME * PTX_NN_MAX_FRAME;
    const int rc = pt_handle_create(fn, "the network denoiser", device, width, height, cap, out, alloc_nn);
    tl_plan = nullptr; tl_max_memory_mb = 0; tl_scratch = nullptr;
    return rc;
}

extern "C" {

void ptx_default_nn_params(ptx_nn_params *p) {
    if (!p) return;
    p->hdr = 0;
    p->srgb = 0;
    p->input_scale = NAN;
}

size_t ptx_sizeof_nn_params(void) { return sizeof(ptx_nn_params); }
size_t ptx_sizeof_nn_info(void) { return sizeof(ptx_nn_info); }
size_t ptx_sizeof_nn_tile(void) { return sizeof(ptx_nn_tile); }
size_t ptx_sizeof_nn_tiling(void) { return sizeof(ptx_nn_tiling); }

int ptx_debug_tza_list(const void *tza, size_t bytes, char *out, size_t cap, size_t *needed) {
    std::vector<PtTzaTensor> tensors;
    std::string err;
    if (!pt_tza_parse(tza, bytes, tensors, err)) return pt_fail(PTX_ERR_INVALID, "ptx_debug_tza_list: " + err);
    std::string text;
    for (const auto &t : tensors) {
        text += t.name + " " + std::to_string(t.dims.size());
        for (const uint32_t d : t.dims) text += " " + std::to_string(d);
        text += " " + t.layout + " " + std::string(1, t.type) + " " + std::to_string(t.offset) + "\n";
    }
    if (needed) *needed = text.size() + 1;
    if (out && cap >= text.size() + 1) memcpy(out, text.c_str(), text.size() + 1);
    return PTX_OK;
}

int ptx_debug_nn_plan(const void *tza, size_t bytes, ptx_nn_info *out) {
    PtNnPlan plan;
    std::string err;
    if (!pt_nn_plan(tza, bytes, plan, err)) return pt_fail(PTX_ERR_INVALID, "ptx_debug_nn_plan: " + err);
    if (out) fill_info(plan, out);
    return PTX_OK;
}

int ptx_nn_create(int device, int width, int height, const void *tza, size_t bytes, ptx_nn **out) {
    if (out) *out = nullptr;
    PtNnPlan plan;
    std::string err;
    if (!pt_nn_plan(tza, bytes, plan, err)) return pt_fail(PTX_ERR_INVALID, "ptx_nn_create: " + err);
    if (width > PTX_NN_MAX_WIDTH || height > PTX_NN_MAX_HEIGHT)
        return pt_fail(PTX_ERR_INVALID, "ptx_nn_create: bad frame size (one tile covers the frame; at most 7680 x 4320)");
    tl_plan = &plan;
    const int rc = pt_handle_create("ptx_nn_create", "the network denoiser", device, width, height, (long long)PTX_NN_MAX_WIDTH * PTX_NN_MAX_HEIGHT, out, alloc_nn);
    tl_plan = nullptr;
    return rc;
}

int ptx_nn_create_from_file(int device, int width, int height, const char *path, ptx_nn **out) {
    if (out) *out = nullptr;
    std::vector<uint8_t> blob;
    if (const int rc = read_file("ptx_nn_create_from_file", path, blob)) return rc;
    return ptx_nn_create(device, width, height, blob.data(), blob.size(), out);
}

int ptx_nn_create_tiled(int device, int width, int height, const void *tza, size_t bytes, int max_memory_mb, ptx_nn **out) {
    if (out) *out = nullptr;
    PtNnPlan plan;
    if (const int rc = tiled_problem("ptx_nn_create_tiled", tza, bytes, width, height, max_memory_mb, plan)) return rc;
    tl_plan = &plan; tl_max_memory_mb = max_memory_mb;
    const int rc = pt_handle_create("ptx_nn_create_tiled", "the network denoiser", device, width, height, (long long)PTX_NN_MAX_FRAME * PTX_NN_MAX_FRAME, out, alloc_nn);
    tl_plan = nullptr; tl_max_memory_mb = 0;
    return rc;
}

int ptx_nn_create_from_file_tiled(int device, int width, int height, const char *path, int max_memory_mb, ptx_nn **out) {
    if (out) *out = nullptr;
    std::vector<uint8_t> blob;
    if (const int rc = read_file("ptx_nn_create_from_file_tiled", path, blob)) return rc;
    return ptx_nn_create_tiled(device, width, height, blob.data(), blob.size(), max_memory_mb, out);
}

int ptx_debug_nn_tiling(const void *tza, size_t bytes, int width, int height, int max_memory_mb, ptx_nn_tiling *tiling, ptx_nn_tile *tiles, int cap) {
    const char *fn = "ptx_debug_nn_tiling";
    PtNnPlan plan;
    if (const int rc = tiled_problem(fn, tza, bytes, width, height, max_memory_mb, plan)) return rc;
    if (!tiling) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": tiling is NULL");
    if (width < 1 || height < 1) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": bad frame size");
    const PtNnTiling t = pt_nn_tiling(plan, width, height, max_memory_mb);
    fill_tiling(t, pt_nn_scratch(plan, t.tile_width, t.tile_height).total, pt_nn_tiling_macs(plan, t), tiling, tiles, cap);
    return PTX_OK;
}

int ptx_nn_get_tiling(ptx_nn *n, ptx_nn_tiling *tiling, ptx_nn_tile *tiles, int cap) {
    if (!n || !tiling) return pt_fail(PTX_ERR_INVALID, "ptx_nn_get_tiling: null handle or tiling");
    fill_tiling(n->tiling, n->scratch_bytes, n->macs, tiling, tiles, cap);
    return PTX_OK;
}

void ptx_nn_destroy(ptx_nn *n) { pt_handle_destroy(n); }

int ptx_nn_get_info(ptx_nn *n, ptx_nn_info *out) {
    if (!n || !out) return pt_fail(PTX_ERR_INVALID, "ptx_nn_get_info: null handle or info");
    *out = ptx_nn_info();
    out->width = n->w; out->height = n->h; out->padded_width = n->wp; out->padded_height = n->hp;
    out->input_channels = n->ic;
    out->layers = PT_NN_LAYERS;
    for (int i = 0; i < PT_NN_LAYERS; i++) {
        out->cin[i] = n->L[i].cin0 + n->L[i].cin1;
        out->cout[i] = n->L[i].cout;
        memcpy(out->name[i], n->names[i], sizeof out->name[i]);
    }
    out->scratch_bytes = n->scratch_bytes;
    out->macs = n->macs;
    return PTX_OK;
}

int ptx_nn_denoise_device(ptx_nn *n, const float *device_rgb, float samples, const float *device_alb3, const float *device_nrm3,
                          const ptx_nn_params *params, float *device_out_rgb, void *stream) {
    ptx_nn_params p;
    if (params) p = *params;
    else ptx_default_nn_params(&p);
    if (const char *why = pt_nn_params_problem(p, samples)) return pt_fail(PTX_ERR_INVALID, why);
    if (!n || !device_rgb || !device_out_rgb) return pt_fail(PTX_ERR_INVALID, "ptx_nn_denoise_device: null handle, frame or result");
    if ((device_alb3 != nullptr) != (n->ic >= 6))
        return pt_fail(PTX_ERR_INVALID, std::string("ptx_nn_denoise_device: the weights take ") + std::to_string(n->ic) + " input channels: albedo " +
                                            (n->ic >= 6 ? "is required" : "must be NULL"));
    if ((device_nrm3 != nullptr) != (n->ic >= 9))
        return pt_fail(PTX_ERR_INVALID, std::string("ptx_nn_denoise_device: the weights take ") + std::to_string(n->ic) + " input channels: normals " +
                                            (n->ic >= 9 ? "are required" : "must be NULL"));
    if (n->tiling.count() > 1) {
        const size_t frame = 3 * sizeof(float) * (size_t)n->w * n->h;
        const void *in[3] = {device_rgb, device_alb3, device_nrm3};
        for (const void *src : in)
            if (src && ranges_overlap(device_out_rgb, frame, src, frame))
                return pt_fail(PTX_ERR_INVALID, "ptx_nn_denoise_device: with more than one tile the result may not overlap the colour, albedo or normal "
                                                "frame in memory (a later tile reads pixels an earlier tile's result would have replaced)");
    }
    PT_HC(hipSetDevice(n->device));
    bool mine;
    if (const int rc = pt_nn_progress_begin("ptx_nn_denoise_device", n, false, &mine)) return rc;
    return pt_nn_progress_end(n, mine, pt_nn_enqueue(n, (hipStream_t)stream, device_rgb, samples, device_alb3, 3, device_nrm3, 3, p, device_out_rgb));
}

int ptx_nn_denoise_host(ptx_nn *n, const float *rgb, float samples, const float *alb3, const float *nrm3, const ptx_nn_params *params, float *out_rgb) {
    if (!n || !rgb || !out_rgb) return pt_fail(PTX_ERR_INVALID, "ptx_nn_denoise_host: null handle, frame or result");
    const size_t count = 3 * (size_t)n->w * n->h;
    PT_HC(hipSetDevice(n->device));
    PT_HC(n->wait_host());
    bool mine;
    if (const int rc = pt_nn_progress_begin("ptx_nn_denoise_host", n, false, &mine)) return rc;
    const float *host[3] = {rgb, alb3, nrm3};
    for (int k = 0; k < 4; k++) {
        if (k < 3 && !host[k]) continue;
        hipError_t e = hipSuccess;
        if (!n->d_stage[k]) e = n->d_stage[k].alloc(count);
        if (e == hipSuccess && k < 3) e = hipMemcpy(n->d_stage[k], host[k], sizeof(float) * count, hipMemcpyHostToDevice);
        if (e != hipSuccess) return pt_nn_progress_end(n, mine, pt_fail(PTX_ERR_HIP, std::string("ptx_nn_denoise_host: staging: ") + hipGetErrorString(e)));
    }
    if (const int rc = pt_nn_progress_end(n, mine, ptx_nn_denoise_device(n, n->d_stage[0], samples, alb3 ? n->d_stage[1].p : nullptr,
                                                                         nrm3 ? n->d_stage[2].p : nullptr, params, n->d_stage[3], nullptr)))
        return rc;
    PT_HC(hipEventSynchronize(n->ev));
    PT_HC(hipMemcpy(out_rgb, n->d_stage[3], sizeof(float) * count, hipMemcpyDeviceToHost));
    return PTX_OK;
}

int ptx_nn_set_progress(ptx_nn *n, ptx_nn_progress_fn fn, void *user) {
    if (!n) return pt_fail(PTX_ERR_INVALID, "ptx_nn_set_progress: null handle");
    if (n->progress.running) return pt_fail(PTX_ERR_INVALID, "ptx_nn_set_progress: called from the monitor of a running call");
    n->progress.fn = fn;
    n->progress.user = fn ? user : nullptr;
    return PTX_OK;
}

int ptx_nn_read_scale(ptx_nn *n, float *scale) {
    if (!n || !scale) return pt_fail(PTX_ERR_INVALID, "ptx_nn_read_scale: null handle or result");
    if (!n->used) return pt_fail(PTX_ERR_INVALID, "ptx_nn_read_scale: no denoise on this handle yet");
    PT_HC(hipSetDevice(n->device));
    PT_HC(hipEventSynchronize(n->ev));
    PT_HC(hipMemcpy(scale, n->d_scale, sizeof(float), hipMemcpyDeviceToHost));
    return PTX_OK;
}

int ptx_kat_nn_conv(int device, int w, int h, int cin0, const uint16_t *src0, int upsample, int cin1, const uint16_t *src1, int cout,
                    const float *weights, const float *bias, int relu, int pool, uint16_t *out_half, float *out_f32) {
    const char *fn = "ptx_kat_nn_conv";
    if (w < 1 || h < 1 || w > PTX_NN_MAX_WIDTH || h > PTX_NN_MAX_HEIGHT) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": bad frame size");
    if (cin0 < 1 || cin0 > PT_NN_MAX_CHANNELS || cin1 < 0 || cin1 > PT_NN_MAX_CHANNELS || cout < 1 || cout > PT_NN_MAX_CHANNELS)
        return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": channel counts must be in 1 .. 256 (cin1: 0 .. 256)");
    if (!src0 || !weights || !bias || (cin1 > 0) != (src1 != nullptr) || (!out_half && !out_f32))
        return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": null array (src1 goes with cin1 > 0)");
    if ((upsample || pool) && ((w | h) & 1)) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": upsample and pool need an even w and h");
    if (out_f32 && (pool || cout > 4)) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": out_f32 is the unpooled form with cout <= 4");
    if (const int rc = device_problem(fn, device)) return rc;
    PT_HC(hipSetDevice(device));
    const int c0p = pad16(cin0), c1p = cin1 ? pad16(cin1) : 0, coutp = pad16(cout), cin = cin0 + cin1;
    const size_t px = (size_t)w * h, px0 = upsample ? px / 4 : px, pxo = pool ? px / 4 : px;
    auto padded = [](const uint16_t *src, size_t pixels, int c, int cp) {
        std::vector<uint16_t> v(pixels * cp, 0);
        for (size_t p = 0; p < pixels; p++) memcpy(&v[p * cp], src + p * c, 2 * (size_t)c);
        return v;
    };
    DevBuf<uint16_t> d0, d1, dw, dout;
    DevBuf<float> db, d32;
    PT_HC(d0.upload(padded(src0, px0, cin0, c0p)));
    if (cin1) PT_HC(d1.upload(padded(src1, px, cin1, c1p)));
    std::vector<uint16_t> wp;
    std::vector<float> bp;
    pack_weights(cin0, cin1, cout, [&](int co, int ci, int tap) { return weights[((size_t)co * cin + ci) * 9 + tap]; }, bias, wp, bp);
    PT_HC(dw.upload(wp));
    PT_HC(db.upload(bp));
    PT_HC(dout.alloc(pxo * coutp));
    if (out_f32) PT_HC(d32.alloc(px * 4));
    ConvArgs a;
    a.src0 = d0; a.src1 = cin1 ? d1.p : nullptr; a.w = dw; a.bias = db;
    a.out = out_f32 ? nullptr : dout.p; a.out32 = out_f32 ? d32.p : nullptr;
    a.W = w; a.H = h; a.c0p = c0p; a.c1p = c1p; a.coutp = coutp; a.nchunks = (c0p + c1p + CHUNK - 1) / CHUNK;
    a.upsample = upsample ? 1 : 0; a.pool = pool ? 1 : 0; a.relu = relu ? 1 : 0;
    if (const int rc = launch_conv(nullptr, a, cout)) return rc;
    PT_HC(hipDeviceSynchronize());
    if (out_f32) { PT_HC(d32.download(out_f32)); return PTX_OK; }
    std::vector<uint16_t> got(pxo * coutp);
    PT_HC(dout.download(got.data()));
    for (size_t p = 0; p < pxo; p++) memcpy(out_half + p * cout, &got[p * coutp], 2 * (size_t)cout);
    return PTX_OK;
}

int ptx_kat_nn_transfer(int device, int w, int h, const float *rgb, const float *alb3, const float *nrm3, int hdr, int srgb, float scale,
                        int inverse, float *out9) {
    const char *fn = "ptx_kat_nn_transfer";
    if (w < 1 || h < 1 || w > PTX_NN_MAX_WIDTH || h > PTX_NN_MAX_HEIGHT) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": bad frame size");
    if (!rgb || !out9) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": null array");
    ptx_nn_params p;
    p.hdr = hdr; p.srgb = srgb; p.input_scale = scale;
    if (isnan(scale)) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": scale must be a number");
    if (const char *why = pt_nn_params_problem(p, 1.f)) return pt_fail(PTX_ERR_INVALID, why);
    if (const int rc = device_problem(fn, device)) return rc;
    PT_HC(hipSetDevice(device));
    const int wp = pad16(w), hp = pad16(h);
    const size_t px = (size_t)w * h, pxp = (size_t)wp * hp;
    DevBuf<float> d_scale, d_rgb, d_alb, d_nrm, d_out, d_net;
    DevBuf<uint16_t> d_in;
    PT_HC(d_scale.upload(&scale, 1));
    if (!inverse) {
        PT_HC(d_rgb.upload(rgb, 3 * px));
        if (alb3) PT_HC(d_alb.upload(alb3, 3 * px));
        if (nrm3) PT_HC(d_nrm.upload(nrm3, 3 * px));
        PT_HC(d_in.alloc(pxp * 16));
        PT_HC(d_out.alloc(9 * px));
        InputArgs ia;
        ia.w = w; ia.h = h; ia.wp = wp; ia.hp = hp; ia.x0 = ia.y0 = 0; ia.W = w;
        ia.rgb = d_rgb; ia.alb = alb3 ? d_alb.p : nullptr; ia.nrm = nrm3 ? d_nrm.p : nullptr; ia.alb_stride = ia.nrm_stride = 3;
        ia.samples = 1.f; ia.scale = scale; ia.scale_ptr = nullptr; ia.scale_out = d_scale;
        ia.mode = mode_of(p); ia.hdr = hdr; ia.norm = pu_norm();
        ia.out = d_in; ia.raw = d_out;
        PT_HC(d_out.zero());
        if (const int rc = launch_input(nullptr, ia)) return rc;
    } else {
        std::vector<float> net(4 * pxp, 0.f);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) memcpy(&net[4 * ((size_t)y * wp + x)], rgb + 3 * ((size_t)y * w + x), 3 * sizeof(float));
        PT_HC(d_net.upload(net));
        PT_HC(d_out.alloc(3 * px));
        OutputArgs oa;
        oa.w = w; oa.h = h; oa.wp = wp; oa.ix = oa.iy = oa.ox = oa.oy = 0; oa.W = w; oa.net = d_net; oa.scale = d_scale; oa.mode = mode_of(p); oa.hdr = hdr; oa.xmax = pu_xmax(); oa.out = d_out;
        if (const int rc = launch_output(nullptr, oa)) return rc;
    }
    PT_HC(hipDeviceSynchronize());
    PT_HC(d_out.download(out9));
    return PTX_OK;
}

}  // extern "C"
