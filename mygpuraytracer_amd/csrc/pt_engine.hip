// pt_engine.hip -- the host unit of the MI355X (gfx950) path-tracing engine behind include/mi355x_pathtracer.h: scene upload, the
// tracer's buffers (the ptx_tracer struct itself: pt_tracer.h), the ptx_* entry points that create, render, read and examine a tracer,
// and the kernels that are the same at every arithmetic level (debug capture, cache replay, gather, statistics, preview, G-buffer,
// k_kat_fast_exact, k_hold) with the entry points that launch them.  Scene preparation: pt_scene.hip.
// The debug switches and the launch plans (iterations per set, grids, LDS bytes, the cut of a short run): pt_plan.hip.
// What is done with a traced frame -- the ptx_denoise* entry points, moments, adaptive sampling, the display transform: pt_post.hip.
//
// What belongs here: everything that is level 0 by nature.  This file is compiled ONCE, at the exact level; the kernels whose results
// depend on the arithmetic level (k_bounce, k_mesh, k_finish, the per-stage test kernels) are pt_kernels.hip's, one code object per
// level, and are launched only through that level's table (ptx_tracer::ks) -- see pt_kernels.hip for the engine's design.  The tables
// the host computes with the device's own functions (tabulated normals, ptx_debug_bvh_check's walks) are computed in pt_scene.hip,
// compiled once with this file's flags, and are therefore the exact ones at every level.  What both units must agree on is pt_kernels.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include <atomic>
#include <cmath>

#include "../../include/mi355x_pathtracer.h"
#include "pt_tracer.h"
#include "pt_denoise.h"
#include "pt_adaptive.h"

namespace {

thread_local std::string g_last_error;      // (written through ptx_internal_set_error: pt_fail and PT_HC, pt_handle.h)

// debug capture: the sorted stream materialised -- what the next k_bounce would read, resolved the slow, obvious way from the same
// tables (run prefixes by one thread, a binary search per position), so that the parity tests see the order the kernels define
// without going through k_bounce's own window search.
__global__ void k_capture_prefix(const int32_t *chunk, int chunk_cap, int nruns, int32_t *gs, int32_t *ga) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int s = 0, a = 0;
    for (int r = 0; r < nruns; r++) { gs[r] = s; ga[r] = a; a += chunk[r]; s += chunk[chunk_cap + r]; }
    gs[nruns] = s; ga[nruns] = a;
}
__global__ void k_capture(PathSoA stage, const int32_t *chunk, int chunk_cap, int nruns, const int32_t *gs, const int32_t *ga, int cap,
                          int32_t *out_i, float *out_f, int idx16, int loop_idx, int nbins) {
    // (bin-major index, BounceParams::loop_idx: stage.i is the index itself, the place inside the chunk the entry's low bits)
    const bool loop = (loop_idx & 1) != 0;
    const int n2s = (loop_idx >> 8) & 31;
    const size_t entries = (size_t)nbins << n2s;
    const int n = min(gs[nruns], cap);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        int lo = 0, hi = nruns - 1;                              // last run that starts at or before k
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (gs[mid] <= k) lo = mid; else hi = mid - 1;
        }
        int li = chunk[2 * chunk_cap + lo] + (k - gs[lo]);
        if (loop) li = li < 0 ? 0 : ((size_t)li >= entries ? (int)entries - 1 : li);
        const uint32_t w = (uint32_t)(loop ? stage.i[li] : stage.lsrc()[li]);
        int j = idx16 ? (loop ? li & ((1 << n2s) - 1) : li) + (int)(int16_t)(w & 0xffffu) : (int)w;
        const int rank = idx16 ? (int)(w >> 16) : loop ? stage.i[entries + li] : stage.lidx()[li];
        j = j < 0 ? 0 : (j >= cap ? cap - 1 : j);
        out_i[k] = stage.pix()[j]; out_i[(size_t)cap + k] = ga[lo] + rank; out_i[2 * (size_t)cap + k] = stage.mg()[j];
        for (int f = 0; f < SOA_LOGICAL_FLOATS; f++) out_f[(size_t)f * cap + k] = stage.fieldAt(f, (size_t)j);
    }
}

// replay of the cached bounce-0 light hits (first-bounce cache, iterations > 1)
// add != 0: image[pix] += rgb (one iteration at a time); add == 0: store into the per-iteration radiance buffer of each of
// the nseg segments and set its lit bit (batched mode; a bounce-0 miss sets none, so k_gather adds nothing for it)
__global__ void k_replay_emission(TileMap tm, const int32_t *count, const int32_t *pix, const float *rgb, float *dst, size_t seg_stride,
                                  int nseg, int add, uint32_t cap) {
    int n = *count;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const float r = rgb[k * 3 + 0], g = rgb[k * 3 + 1], b = rgb[k * 3 + 2];
        if (add) {
            float *px = dst + (size_t)slot_to_pixel(tm, pix[k]) * 3;      // dst = the image (pixels), pix[] holds slots
            px[0] += r; px[1] += g; px[2] += b;
        } else {
            for (int sg = 0; sg < nseg; sg++) {
                float *px = dst + seg_stride * sg + (size_t)pix[k] * 3;
                px[0] = r; px[1] = g; px[2] = b;
                set_lit(dst + seg_stride * sg, cap, (uint32_t)pix[k]);
            }
        }
    }
}

// the cached bounce-0 totals into the totals block of every segment of a batch
__global__ void k_seed_totals(int32_t *dst, size_t seg_totals, int nseg, const int32_t *src, int n) {
    for (int k = threadIdx.x; k < n * nseg; k += blockDim.x) dst[seg_totals * (k / n) + (k % n)] = src[k % n];
}

// batched mode: image[pix] += part[0][pix]; += part[1][pix]; ... in iteration order, over the pixels this device owns
// (only the slots whose lit bit of that iteration is set hold anything: see deposit), and the lit planes left zero behind it.
// A wave takes 64 consecutive slots (i0 .. i0 + 63; i0 a multiple of 64, so i0 + 64 <= cap), i.e. two whole words of every plane:
// lane 2s + h (and 64 + 2s + h, nseg > 32) loads word h of plane s -- all of them in one round trip -- and writes the zero back
// if the word held a bit (it needs the value read: the store cannot pass the load).  It is the word's only reader, so no ordering
// between waves is needed.  Each slot's lane then takes its bit of every plane from the lane that holds the word.
__global__ void k_gather(TileMap tm, int resx, int nseg, size_t seg_part, float *part, float *image, uint32_t cap) {
    const int lane = threadIdx.x & 63;
    for (int i0 = (blockIdx.x * blockDim.x + threadIdx.x) & ~63; i0 < tm.owned; i0 += gridDim.x * blockDim.x) {      // (wave-uniform)
        uint32_t *w_lo = lit_flags(part + seg_part * (lane >> 1), cap) + (i0 >> 5) + (lane & 1);      // planes 0 .. 31
        uint32_t *w_hi = lit_flags(part + seg_part * (32 + (lane >> 1)), cap) + (i0 >> 5) + (lane & 1);      // planes 32 .. 63
        const uint32_t lo = lane < 2 * nseg ? *w_lo : 0u, hi = lane + 64 < 2 * nseg ? *w_hi : 0u;
        if (lo) *w_lo = 0u;
        if (hi) *w_hi = 0u;
        const int i = i0 + lane;
        unsigned long long lit = 0;                      // bit s: iteration s of the batch ended this pixel's path on a light (nseg <= 64)
        for (int s = 0; s < nseg; s++) {
            const uint32_t src = s < 32 ? lo : hi;
            const uint32_t w0 = __builtin_amdgcn_readlane(src, (2 * s) & 63), w1 = __builtin_amdgcn_readlane(src, (2 * s + 1) & 63);
            lit |= (unsigned long long)(((lane < 32 ? w0 : w1) >> (lane & 31)) & 1u) << s;
        }
        if (i >= tm.owned || !lit) continue;             // (a pixel no iteration of the batch lit: its sum does not move)
        int x, y;
        owned_pixel(tm, i, x, y);
        const size_t o = ((size_t)x + (size_t)y * resx) * 3;
        float r = image[o], g = image[o + 1], b = image[o + 2];
        const float *pi = part + (size_t)i * 3;
        auto next_lit = [&]() { if (!lit) return -1; const int s = __ffsll((long long)lit) - 1; lit &= lit - 1; return s; };
        auto rgb_of = [&](int s) { const float *ps = pi + seg_part * (size_t)s; return V3(ps[0], ps[1], ps[2]); };
        while (lit) {                                    // in iteration order: the same fp32 sums as one iteration at a time
            // (four segments' loads in flight at once, with the image's: a pixel lit by several iterations -- one that sees the light --
            // is not a chain of dependent round trips)
            const int s0 = next_lit(), s1 = next_lit(), s2 = next_lit(), s3 = next_lit();
            const vec3 z = V3(0.f, 0.f, 0.f);          // (never added: only a segment that is there is)
            const vec3 c0 = rgb_of(s0), c1 = s1 >= 0 ? rgb_of(s1) : z, c2 = s2 >= 0 ? rgb_of(s2) : z, c3 = s3 >= 0 ? rgb_of(s3) : z;
            r += c0.x; g += c0.y; b += c0.z;
            if (s1 >= 0) { r += c1.x; g += c1.y; b += c1.z; }
            if (s2 >= 0) { r += c2.x; g += c2.y; b += c2.z; }
            if (s3 >= 0) { r += c3.x; g += c3.y; b += c3.z; }
        }
        image[o] = r; image[o + 1] = g; image[o + 2] = b;
    }
}

// per-iteration statistics: rays entering the intersect stage of each bounce = sum of totals_all[bounce]
// (bounce 0 is not counted on iterations that took it from the first-bounce cache: nothing was traced -- so the cached bounce-0 records
// that every such iteration RE-READS are not part of stored_* either: the mix describes what was written, once.)
// dir_bins / ntab_bins = the masks the batch's launches wrote with (enqueue_batch: batch_dir_bins), not the tracer's.
// The last reader of the batch's totals: it leaves them zero for the lane's next batch -- the per-bounce totals it has summed, and the
// group totals of bounces 0 .. nbounces - 1 (super_words per segment from super_off: read only by the bounce after the one that wrote
// them), which workgroups 1 .. take.  Launch: dim3(1 + n), dim3(64).
__global__ void k_stats(int32_t *totals, int nbins, int nbounces, int stride, int skip_first, int nseg, size_t seg_totals,
                        size_t super_off, int super_words,
                        int64_t *last, int64_t *total, unsigned long long dir_bins, unsigned long long ntab_bins, int64_t *kinds) {
    if (blockIdx.x != 0) {
        const size_t n = (size_t)nseg * super_words;
        for (size_t k = (size_t)(blockIdx.x - 1) * blockDim.x + threadIdx.x; k < n; k += (size_t)(gridDim.x - 1) * blockDim.x)
            totals[seg_totals * (k / super_words) + super_off + k % super_words] = 0;
        return;
    }
    // one wave: lane j takes the (segment, bounce) pairs j, j + 64, ...
    if (threadIdx.x >= 64) return;
    long long sum = 0, st = 0, sd = 0, sn = 0;      // rays; stored paths: all, with a direction, with a normal code (what the records weigh)
    for (int k = threadIdx.x; k < nseg * nbounces; k += 64) {
        const int sg = k / nbounces, b = k - sg * nbounces;
        long long s = 0;
        if (!(b == 0 && skip_first))
            for (int q = 0; q < nbins; q++) {
                s += totals[seg_totals * sg + (size_t)b * stride + q];
                const long long c = totals[seg_totals * sg + (size_t)b * stride + nbins + q];
                st += c;
                if (nbins > 64 || ((dir_bins >> q) & 1ull)) sd += c;
                if (nbins <= 64 && ((ntab_bins >> q) & 1ull)) sn += c;
            }
        if (sg == nseg - 1 && b < 64) last[b] = s;      // per-bounce counts of the last iteration of the batch
        sum += s;
        for (int q = 0; q < stride; q++) totals[seg_totals * sg + (size_t)b * stride + q] = 0;      // (read: by this lane, just now)
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { sum += __shfl_xor(sum, off); st += __shfl_xor(st, off); sd += __shfl_xor(sd, off); sn += __shfl_xor(sn, off); }
    if (threadIdx.x == 0) {
        atomicAdd(reinterpret_cast<unsigned long long *>(total), (unsigned long long)sum);
        atomicAdd(reinterpret_cast<unsigned long long *>(kinds), (unsigned long long)st);
        atomicAdd(reinterpret_cast<unsigned long long *>(kinds + 1), (unsigned long long)sd);
        atomicAdd(reinterpret_cast<unsigned long long *>(kinds + 2), (unsigned long long)sn);
    }
}

// sendImageToPBO, src/pathtrace.cu:69-89
__global__ void k_pbo(uchar4 *pbo, int n, int iter, const float *image) {
    int index = blockIdx.x * blockDim.x + threadIdx.x;
    if (index < n) {
        const float *pix = image + (size_t)index * 3;
        int c[3];
        for (int k = 0; k < 3; k++) {
            int v = (int)(pix[k] / (float)iter * 255.0);
            c[k] = v < 0 ? 0 : (v > 255 ? 255 : v);
        }
        uchar4 o; o.w = 0; o.x = (unsigned char)c[0]; o.y = (unsigned char)c[1]; o.z = (unsigned char)c[2];
        pbo[index] = o;
    }
}

// every float bit pattern through the guarded core routines and through the compiler's own expansions
__global__ void k_kat_fast_exact(unsigned long long *mism) {
    unsigned long long m0 = 0, m1 = 0, m2 = 0;
    const unsigned long long total = 1ull << 32, step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += step) {
        float x = __uint_as_float((uint32_t)k);
        asm volatile("" : "+v"(x));                          // (the two sides must not be merged into one computation)
        float y = x;
        asm volatile("" : "+v"(y));
        const float a0 = pt_sqrt(x), b0 = __builtin_sqrtf(y);
        const float a1 = pt_rsqrt_glm(x), b1 = 1.0f / __builtin_sqrtf(y);
        // pt_rcp_pos is only ever called with a >= FLT_EPSILON (or NaN): the patterns below that are the caller's business
        const bool dom = !(x < 1.1920928955078125e-07f);
        const float a2 = dom ? pt_rcp_pos(x) : 0.f, b2 = dom ? 1.0f / y : 0.f;
        auto same = [](float p, float q) { return __float_as_uint(p) == __float_as_uint(q) || (p != p && q != q); };
        m0 += same(a0, b0) ? 0 : 1; m1 += same(a1, b1) ? 0 : 1; m2 += same(a2, b2) ? 0 : 1;
    }
    if (m0) atomicAdd(&mism[0], m0);
    if (m1) atomicAdd(&mism[1], m1);
    if (m2) atomicAdd(&mism[2], m2);
}

// G-buffer of the denoiser (ptx_denoise; layout in pt_denoise.h), compiled here only, at the exact level: per pixel the pixel-centre
// pinhole ray (generateRay without jitter or lens, whatever the tracer's options), the path's own intersection (intersectScene, as
// k_kat_intersect: meshes through their BVH), the shade point o + t*d in the order shadeFakeMaterial forms it (src/pathtrace.cu:392),
// the Hit normal (bump-mapped as the intersection returns it) and write_albedo's albedo.  Misses: all zeros.
__global__ __launch_bounds__(256) void k_gbuffer(const DScene sc, const DCamera cam, int traceDepth, float4 *nh, float4 *xt, float4 *alb, int2 *ids) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cam.resx * cam.resy) return;
    const int y = i / cam.resx, x = i - y * cam.resx;
    PathState ps;
    generateRay(cam, 1, traceDepth, /*aa*/ false, /*dof*/ false, x, y, ps);
    Ray r; r.o = ps.o; r.d = ps.d;
    Hit h;
    intersectScene(sc, r, h);
    if (h.t > 0.f) {
        float a[3];
        write_albedo(sc, h, a);
        const vec3 p = add(r.o, scale(r.d, h.t));
        nh[i] = make_float4(h.n.x, h.n.y, h.n.z, 1.f);
        xt[i] = make_float4(p.x, p.y, p.z, h.t);
        alb[i] = make_float4(a[0], a[1], a[2], 0.f);
        ids[i] = make_int2(h.mat, h.geom);
    } else {
        nh[i] = xt[i] = alb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        ids[i] = make_int2(0, 0);
    }
}
}  // namespace

// pt_kat_unit.hip: the known-answer kernels of pt_rsqrt_unit and pt_div_pairs3 (ptx_kat_unit_rsqrt)
namespace ptd { void launch_kat_unit_rsqrt(int cus, hipStream_t stream, unsigned long long *out, int exponent_reps, unsigned long long random_sets); }


namespace {

// field arrays of `stride` elements each (stride = segments x cap: segment s of a field starts at s*cap)
void carve(PathSoA &s, float *f, int32_t *i, size_t stride) {
    s.q = f; s.i = i; s.stride = (uint32_t)stride;
}

PathSoA soa_shift(PathSoA s, size_t off) {       // host side of soa_offset: the same fields `off` elements further
    s.q += 4 * off; s.i += off;
    return s;
}

// multiplier and shift of fastdiv (device) for the divisor d >= 1
void fastdiv_magic(uint32_t d, uint32_t &mul, uint32_t &sh) {
    if (d <= 1) { mul = 0; sh = 255; return; }
    int l = 0;
    while ((1ull << l) < d) l++;
    sh = (uint32_t)(l - 1);
    mul = (uint32_t)(((1ull << (31 + l)) / d) + 1);
}

void ahead_discard(ptx_tracer *t);

// enqueues k_tile_mask (pt_adaptive.hip: this unit holds the tracer's own kernels only) on the tracer's stream: the base table and the
// flags into the effective table, and the flags into the tracer's copy
int apply_tile_mask(ptx_tracer *t, const uint8_t *d_flags) {
    PT_HC(pt_tile_mask_enqueue(t->stream, t->maxTiles, d_flags, t->d_tile_active.p, t->d_tile_geoms.p, t->d_tile_eff.p));
    return PTX_OK;
}

int update_tile_geoms(ptx_tracer *t) {
    t->tile_geoms_valid = false;
    if (!t->cull || t->ngeoms > 32 || t->ngeoms < 1 || t->dbg.no_tile_geoms) return PTX_OK;
    const bool dof = t->opt.depth_of_field != 0;
    if (dof && t->dbg.no_tile_geoms_dof) return PTX_OK;
    std::vector<uint32_t> masks;
    tile_geom_masks(t->cam, t->tm.tile_rows, t->tm.tile_rank, t->tm.tile_world, t->tm.owned, t->maxTiles, t->ngeoms, t->h_aabb.data(), dof, masks);
    PT_HC(hipMemcpyAsync(t->d_tile_geoms, masks.data(), sizeof(uint32_t) * masks.size(), hipMemcpyHostToDevice, t->stream));
    PT_HC(hipStreamSynchronize(t->stream));      // (masks is a local)
    t->tile_geoms_valid = true;
    if (t->mask_set) return apply_tile_mask(t, t->d_tile_active);      // the mask outlives a camera change
    return PTX_OK;
}

int mask_buffers(ptx_tracer *t) {                       // (on the first mask)
    if (t->d_tile_eff) return PTX_OK;
    PT_HC(t->d_tile_active.alloc((size_t)t->maxTiles));
    PT_HC(t->d_tile_eff.alloc((size_t)t->maxTiles));
    return PTX_OK;
}

}  // namespace

// (pt_tracer.h: pt_post.hip's ptx_adaptive_select calls these two)
// why this tracer cannot take a mask of `ntiles` flags (the code through `code`), or NULL
const char *pt_active_tiles_problem(const ptx_tracer *t, int ntiles, int &code) {
    code = PTX_ERR_INVALID;
    if (t->tm.tile_world > 1) return "this tracer renders a row tile (tile_world > 1)";
    if (ntiles != t->maxTiles) return "ntiles differs from ptx_num_tiles";
    code = PTX_ERR_UNSUPPORTED;
    if (!t->tile_geoms_valid) return "this tracer has no per-tile geom table (no_cull, more than 32 geoms, or switched off for debugging)";
    if (t->cache_active()) return "the first-bounce cache replays a camera bounce of the whole frame";
    return nullptr;
}

// the order of a camera change (ptx_set_camera): what is on the tracer's stream ends, what was traced ahead is dropped, then the table
// is written by a launch of its own; d_flags: one byte per tile on the device
int pt_set_tile_mask(ptx_tracer *t, const uint8_t *d_flags) {
    if (const int rc = mask_buffers(t)) return rc;
    PT_HC(hipStreamSynchronize(t->stream));
    ahead_discard(t);
    if (const int rc = apply_tile_mask(t, d_flags ? d_flags : t->d_tile_active.p)) return rc;
    t->mask_set = true;
    return PTX_OK;
}

namespace {

void free_tracer(ptx_tracer *t) {
    if (!t) return;
    hipSetDevice(t->device);
    if (t->stream) hipStreamSynchronize(t->stream);
    for (int l = 1; l < MAX_LANES; l++) if (t->lane_stream[l]) hipStreamSynchronize(t->lane_stream[l]);      // work traced ahead
    delete t;                                            // (buffers, events and streams go with it, in that order: pt_tracer.h)
}

// The specialised variants k_bounce<., ., FAST> hard-wire option values inside the kernel (sort = 1, no cache fill, no albedo, per-
// iteration radiance buffers; the unsplit one also: all scene tables in LDS, no texture, no bump map, no BVH, no depth of field).
// Run outside them they index tables the host sized for OTHER values: with sort_by_material = 0 the host has ONE bin, the kernel
// computes bin = nmats - 1 - material and writes past every per-bin table in LDS and in global memory -- that was round 2's fault
// (gpurun_out/quick_S1.log: an A/B build that took the variant unconditionally; wrong frames on the cache-filling pass and with
// depth of field, then "Memory access fault" on cornellObj with sort_by_material = 0).  So there is ONE predicate, used by every
// launch site: it names the first assumption that does not hold (nullptr: all hold), and launch_bounce refuses -- PTX_ERR_INVALID,
// nothing is launched -- when the variant is asked for regardless (PTX_DEBUG_FORCE_FAST, tests only).
const char *fast_violation(const ptx_tracer *t, int mode, bool first, bool needs_albedo, const BounceParams &bp) {
    if (!bp.part) return "no per-iteration radiance buffers (part == NULL): the variant stores, it never adds to the image";
    if (!bp.sort || bp.nbins != std::max(t->nmats, 1)) return "sort_by_material = 0: the per-bin tables hold one bin";
    if (bp.nbins > 64) return "more than 64 material bins (lane b of a wave owns bin b in the variant's tile epilogue)";
    if (bp.emit_count) return "the cache-filling pass (emit_count != NULL) records bounce-0 light hits";
    if (needs_albedo) return "the launch set contains iteration 1 of the apps variant (albedo AOV)";
    if (!bp.sc.cull || !bp.sc.tri_lds) return "candidate masks or LDS scene tables are off";
    if (bp.sc.cull != 1) return "rays can start beyond CULL_FAR_ORIGIN (far geometry or camera): the pre-test must look at origins";
    if (mode == 0) {
        if (t->split_mesh) return "the scene takes the split mesh search";
        if (first && bp.dof) return "depth of field on the camera-ray bounce";
        if (bp.uses_uv) return "textured scene";
        if (bp.sc.bump_bits) return "bump-mapped mesh";
        if (bp.sc.ntri_lds != bp.sc.ntri) return "triangle tables not staged in LDS";
        if (bp.sc.bvh_root) return "mesh with a BVH";
    } else if (!t->split_mesh || !bp.keys || !bp.items || !bp.item_count) return "not the split mesh search";
    return nullptr;
}

// The light-only variant k_bounce<false, 3, .> stores no path, ranks nothing and leaves no run table: right only for the launch whose paths all
// end (bounce traceDepth - 1), and it finds its rays' candidates through the tile path alone.  The same shape as above: the first
// assumption that does not hold (nullptr: all hold); launch_bounce takes the variant only then.  There is no switch that forces it.
const char *last_violation(const ptx_tracer *t, int mode, bool first, const BounceParams &bp) {
    if (bp.bounce != bp.traceDepth - 1) return "not the last bounce: paths that go on must be ranked and stored";
    if (first) return "the camera bounce (depth 1)";
    if (mode != 0 || t->split_mesh) return "the scene takes the split mesh search";
    if (!bp.sc.cull || !bp.sc.tri_lds) return "candidate masks or LDS scene tables are off";
    if (bp.sc.ngeoms > 32 || bp.sc.ngeoms < 1) return "more than 32 geoms: no bit per geom";
    if (bp.uses_uv) return "textured scene (an emissive texel ends a path where it scatters)";
    if (t->capture_bounce == bp.bounce) return "debug capture of this bounce";
    return nullptr;
}

// the one launch site of k_bounce: picks the variant by the predicates above.  gx_last != 0: the workgroups per segment of the
// light-only variant, where it is taken (it reads the previous launch's run tables and writes none: any grid will do).
int launch_bounce(const ptx_tracer *t, bool first, int mode, bool needs_albedo, dim3 grid, size_t lds, hipStream_t stream, const BounceParams &bp, int gx_last = 0) {
    const char *why = fast_violation(t, mode, first, needs_albedo, bp);
    bool fast = !t->dbg.no_fast && !why;
    if (t->dbg.force_fast) {
        if (why) return pt_fail(PTX_ERR_INVALID, std::string("specialised k_bounce requested outside its preconditions: ") + why);
        fast = true;
    }
    if (!t->dbg.no_last && !last_violation(t, mode, first, bp)) {
        if (gx_last > 0) grid.x = (unsigned)gx_last;
        t->ksl->bounce_last(fast ? 1 : 0, grid, lds, stream, &bp);
        return PTX_OK;
    }
    t->ks->bounce(first ? 1 : 0, mode, fast ? 1 : 0, grid, lds, stream, &bp);
    return PTX_OK;
}

// Enqueues K iterations (iter_first, iter_first + stride, ...) as K segments of every launch: blockIdx.y picks
// the segment, each segment is an independent stream with its own buffers, so the launches carry K times the work
// (what keeps a 1/8-frame tile of a multi-GPU run, or the thin late bounces, from being launch- and tail-bound).
// Lane `lane` works on segments lane*kmax .. of every per-iteration buffer and on its own stream; the image is touched
// only by k_gather, and the gathers of successive batches are chained by events (prev_lane = the lane the previous batch
// ran on), so the fp32 sums happen in iteration order whatever the overlap.
int enqueue_batch_body(ptx_tracer *t, int iter_first, int K, int stride, int lane, int prev_lane, bool defer);
int enqueue_batch(ptx_tracer *t, int iter_first, int K, int stride = 1, int lane = 0, int prev_lane = -1, bool defer = false) {
    const int rc = enqueue_batch_body(t, iter_first, K, stride, lane, prev_lane, defer);
    if (rc != PTX_OK) t->aux_dirty[lane] = true;       // (whatever it had launched may have left bits and totals behind)
    return rc;
}

// The tail of a launch set, or of one segment of a traced-ahead one: the nseg segments from segment seg into the image (k_gather, where
// ending paths stored into per-iteration buffers) and their statistics (k_stats).  Both leave what they read -- the lit planes, the
// totals -- zero behind them.
void launch_gather_stats(ptx_tracer *t, hipStream_t stream, size_t seg, int nseg, bool use_cache, unsigned long long dir_bins, unsigned long long ntab_bins) {
    if (nseg > 1 || t->lanes > 1)
        hipLaunchKernelGGL(k_gather, dim3(std::min(2048, (t->tm.owned + 255) / 256)), dim3(256), 0, stream, t->tm, t->cam.resx, nseg,
                           t->seg_part, t->d_part + seg * t->seg_part, t->d_image, (uint32_t)t->cap);
    const size_t super_off = 2 * (size_t)t->nbins * t->maxBounces;              // (t->d_super's offset in every segment)
    const int super_words = t->traceDepth * 2 * t->nbins * t->nsuper;
    const int nclear = (int)std::min<size_t>(128, ((size_t)nseg * super_words + 255) / 256);
    hipLaunchKernelGGL(k_stats, dim3(1 + nclear), dim3(64), 0, stream, t->d_totals + seg * t->seg_totals, t->nbins, t->traceDepth, 2 * t->nbins,
                       use_cache ? 1 : 0, nseg, t->seg_totals, super_off, super_words, t->d_stats, t->d_stats + 64, dir_bins, ntab_bins, t->d_stats + 66);
}

// per-kernel timing (ptx_set_kernel_timing; costs two event records per launch): begin(kind) in front of a launch, end() behind it
struct KernelTimer {
    ptx_tracer *t;
    hipStream_t stream;
    int begin(int kind) const {
        if (!t->ktiming) return PTX_OK;
        if (t->kev_used + 2 > t->kev.size()) {
            OwnedEvent a, b2;
            PT_HC(a.create()); PT_HC(b2.create());
            t->kev.push_back(std::move(a)); t->kev.push_back(std::move(b2));
        }
        if (t->kev_kind.size() < t->kev.size() / 2) t->kev_kind.resize(t->kev.size() / 2);
        t->kev_kind[t->kev_used / 2] = kind;
        PT_HC(hipEventRecord(t->kev[t->kev_used], stream));
        return PTX_OK;
    }
    int end() const {
        if (!t->ktiming) return PTX_OK;
        PT_HC(hipEventRecord(t->kev[t->kev_used + 1], stream));
        t->kev_used += 2;
        return PTX_OK;
    }
};

// a lane's segments of the per-iteration tables (seg0 = its first segment)
struct SegmentViews {
    int32_t *counts_all, *counts_scat, *chunk, *total, *super;
    size_t chunk_cap, nb, nsuper;
    SegmentViews(const ptx_tracer *t, const BatchPlan &p, size_t seg0)
        : counts_all(t->d_counts + seg0 * p.seg_counts), counts_scat(counts_all + (size_t)t->nbins * t->maxTiles), chunk(t->d_chunk + seg0 * p.seg_chunk),
          total(t->d_totals + seg0 * t->seg_totals), super(t->d_super + seg0 * t->seg_totals), chunk_cap(p.chunk_cap), nb(t->nbins), nsuper(t->nsuper) {}
    // run tables of bounce b: parity b & 1 of the segment's pair (bounce b + 1 reads them while it writes its own)
    int32_t *chunks(int bounce) const { return chunk + (size_t)(bounce & 1) * 3 * chunk_cap; }
    int32_t *totals(int bounce, int which) const { return total + ((size_t)bounce * 2 + which) * nb; }
    int32_t *supers(int bounce, int which) const { return super + ((size_t)bounce * 2 + which) * nb * nsuper; }
};

// what every bounce of one launch set has in common
struct BatchSet {
    int iter_first, K, stride;
    size_t seg0;                                  // the lane's first segment
    bool cache_on, use_cache, fill_cache;         // the first-bounce cache: in use at all / replayed by this set / filled by it
    bool batched;                                 // ending paths store into per-iteration buffers, k_gather sums them
    // what this set's launches WRITE their records with (a debug capture switches the masks off for its own launches); k_stats weighs
    // the set's stored paths by these, not by the tracer's
    unsigned long long dir_bins, ntab_bins;
};

// the parameters of bounce b's launches (the split bounce's three kernels share them)
BounceParams fill_bounce_params(const ptx_tracer *t, const BatchSet &s, const BatchPlan &p, const SegmentViews &v, int b) {
    const bool first = b == 0;
    const size_t seg0 = s.seg0;
    BounceParams bp;
    bp.sc = t->scene(); bp.sc.tri_lds = t->tri_lds; bp.sc.ntri_lds = t->split_mesh ? 0 : t->ntri_lds; bp.sc.cull = t->cull; bp.cam = t->cam; bp.tm = t->tm;
    for (int k = 0; k < 3; k++) if (bp.sc.cull && !(std::fabs(t->cam.position[k]) <= 0.5f * CULL_FAR_ORIGIN)) bp.sc.cull = 2;      // (a camera far out: cullMask, FAR ORIGINS)
    bp.sc.ldsblob = t->d_ldsblob;
    // bounce b writes its stage into soa[1 - (b & 1)] (bounce 0 of a cache-enabled tracer: into soa[2], kept across
    // iterations) and reads the previous bounce's through that bounce's local index and run tables
    const bool from_cache = (b == 1 && s.cache_on), to_cache = (first && s.cache_on);
    bp.in = from_cache ? t->soa[2] : soa_shift(t->soa[b & 1], seg0 * t->cap);
    bp.stage = to_cache ? t->soa[2] : soa_shift(t->soa[1 - (b & 1)], seg0 * t->cap);
    bp.in_totals = first ? nullptr : from_cache ? t->d_cache_totals : v.totals(b - 1, 0);
    bp.in_super = first ? nullptr : from_cache ? t->d_cache_super : v.supers(b - 1, 0);
    bp.in_chunk = first ? nullptr : from_cache ? t->d_cache_chunk : v.chunks(b - 1);
    bp.in_gx = from_cache ? t->cache_gx : (b == 1 ? p.gx_first : p.gx_later);      // workgroups per segment of the launch whose run tables it reads
    bp.seg_in_totals = from_cache ? 0 : t->seg_totals; bp.seg_in_chunk = from_cache ? 0 : p.seg_chunk;
    bp.image = t->d_image;
    bp.iter = s.iter_first; bp.iter_stride = s.stride; bp.traceDepth = t->traceDepth; bp.bounce = b;
    bp.aa = t->opt.antialiasing; bp.dof = t->opt.depth_of_field; bp.sort = t->opt.sort_by_material; bp.uses_uv = t->uses_uv; bp.dir_bins = s.dir_bins;
    bp.ntab_bins = s.ntab_bins; bp.apps = t->opt.apps_variant; bp.albedo = t->d_albedo;
    // (the masks tell the READER of a stage what its records hold; a launch that WRITES with other masks than it reads with -- a cached
    // camera bounce replayed while a debug capture has switched them off, or the other way round -- gets both: in_* for what it reads)
    bp.in_dir_bins = from_cache ? t->cache_dir_bins : bp.dir_bins; bp.in_ntab_bins = from_cache ? t->cache_ntab_bins : bp.ntab_bins;
    // (the local index's form: this launch's, and that of the launch whose stage it reads)
    bp.idx16 = first ? p.idx16_first : p.idx16_later;
    bp.in_idx16 = first ? 0 : from_cache ? t->cache_idx16 : (b == 1 ? p.idx16_first : p.idx16_later);
    // ... and its layout.  Bin-major: the stages' int pointers are the lane's first segment of the index itself (a cached stage's: its one)
    const bool in_loop = first ? false : from_cache ? t->cache_loop : t->ix.loop;
    bp.loop_idx = (t->ix.loop ? 1 : 0) | (in_loop ? 2 : 0) | (t->ix.words == 2 ? 4 : 0) | (t->ix.n2_log2 << 8);
    if (t->ix.loop) {
        bp.in.i = from_cache ? t->d_ibuf[2].p : t->d_ibuf[b & 1] + seg0 * t->ix.seg_words;
        bp.stage.i = to_cache ? t->d_ibuf[2].p : t->d_ibuf[1 - (b & 1)] + seg0 * t->ix.seg_words;
    }
    bp.nbins = t->nbins; bp.maxTiles = t->maxTiles;
    bp.counts_all = v.counts_all; bp.counts_scat = v.counts_scat;
    bp.chunk = to_cache ? t->d_cache_chunk : v.chunks(b); bp.chunk_cap = (int32_t)p.chunk_cap;
    bp.super_all = v.supers(b, 0); bp.super_scat = v.supers(b, 1);
    bp.totals_all = v.totals(b, 0); bp.totals_scat = v.totals(b, 1);
    bp.nsuper = t->nsuper;
    bp.seg_in = from_cache ? 0 : (size_t)t->cap; bp.seg_stage = to_cache ? 0 : (size_t)t->cap;
    bp.seg_counts = p.seg_counts; bp.seg_chunk = to_cache ? 0 : p.seg_chunk; bp.seg_totals = t->seg_totals;
    bp.stamps = t->d_stamps;
    bp.seg_part = t->seg_part;
    bp.part = s.batched ? t->d_part + seg0 * bp.seg_part : nullptr;
    bp.emit_count = (first && s.fill_cache) ? t->d_emit_count : nullptr;
    bp.emit_pix = t->d_emit_pix; bp.emit_rgb = t->d_emit_rgb;
    bp.fenced = reinterpret_cast<unsigned long long *>(t->d_stats + 65); bp.fence_slots_cap = (uint32_t)t->cap;
    bp.fence_slots = t->dbg.fence_slots > 0 ? (uint32_t)std::min<long long>(t->cap, t->dbg.fence_slots) : (uint32_t)t->cap;
    bp.last_inplace = t->dbg.last_inplace ? 1 : 0;
    bp.tile_geoms = (first && t->tile_geoms_valid) ? (t->mask_set ? t->d_tile_eff : t->d_tile_geoms) : nullptr;
    if (t->split_mesh) {
        bp.keys = t->d_keys + seg0 * (size_t)t->cap; bp.seg_keys = (size_t)t->cap;
        bp.items = t->d_items + seg0 * t->seg_items; bp.seg_items = t->seg_items;
        bp.item_count = t->d_item_count + 2 * seg0;          // (a launch set's K counts, then its K cursors: one memset)
        bp.item_cursor = bp.item_count + s.K;
        bp.tile_done = (first && t->d_tile_done) ? t->d_tile_done + seg0 * (size_t)t->maxTiles : nullptr;
    } else {
        bp.keys = nullptr; bp.items = nullptr; bp.item_count = nullptr; bp.item_cursor = nullptr; bp.seg_keys = bp.seg_items = 0; bp.tile_done = nullptr;
    }
    return bp;
}

int enqueue_batch_body(ptx_tracer *t, int iter_first, int K, int stride, int lane, int prev_lane, bool defer) {
    hipStream_t stream = lane == 0 ? t->stream : t->lane_stream[lane];
    const int nb = t->nbins;
    // (the apps variant's albedo AOV is written by iteration 1 alone: only a launch set that contains it needs the general kernel for it)
    const bool needs_albedo = t->d_albedo && iter_first == 1;
    const BatchPlan p = plan_batch(*t, K, defer, needs_albedo);
    BatchSet s;
    s.iter_first = iter_first; s.K = K; s.stride = stride; s.seg0 = (size_t)lane * t->kmax;
    s.cache_on = t->cache_active(); s.use_cache = s.cache_on && t->cache_valid && iter_first != 1; s.fill_cache = s.cache_on && !s.use_cache;
    s.batched = K > 1 || t->lanes > 1;
    const bool masks_off = t->capture_bounce >= 0 && !t->dbg.keep_dir_skip;
    s.dir_bins = masks_off ? ~0ull : t->dir_bins; s.ntab_bins = masks_off ? 0ull : t->ntab_bins;
    const SegmentViews v(t, p, s.seg0);
    const KernelTimer kt{t, stream};
    // per-bounce totals and group totals are accumulated with atomics, and the lit planes are set bit by bit: the lane's previous set
    // left them zero (k_stats, k_gather) -- unless the lane is marked, then all of its segments are cleared here, once
    if (t->aux_dirty[lane]) {
        PT_HC(hipMemsetAsync(v.total, 0, sizeof(int32_t) * t->seg_totals * (size_t)t->kmax, stream));
        if (t->d_part)                               // (the planes: behind each segment's radiance, cap / 32 words per segment)
            PT_HC(hipMemset2DAsync(t->d_part + s.seg0 * t->seg_part + 3 * (size_t)t->cap, sizeof(float) * t->seg_part, 0,
                                      (size_t)t->cap / 8, (size_t)t->kmax, stream));
        t->aux_dirty[lane] = false;
    }
    if (s.fill_cache) PT_HC(hipMemsetAsync(t->d_emit_count, 0, sizeof(int32_t), stream));
    for (int b = 0; b < t->traceDepth; b++) {
        const bool first = b == 0;
        if (first && s.use_cache) {
            // first-bounce cache: the sorted bounce-0 stream and its light hits are identical every iteration
            // when primary rays are not jittered, so bounce 0 is skipped (intent of src/pathtrace.cu:492-499,514)
            // (the cached bounce-0 misses need nothing: their flags were cleared with the batch's)
            hipLaunchKernelGGL(k_seed_totals, dim3(1), dim3(256), 0, stream, v.totals(0, 0), t->seg_totals, K, t->d_cache_totals, 2 * nb);
            if (s.batched)
                hipLaunchKernelGGL(k_replay_emission, dim3(64), dim3(256), 0, stream, t->tm, t->d_emit_count, t->d_emit_pix, t->d_emit_rgb,
                                   t->d_part + s.seg0 * t->seg_part, t->seg_part, K, 0, (uint32_t)t->cap);
            else
                hipLaunchKernelGGL(k_replay_emission, dim3(64), dim3(256), 0, stream, t->tm, t->d_emit_count, t->d_emit_pix, t->d_emit_rgb,
                                   t->d_image, (size_t)0, 1, 1, (uint32_t)t->cap);
            continue;
        }
        const BounceParams bp = fill_bounce_params(t, s, p, v, b);
        const int gx_b = first ? p.gx_first : p.gx_later;                       // this launch's workgroups per segment
        int rc;
        if (t->split_mesh) {       // pass 1 parks the mesh candidates, k_mesh searches them, k_finish shades what it found, pass 2 ranks
            PT_HC(hipMemsetAsync(bp.item_count, 0, sizeof(int32_t) * 2 * (size_t)K, stream));
            if ((rc = kt.begin(first ? 0 : 1)) != PTX_OK) return rc;
            if ((rc = launch_bounce(t, first, 1, needs_albedo, dim3(gx_b, K), p.lds_bounce, stream, bp)) != PTX_OK) return rc;
            if ((rc = kt.end()) != PTX_OK || (rc = kt.begin(2)) != PTX_OK) return rc;
            t->ks->mesh(first ? 1 : 0, dim3(p.mesh_gx, K), p.lds_mesh, stream, &bp, t->bvh_stack);
            t->ks->finish(first ? 1 : 0, dim3(p.finish_gx, K), stream, &bp);
            if ((rc = kt.end()) != PTX_OK || (rc = kt.begin(3)) != PTX_OK) return rc;
            if ((rc = launch_bounce(t, first, 2, needs_albedo, dim3(gx_b, K), p.lds_pass2, stream, bp)) != PTX_OK) return rc;
            if ((rc = kt.end()) != PTX_OK) return rc;
        } else {
            if ((rc = kt.begin(first ? 0 : 1)) != PTX_OK) return rc;
            if ((rc = launch_bounce(t, first, 0, needs_albedo, dim3(gx_b, K), p.lds_bounce, stream, bp, p.gx_last)) != PTX_OK) return rc;
            if ((rc = kt.end()) != PTX_OK) return rc;
        }
        if (first && s.fill_cache) {
            PT_HC(hipMemcpyAsync(t->d_cache_totals, v.totals(0, 0), sizeof(int32_t) * 2 * nb, hipMemcpyDeviceToDevice, stream));
            PT_HC(hipMemcpyAsync(t->d_cache_super, v.supers(0, 0), sizeof(int32_t) * 2 * nb * t->nsuper, hipMemcpyDeviceToDevice, stream));
            t->cache_gx = gx_b;
            t->cache_dir_bins = bp.dir_bins; t->cache_ntab_bins = bp.ntab_bins; t->cache_idx16 = bp.idx16; t->cache_loop = (bp.loop_idx & 1) != 0;
            t->cache_valid = true;
        }
        if (t->capture_bounce == b && t->d_cap && b + 1 < t->traceDepth) {       // (K == 1, lane 0 -- see ptx_render: segment 0 of the buffers)
            int32_t *gs = t->d_cap + 3 * (size_t)t->cap + nb, *ga = gs + p.chunk_cap + 1;
            hipLaunchKernelGGL(k_capture_prefix, dim3(1), dim3(64), 0, stream, bp.chunk, (int)p.chunk_cap, nb * gx_b, gs, ga);
            hipLaunchKernelGGL(k_capture, dim3(std::min(1024, (t->cap + 255) / 256)), dim3(256), 0, stream, bp.stage, bp.chunk, (int)p.chunk_cap,
                               nb * gx_b, gs, ga, t->cap, t->d_cap, t->d_cap_f, bp.idx16, bp.loop_idx, nb);
            PT_HC(hipMemcpyAsync(t->d_cap + 3 * (size_t)t->cap, v.totals(b, 1), sizeof(int32_t) * nb, hipMemcpyDeviceToDevice, stream));
            t->cap_filled = true;
        }
    }
    if (defer) {                                     // render-ahead: gather and statistics follow per iteration (ahead_finish_segment)
        t->ahead[lane].use_cache = s.use_cache;
        t->ahead[lane].dir_bins = s.dir_bins; t->ahead[lane].ntab_bins = s.ntab_bins;
        PT_HC(hipGetLastError());
        return PTX_OK;
    }
    if (prev_lane >= 0 && prev_lane != lane) PT_HC(hipStreamWaitEvent(stream, t->ev_chain[prev_lane], 0));      // the previous batch's gather + stats
    launch_gather_stats(t, stream, s.seg0, K, s.use_cache, s.dir_bins, s.ntab_bins);
    if (t->lanes > 1) PT_HC(hipEventRecord(t->ev_chain[lane], stream));
    PT_HC(hipGetLastError());
    t->iterations += K;
    return PTX_OK;
}

// ---- render-ahead (ptx_iterate) ---------------------------------------------------------------------------------------
// adds the time of the lane's batch, in proportion to the iterations that were taken from it, to the running total
void ahead_fold_time(ptx_tracer *t, int lane) {
    ptx_tracer::Ahead &a = t->ahead[lane];
    if (!a.timed || !a.unfolded || !a.count) { a.unfolded = 0; return; }
    float ms = 0.f;
    if (hipEventSynchronize(t->ev_ahead1[lane]) == hipSuccess && hipEventElapsedTime(&ms, t->ev_ahead0[lane], t->ev_ahead1[lane]) == hipSuccess)
        t->loop_ms_total += (double)ms * a.unfolded / a.count;
    a.unfolded = 0;
}

// forgets what was traced ahead (camera changed, another kind of call came in, the sequence jumped)
void ahead_discard(ptx_tracer *t) {
    for (int l = 1; l < MAX_LANES; l++) {
        if (t->ahead[l].valid || t->ahead[l].unfolded) ahead_fold_time(t, l);
        if (t->ahead[l].valid) t->aux_dirty[l] = true;       // (segments traced and never gathered keep their bits and totals)
        t->ahead[l].valid = false;
    }
    t->ahead_cur = t->ahead_nxt = -1;
    t->last_ahead_lane = -1;
}

bool ahead_possible(const ptx_tracer *t, int iter) {
    if (!t->render_ahead || t->lanes < 3 || t->kmax < 2 || t->ktiming || t->capture_bounce >= 0) return false;
    if (t->cache_active() && (!t->cache_valid || iter == 1)) return false;       // that call fills the first-bounce cache
    return true;
}

// traces iterations first .. first + kmax - 1 on `lane`, gathers nothing yet
int ahead_start(ptx_tracer *t, int lane, int first) {
    hipStream_t ls = t->lane_stream[lane];
    ahead_fold_time(t, lane);                            // the events are about to be re-recorded
    PT_HC(hipEventRecord(t->ev_fork, t->stream));     // after everything on the main stream so far: the cache fill, and the
    PT_HC(hipStreamWaitEvent(ls, t->ev_fork, 0));     // gathers that still read this lane's buffers
    PT_HC(hipEventRecord(t->ev_ahead0[lane], ls));
    int rc = enqueue_batch(t, first, t->kmax, 1, lane, -1, true);
    if (rc != PTX_OK) return rc;
    PT_HC(hipEventRecord(t->ev_ahead1[lane], ls));
    ptx_tracer::Ahead &a = t->ahead[lane];
    a.first = first; a.count = t->kmax; a.next = first; a.unfolded = 0; a.valid = true; a.timed = true;
    return PTX_OK;
}

// one iteration of a traced-ahead batch into the image: what the tail of enqueue_batch does for a whole batch
// (its k_gather and k_stats leave the segment's plane and totals zero, as the tail of a whole batch does)
int ahead_finish_segment(ptx_tracer *t, int lane, int seg) {
    const ptx_tracer::Ahead &a = t->ahead[lane];
    const bool was_dirty = t->aux_dirty[lane];
    t->aux_dirty[lane] = true;                           // (until both are enqueued)
    PT_HC(hipStreamWaitEvent(t->stream, t->ev_ahead1[lane], 0));
    launch_gather_stats(t, t->stream, (size_t)lane * t->kmax + seg, 1, a.use_cache, a.dir_bins, a.ntab_bins);
    PT_HC(hipGetLastError());
    t->aux_dirty[lane] = was_dirty;
    t->iterations += 1;
    return PTX_OK;
}

// The kernel tables of arithmetic level `arith` -- the plain ones (PTX_DEBUG_NO_UNIT_RSQRT) where `plain` -- out of the ten exports of
// the kernel units (pt_tracer.h; a weak one whose object was not linked is null), or the refusal, in the order ptx_create has always
// given them.  (a missing kernel is an error, never a quiet return to the full bounce)
int kernel_tables(int arith, bool plain, const KernelSet **ks, const LastKernelSet **ksl) {
    typedef const void *(*Export)(void);
    static const struct { Export kernels, last; } table[3][2] = {
        {{ptx_arith_kernels_0, ptx_arith_last_0}, {ptx_arith_kernels_0p, ptx_arith_last_0p}},
        {{ptx_arith_kernels_1, ptx_arith_last_1}, {ptx_arith_kernels_1p, ptx_arith_last_1p}},
        {{ptx_arith_kernels_2, ptx_arith_last_2}, {ptx_arith_kernels_2, ptx_arith_last_2}}};      // (level 2 takes the hardware's seeds either way)
    if (arith < 0 || arith > 2) return pt_fail(PTX_ERR_INVALID, "ptx_options.arith: 0 (exact), 1 (contracted) or 2 (fast)");
    const auto get = [](Export f) { return f ? f() : nullptr; };
    const std::string level = std::to_string(arith);
    *ks = static_cast<const KernelSet *>(get(table[arith][0].kernels));
    if (!*ks) return pt_fail(PTX_ERR_UNSUPPORTED, "this library was built without the code object of arithmetic level " + level);
    if ((*ks)->arith != arith) return pt_fail(PTX_ERR_HIP, "arithmetic code object mismatch");
    *ksl = static_cast<const LastKernelSet *>(get(table[arith][0].last));
    if (!*ksl) return pt_fail(PTX_ERR_UNSUPPORTED, "this library was built without the last-bounce code object of arithmetic level " + level);
    if ((*ksl)->arith != arith) return pt_fail(PTX_ERR_HIP, "arithmetic code object mismatch (last bounce)");
    if (!plain) return PTX_OK;
    *ks = static_cast<const KernelSet *>(get(table[arith][1].kernels));
    *ksl = static_cast<const LastKernelSet *>(get(table[arith][1].last));
    if (!*ks || !*ksl) return pt_fail(PTX_ERR_UNSUPPORTED, "PTX_DEBUG_NO_UNIT_RSQRT: this library was built without the plain code objects of arithmetic level " + level);
    if ((*ks)->arith != arith || (*ksl)->arith != arith) return pt_fail(PTX_ERR_HIP, "arithmetic code object mismatch (plain)");
    return PTX_OK;
}

// ptx_create's step 6: the main stream (the caller's, or one of the tracer's own), the loop timing's events and, with more than one
// lane, each lane's stream and events.  The first failure is handed back; what was made by then is the tracer's and goes with it.
hipError_t create_streams_and_events(ptx_tracer *t, hipStream_t callers) {
#define HE(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)
    if (callers) t->stream.borrow(callers);
    else {
        // the main stream carries what a caller waits for (per-call gather, preview, frame read-back) while the other lanes
        // trace ahead in the background: it gets the highest priority, so that those short kernels are not queued behind
        // the bounce kernels' workgroups
        int prio_lo = 0, prio_hi = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) { prio_lo = prio_hi = 0; (void)hipGetLastError(); }
        if (t->dbg.no_priority) prio_hi = prio_lo;
        HE(t->stream.create(hipStreamNonBlocking, prio_hi));
    }
    HE(t->ev_start.create()); HE(t->ev_stop.create());
    if (t->lanes <= 1) return hipSuccess;
    HE(t->ev_fork.create(hipEventDisableTiming));
    for (int l = 0; l < t->lanes; l++) {
        if (l) {
            // every lane at the device's highest priority, like the main stream: measured, not reasoned -- sets of equal
            // priority at that level dispatch 2 % faster than at the default level (C4 wall 0.216 -> 0.211 ms), any
            // mix of levels lies in between, the veneer's per-call loop does not care
            int prio_lo = 0, prio = 0;
            if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio) != hipSuccess || t->dbg.no_priority) { prio = 0; (void)hipGetLastError(); }
            if (t->dbg.has_lane_prio) prio = t->dbg.lane_prio[l];
            HE(t->lane_stream[l].create(hipStreamNonBlocking, prio));
        }
        HE(t->ev_join[l].create(hipEventDisableTiming)); HE(t->ev_chain[l].create(hipEventDisableTiming));
        if (l) { HE(t->ev_ahead0[l].create()); HE(t->ev_ahead1[l].create()); }
    }
    return hipSuccess;
#undef HE
}

}  // namespace

extern "C" {

const char *ptx_last_error(void) { return g_last_error.c_str(); }
void ptx_internal_set_error(const char *msg) { g_last_error = msg ? msg : ""; }

int ptx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void ptx_default_options(ptx_options *o) {
    memset(o, 0, sizeof *o);
    o->depth_of_field = 0; o->cache_first_bounce = 1; o->sort_by_material = 1; o->antialiasing = 1; o->bounding_box = 0;
    o->tile_rows = 0; o->tile_rank = 0; o->tile_world = 1; o->device = -1; o->batch = 0; o->no_lds_triangles = 0; o->apps_variant = 0; o->no_cull = 0;
}

// (kmax_cap > 0: at most that many iterations per launch set, whatever the rule or the option says; *oom = an allocation failed for
// want of memory and *kmax_used iterations per set were being allocated for)
static int create_tracer(int ngeoms, const ptx_geom *geoms, int nmaterials, const ptx_material *materials,
                         const ptx_camera *camera, int trace_depth, const ptx_options *options, float *external_image,
                         void *stream, ptx_tracer **out, int kmax_cap, bool *oom, int *kmax_used);

int ptx_create(int ngeoms, const ptx_geom *geoms, int nmaterials, const ptx_material *materials,
               const ptx_camera *camera, int trace_depth, const ptx_options *options, float *external_image,
               void *stream, ptx_tracer **out) {
    // an out-of-memory failure is retried with half the iterations per launch set (they only set how much is in flight, never what
    // is computed) until one iteration per set does not fit either
    int cap = 0;
    for (;;) {
        bool oom = false;
        int used = 0;
        const int rc = create_tracer(ngeoms, geoms, nmaterials, materials, camera, trace_depth, options, external_image, stream, out, cap, &oom, &used);
        if (rc == PTX_OK || !oom || used <= 1) return rc;
        (void)hipGetLastError();
        cap = used / 2;
    }
}

static int create_tracer(int ngeoms, const ptx_geom *geoms, int nmaterials, const ptx_material *materials,
                         const ptx_camera *camera, int trace_depth, const ptx_options *options, float *external_image,
                         void *stream, ptx_tracer **out, int kmax_cap, bool *oom, int *kmax_used) {
    // ---- 1. the arguments
    if (!out) return pt_fail(PTX_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (ngeoms < 0 || nmaterials < 0 || (ngeoms && !geoms) || (nmaterials && !materials) || !camera)
        return pt_fail(PTX_ERR_INVALID, "missing scene arrays");
    if (camera->resolution[0] <= 0 || camera->resolution[1] <= 0) return pt_fail(PTX_ERR_INVALID, "resolution must be positive");
    if (trace_depth < 1) return pt_fail(PTX_ERR_UNSUPPORTED, "trace depth must be >= 1");
    if (nmaterials >= (1 << BIN_BITS) || ngeoms > 32767) return pt_fail(PTX_ERR_UNSUPPORTED, "more than 65535 materials or 32767 geoms");
    ptx_options opt;
    if (options) opt = *options; else ptx_default_options(&opt);
    if (opt.bounding_box) return pt_fail(PTX_ERR_UNSUPPORTED, "BOUNDING_BOX culling is off in the reference and not implemented");
    if (opt.tile_world < 1) opt.tile_world = 1;
    if (opt.tile_world > 1 && (opt.tile_rows < 1 || opt.tile_rank < 0 || opt.tile_rank >= opt.tile_world))
        return pt_fail(PTX_ERR_INVALID, "bad tile split");
    for (int i = 0; i < ngeoms; i++) {
        if (geoms[i].materialid < 0 || geoms[i].materialid >= nmaterials)
            return pt_fail(PTX_ERR_INVALID, "geom " + std::to_string(i) + " refers to a material that does not exist");
        if (geoms[i].faceSize < 0 || (geoms[i].faceSize > 0 && !geoms[i].faces)) return pt_fail(PTX_ERR_INVALID, "bad face array");
    }
    // ---- 2. the device and the code object of the arithmetic level
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return pt_fail(PTX_ERR_NODEVICE, "no HIP device available; this library has no CPU path");
    int dev = opt.device;
    if (dev < 0) PT_HC(hipGetDevice(&dev));
    if (dev >= ndev) return pt_fail(PTX_ERR_INVALID, "device ordinal out of range");
    PT_HC(hipSetDevice(dev));
    const DebugSwitches dbg = read_debug_switches();     // (once: nothing below, and no later call, looks at the environment again)
    const KernelSet *ks = nullptr; const LastKernelSet *ksl = nullptr;
    if (const int rc = kernel_tables(opt.arith, dbg.no_unit_rsqrt, &ks, &ksl)) return rc;
    ptx_tracer *t = new ptx_tracer;
    auto fail = [&](int code) { free_tracer(t); return code; };      // (sets the device; what the half-made tracer owns goes with it)
#define HC(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { if (e_ == hipErrorOutOfMemory) *oom = true; return fail(pt_fail(PTX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_))); } } while (0)
    t->ks = ks; t->ksl = ksl; t->dbg = dbg;
    t->device = dev; t->opt = opt; t->traceDepth = t->maxBounces = trace_depth; t->ngeoms = ngeoms; t->nmats = nmaterials;
    t->sort_by_material = opt.sort_by_material != 0;
    hipDeviceProp_t prop;
    HC(hipGetDeviceProperties(&prop, dev));
    // ---- 3. tile split: rows owned by this device, and the grid its tiles can use
    camera_to_device(*camera, t->cam);
    const int W = t->cam.resx, H = t->cam.resy;
    t->tm.W = W; t->tm.H = H; t->tm.tile_world = opt.tile_world; t->tm.tile_rank = opt.tile_rank;
    t->tm.tile_rows = opt.tile_world > 1 ? opt.tile_rows : H;
    fastdiv_magic((uint32_t)W, t->tm.w_mul, t->tm.w_sh);
    fastdiv_magic((uint32_t)t->tm.tile_rows, t->tm.rows_mul, t->tm.rows_sh);
    t->tm.owned = owned_pixels(W, H, t->tm.tile_rows, opt.tile_rank, opt.tile_world);
    t->maxTiles = (std::max(t->tm.owned, 1) + TILE - 1) / TILE;
    t->cap = t->maxTiles * TILE;                          // whole tiles: the stage is written tile by tile
    t->nbins = opt.sort_by_material ? (nmaterials > 0 ? nmaterials : 1) : 1;
    t->cus = prop.multiProcessorCount;
    plan_grids(*t);
    t->nsuper = (t->grid_seg + 63) / 64;
    // ---- 4. the scene's tables, on the host (pt_scene.hip)
    HostScene hs;
    if (const int rc = pt_prepare_scene(ngeoms, geoms, nmaterials, materials, opt, t->tm.owned, t->nbins, prop.sharedMemPerBlock, t->dbg.scene, hs)) return fail(rc);
    static_cast<SceneFacts &>(*t) = hs;
    // ---- 5. iterations per launch set, launch sets in flight
    long long ix_budget = 0;
    {
        size_t mem_free = 0, mem_total = 0;
        if (opt.batch <= 0 && hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { mem_free = mem_total = 0; (void)hipGetLastError(); }
        const LaunchPlan plan = plan_launch_sets(t->tm.owned, t->nbins, t->maxTiles, opt, kmax_cap, mem_free, mem_total, t->dbg.mem_budget_mb);
        if (!plan.refusal.empty()) { pt_fail(PTX_ERR_UNSUPPORTED, plan.refusal); return fail(PTX_ERR_UNSUPPORTED); }
        t->kmax = *kmax_used = plan.kmax;
        t->lanes = plan.lanes;
        ix_budget = launch_budget_bytes(mem_free, mem_total, t->dbg.mem_budget_mb);
    }
    // ---- 6. streams and events
    HC(create_streams_and_events(t, (hipStream_t)stream));
    // ---- 7. upload the scene, allocate the streams' buffers
    HC(t->d_geoms.upload(hs.geoms)); HC(t->d_mats.upload(hs.mats)); HC(t->d_faces.upload(hs.faces)); HC(t->d_texels.upload(hs.texels));
    HC(t->d_tri9.upload(hs.tri9)); HC(t->d_gtab.upload(hs.gtab)); HC(t->d_aabb.upload(hs.aabb_ch)); HC(t->d_objcull.upload(hs.objcull));
    HC(t->d_fnorm.upload(hs.fnorm)); HC(t->d_cnorm.upload(hs.cnorm)); HC(t->d_ctan.upload(hs.ctan));
    if (t->bvh_meshes) {
        HC(t->d_bvh_nodes.upload(hs.bvh.nodes)); HC(t->d_bvh_tris.upload(hs.bvh.tris));
        HC(t->d_bvh_root.upload(hs.roots)); HC(t->d_bvh_depth.upload(hs.depths));
        if (!hs.bvh.wide.empty()) {
            HC(t->d_bvh_wide.upload(hs.bvh.wide)); HC(t->d_bvh_wroot.upload(hs.wroots)); HC(t->d_bvh_wneed.upload(hs.wneeds));
        }
    }
    if (t->tri_lds) {
        HC(t->d_ldsblob.alloc(std::max<size_t>(hs.ldsblob.size(), 4)));
        if (!hs.ldsblob.empty()) HC(hipMemcpy(t->d_ldsblob, hs.ldsblob.data(), sizeof(float) * hs.ldsblob.size(), hipMemcpyHostToDevice));
    }
    t->h_aabb = std::move(hs.aabb);                       // (the host keeps corners for the camera tile masks)
    for (const DGeom &g : hs.geoms) t->h_geom_type.push_back(g.type);
    t->has_bvh = t->d_bvh_root != nullptr;
    t->ix = plan_local_index(*t, t->cap, t->tm.owned, t->kmax, ix_budget);      // (behind has_bvh: it asks plan_batch for every set's grids)
    t->h_roots = hs.roots; t->h_depths = hs.depths; t->h_wroots = hs.wroots; t->h_wneeds = hs.wneeds;
    t->h_spec = std::move(hs.h_spec);
    const size_t npix = (size_t)W * H, nseg = (size_t)t->kmax * t->lanes, nb = (size_t)t->nbins;
    if (external_image) t->d_image = external_image;
    else { HC(t->d_image_own.alloc(3 * npix)); HC(t->d_image_own.zero()); t->d_image = t->d_image_own; }
    if (opt.apps_variant) { HC(t->d_albedo.alloc(3 * npix)); HC(t->d_albedo.zero()); }
    t->field_stride = nseg * t->cap;
    for (int k = 0; k < (t->cache_active() ? 3 : 2); k++) {
        const size_t stride = k == 2 ? (size_t)t->cap : t->field_stride;
        HC(t->d_fbuf[k].alloc(SOA_FLOATS * stride));
        // (bin-major index: the ints of a stage are its index alone, nbins x N2 entries per segment)
        HC(t->d_ibuf[k].alloc(t->ix.loop ? t->ix.seg_words * (k == 2 ? 1 : nseg) : SOA_INTS * stride));
        carve(t->soa[k], t->d_fbuf[k], t->d_ibuf[k], stride);
    }
    t->seg_part = 3 * (size_t)t->cap + (size_t)t->cap / 32;     // per-iteration radiance of the OWNED pixels (slot-indexed), whole tiles, then the
                                                                // iteration's lit plane, a bit per slot (cap is a multiple of 256)
    if (nseg > 1) HC(t->d_part.alloc(t->seg_part * nseg));
    for (int l = 0; l < MAX_LANES; l++) t->aux_dirty[l] = true;      // (the planes are not cleared here: each lane's first set does it)
    if (t->split_mesh) {                                  // a queue entry per ray in the worst case
        t->seg_items = (size_t)t->cap;
        HC(t->d_keys.alloc((size_t)t->cap * nseg));
        HC(t->d_items.alloc(t->seg_items * nseg));
        HC(t->d_item_count.alloc(2 * nseg));              // [nseg] counts (pass 1), [nseg] cursors (k_mesh)
        if (!t->dbg.no_first_fusion) { HC(t->d_tile_done.alloc((size_t)t->maxTiles * nseg)); HC(t->d_tile_done.zero()); }
    }
    HC(t->d_counts.alloc((2 * nb + 1) * t->maxTiles * nseg));
    HC(t->d_chunk.alloc(2 * 3 * nb * t->grid_seg * nseg)); HC(t->d_chunk.zero());
    if (t->cache_active()) { HC(t->d_cache_chunk.alloc(3 * nb * t->grid_seg)); HC(t->d_cache_chunk.zero()); }
    t->seg_totals = 2 * nb * t->maxBounces * (1 + (size_t)t->nsuper);
    t->totals_bytes = sizeof(int32_t) * t->seg_totals * nseg;
    HC(t->d_totals.alloc(t->seg_totals * nseg)); HC(t->d_totals.zero());
    t->d_super = t->d_totals + 2 * nb * t->maxBounces;
    HC(t->d_cache_totals.alloc(2 * nb));
    HC(t->d_cache_super.alloc(2 * nb * t->nsuper));
    HC(t->d_emit_count.alloc(1)); HC(t->d_emit_count.zero());
    HC(t->d_emit_pix.alloc((size_t)t->cap));
    HC(t->d_emit_rgb.alloc(3 * (size_t)t->cap));
#if defined(PT_STAMPS) || defined(PT_WGCLOCK)
    HC(t->d_stamps.alloc(48 + 2 * 64 * 4096 * 5)); HC(t->d_stamps.zero());
#endif
    HC(t->d_tile_geoms.alloc((size_t)std::max(t->maxTiles, 1)));
    if (update_tile_geoms(t) != PTX_OK) return fail(PTX_ERR_HIP);
    HC(t->d_stats.alloc(69)); HC(t->d_stats.zero());
#undef HC
    *out = t;
    return PTX_OK;
}

int ptx_create_from_scene(const ptx_scene *s, const ptx_options *options, float *external_image, void *stream, ptx_tracer **out) {
    if (!s) return pt_fail(PTX_ERR_INVALID, "null scene");
    return ptx_create(ptx_scene_num_geoms(s), ptx_scene_geoms(s), ptx_scene_num_materials(s), ptx_scene_materials(s),
                      ptx_scene_camera(const_cast<ptx_scene *>(s)), ptx_scene_trace_depth(s), options, external_image, stream, out);
}

void ptx_destroy(ptx_tracer *t) { free_tracer(t); }

int ptx_set_camera(ptx_tracer *t, const ptx_camera *camera, int trace_depth) {
    if (!t || !camera) return pt_fail(PTX_ERR_INVALID, "null argument");
    if (camera->resolution[0] != t->cam.resx || camera->resolution[1] != t->cam.resy)
        return pt_fail(PTX_ERR_INVALID, "resolution is fixed at create (buffer sizes, src/pathtrace.cu:104-109)");
    if (trace_depth < 1 || trace_depth > t->maxBounces) return pt_fail(PTX_ERR_INVALID, "trace depth exceeds the depth given at create");
    {   // the reference-shaped loop sets the camera before every iteration (src/pathtrace.cu:434-436): the same values
        // again change nothing, so neither the first-bounce cache nor what was traced ahead is thrown away
        DCamera same;
        memcpy(&same, &t->cam, sizeof same);
        camera_to_device(*camera, same);
        if (trace_depth == t->traceDepth && memcmp(&same, &t->cam, sizeof same) == 0) return PTX_OK;
    }
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipStreamSynchronize(t->stream));
    ahead_discard(t);
    camera_to_device(*camera, t->cam);
    t->traceDepth = trace_depth;
    t->cache_valid = false;
    t->gbuf_valid = false;                               // the denoiser's G-buffer is of the old view
    return update_tile_geoms(t);
}

// ---- the active-tile mask (definition in include/mi355x_pathtracer.h) -------------------------------------------------------------
int ptx_tile_pixels(void) { return TILE; }
int ptx_num_tiles(const ptx_tracer *t) { return t ? t->maxTiles : 0; }

int ptx_set_active_tiles(ptx_tracer *t, const uint8_t *host_active, int ntiles) {
    if (!t || !host_active) return pt_fail(PTX_ERR_INVALID, "ptx_set_active_tiles: null tracer or mask");
    int code = 0;
    if (const char *why = pt_active_tiles_problem(t, ntiles, code)) return pt_fail(code, std::string("ptx_set_active_tiles: ") + why);
    PT_HC(hipSetDevice(t->device));
    if (const int rc = mask_buffers(t)) return rc;
    PT_HC(hipStreamSynchronize(t->stream));           // (no launch reads the flags now: only k_tile_mask does, on this stream)
    PT_HC(hipMemcpy(t->d_tile_active, host_active, (size_t)ntiles, hipMemcpyHostToDevice));
    return pt_set_tile_mask(t, nullptr);
}

int ptx_clear_active_tiles(ptx_tracer *t) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "ptx_clear_active_tiles: null tracer");
    if (!t->mask_set) return PTX_OK;
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipStreamSynchronize(t->stream));
    ahead_discard(t);
    t->mask_set = false;
    return PTX_OK;
}

// Every computation of any tracer's G-buffer has a number of its own, from 1 (ptx_tracer::gbuf_serial: what cached clean guides are of)
static uint64_t next_gbuf_serial() {
    static std::atomic<uint64_t> serial{0};
    return ++serial;
}

int ptx_reset_image(ptx_tracer *t) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    if (t->gbuf_serial) t->gbuf_serial = next_gbuf_serial();      // (the G-buffer stays; what was derived from it before the reset is not reused)
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipMemsetAsync(t->d_image, 0, sizeof(float) * 3 * (size_t)t->cam.resx * t->cam.resy, t->stream));
    PT_HC(hipMemsetAsync(t->d_stats, 0, sizeof(int64_t) * 69, t->stream));
    t->iterations = 0; t->loop_ms_total = 0.0; t->cache_valid = false;
    for (int l = 0; l < MAX_LANES; l++) t->aux_dirty[l] = true;
    return PTX_OK;
}

// Experiment hook (PTX_DEBUG_PREQUEUE_US): one lane that holds the main stream for that long, so that the host has queued the whole run
// before its first kernel starts -- what a replayed launch graph would look like from the device's side.  The loop timer starts behind it.
namespace { __global__ void k_hold(long long ticks) { const long long t0 = wall_clock64(); while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32); } }

// the previous ptx_render's time into the running total
static int fold_render_time(ptx_tracer *t) {
    if (!t->timing_valid) return PTX_OK;
    float ms = 0.f;
    PT_HC(hipEventSynchronize(t->ev_stop));
    PT_HC(hipEventElapsedTime(&ms, t->ev_start, t->ev_stop));
    t->loop_ms_total += ms;
    t->timing_valid = false;
    return PTX_OK;
}

int ptx_render(ptx_tracer *t, int iter_first, int count) { return ptx_render_strided(t, iter_first, count, 1); }

int ptx_render_strided(ptx_tracer *t, int iter_first, int count, int stride) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    if (stride < 1) return pt_fail(PTX_ERR_INVALID, "ptx_render_strided: stride must be >= 1");
    if (count <= 0) return PTX_OK;
    PT_HC(hipSetDevice(t->device));
    ahead_discard(t);
    if (const int rc = fold_render_time(t)) return rc;      // (before the events are reused)
    // (the one switch read per call, not at create: tools/gpu_prequeue.py toggles it on a live tracer)
    if (const char *e = getenv("PTX_DEBUG_PREQUEUE_US")) hipLaunchKernelGGL(k_hold, dim3(1), dim3(64), 0, t->stream, (long long)atoi(e) * 100);      // (100 MHz)
    PT_HC(hipEventRecord(t->ev_start, t->stream));
    // per-kernel timing and the debug capture look at one launch set at a time
    const int kb = sets_per_call(count, t->kmax, t->lanes, t->tm.owned, t->dbg.split_min_paths, t->dbg.nsets);
    const int nl = (t->lanes > 1 && !t->ktiming && t->capture_bounce < 0 && count > kb) ? t->lanes : 1;
    auto fork = [&]() -> int {                           // the other lanes start after what is on the main stream so far
        PT_HC(hipEventRecord(t->ev_fork, t->stream));
        for (int l = 1; l < nl; l++) PT_HC(hipStreamWaitEvent(t->lane_stream[l], t->ev_fork, 0));
        return PTX_OK;
    };
    if (nl > 1) { int rc = fork(); if (rc != PTX_OK) return rc; }
    int batch = 0, prev_lane = -1;
    bool used[MAX_LANES] = {};
    const int first_set = t->dbg.first_set;
    for (int k = 0; k < count; batch++) {
        int K = std::min(nl > 1 ? kb : t->kmax, count - k);
        if (nl > 1 && first_set > 0 && count <= 2 * t->kmax) K = std::min(batch == 0 ? std::min(first_set, t->kmax) : t->kmax, count - k);
        if (t->capture_bounce >= 0) K = 1;                        // the debug capture looks at one stream
        if (t->cache_active() && (!t->cache_valid || iter_first + k * stride == 1)) K = 1;
        const int lane = nl > 1 ? batch % nl : 0;
        const bool fills = t->cache_active() && (!t->cache_valid || iter_first + k * stride == 1);
        int rc = enqueue_batch(t, iter_first + k * stride, K, stride, lane, nl > 1 ? prev_lane : -1);
        if (rc != PTX_OK) return rc;
        if (fills && nl > 1 && lane == 0) {              // the other lanes must not read the cache before it is written
            rc = fork();
            if (rc != PTX_OK) return rc;
        }
        used[lane] = true;
        prev_lane = lane;
        k += K;
    }
    for (int l = 1; l < nl; l++)
        if (used[l]) {
            PT_HC(hipEventRecord(t->ev_join[l], t->lane_stream[l]));
            PT_HC(hipStreamWaitEvent(t->stream, t->ev_join[l], 0));
        }
    PT_HC(hipEventRecord(t->ev_stop, t->stream));
    t->timing_valid = true;
    return PTX_OK;
}

int ptx_set_render_ahead(ptx_tracer *t, int on) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    if (!on) ahead_discard(t);
    t->render_ahead = on != 0;
    return PTX_OK;
}

int ptx_iterate(ptx_tracer *t, int iter) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    if (!ahead_possible(t, iter)) return ptx_render(t, iter, 1);
    PT_HC(hipSetDevice(t->device));
    if (t->ahead_cur < 0 || !t->ahead[t->ahead_cur].valid || t->ahead[t->ahead_cur].next != iter) {
        // nothing traced ahead for this iteration (first call, or the sequence jumped): start at it
        ahead_discard(t);
        if (const int rc = fold_render_time(t)) return rc;      // (before "previous operation" becomes this call)
        int rc = ahead_start(t, 1, iter);
        if (rc != PTX_OK) return rc;
        t->ahead_cur = 1;
    }
    const int lane = t->ahead_cur;
    ptx_tracer::Ahead &a = t->ahead[lane];
    // keep one batch ahead of the one being consumed, on the other lane
    if (t->ahead_nxt < 0) {
        const int other = lane == 1 ? 2 : 1;
        int rc = ahead_start(t, other, a.first + a.count);
        if (rc != PTX_OK) return rc;
        t->ahead_nxt = other;
    }
    int rc = ahead_finish_segment(t, lane, iter - a.first);
    if (rc != PTX_OK) return rc;
    a.next++; a.unfolded++;
    t->last_ahead_lane = lane;
    if (a.next == a.first + a.count) {                   // used up: on to the batch traced meanwhile
        a.valid = false;
        t->ahead_cur = t->ahead_nxt;
        t->ahead_nxt = -1;
    }
    return PTX_OK;
}

int ptx_synchronize(ptx_tracer *t) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipStreamSynchronize(t->stream));
    return PTX_OK;
}

int ptx_read_image(ptx_tracer *t, float *host_rgb) {
    if (!t || !host_rgb) return pt_fail(PTX_ERR_INVALID, "null argument");
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipMemcpyAsync(host_rgb, t->d_image, sizeof(float) * 3 * (size_t)t->cam.resx * t->cam.resy, hipMemcpyDeviceToHost, t->stream));
    PT_HC(hipStreamSynchronize(t->stream));
    return PTX_OK;
}

// the accumulation buffer back from a checkpoint (W*H*3 floats, the layout ptx_read_image returns)
int ptx_write_image(ptx_tracer *t, const float *host_rgb) {
    if (!t || !host_rgb) return pt_fail(PTX_ERR_INVALID, "null argument");
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipMemcpyAsync(t->d_image, host_rgb, sizeof(float) * 3 * (size_t)t->cam.resx * t->cam.resy, hipMemcpyHostToDevice, t->stream));
    PT_HC(hipStreamSynchronize(t->stream));
    return PTX_OK;
}

int ptx_read_albedo(ptx_tracer *t, float *host_rgb) {
    if (!t || !host_rgb) return pt_fail(PTX_ERR_INVALID, "null argument");
    if (!t->d_albedo) return pt_fail(PTX_ERR_INVALID, "the albedo AOV exists only with options.apps_variant = 1");
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipMemcpyAsync(host_rgb, t->d_albedo, sizeof(float) * 3 * (size_t)t->cam.resx * t->cam.resy, hipMemcpyDeviceToHost, t->stream));
    PT_HC(hipStreamSynchronize(t->stream));
    return PTX_OK;
}

// sendToGPU + sendDenosiedImageToPBO (apps/src/pathtrace.cu:96-116,673-685): a finished host frame -> 8-bit, no /iter
int ptx_write_denoised_pbo(ptx_tracer *t, const float *host_rgb, uint8_t *host_rgba) {
    if (!t || !host_rgb || !host_rgba) return pt_fail(PTX_ERR_INVALID, "null argument");
    PT_HC(hipSetDevice(t->device));
    const size_t n = (size_t)t->cam.resx * t->cam.resy;
    DevBuf<float> d_in; DevBuf<uchar4> d_out;
    PT_HC(d_in.alloc(3 * n));
    PT_HC(d_out.alloc(n));
    PT_HC(hipMemcpyAsync(d_in, host_rgb, sizeof(float) * 3 * n, hipMemcpyHostToDevice, t->stream));
    hipLaunchKernelGGL(k_pbo, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, t->stream, d_out.p, (int)n, 1, d_in.p);   // iter = 1: pix / 1
    hipError_t e = hipMemcpyAsync(host_rgba, d_out, 4 * n, hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return pt_fail(PTX_ERR_HIP, hipGetErrorString(e));
    return PTX_OK;
}

// sendToGPU itself (apps/src/pathtrace.cu:673-685): host frame in, the preview written to a DEVICE pbo, as the reference's
// mapped GL buffer is
int ptx_write_denoised_pbo_device(ptx_tracer *t, const float *host_rgb, void *device_uchar4) {
    if (!t || !host_rgb) return pt_fail(PTX_ERR_INVALID, "null argument");
    if (!device_uchar4) return PTX_OK;                    // NULL pbo => skip, like ptx_write_pbo_device
    PT_HC(hipSetDevice(t->device));
    const size_t n = (size_t)t->cam.resx * t->cam.resy;
    if (!t->d_denoised) PT_HC(t->d_denoised.alloc(3 * n));      // dev_denoised_output, kept like the reference's
    PT_HC(hipMemcpyAsync(t->d_denoised, host_rgb, sizeof(float) * 3 * n, hipMemcpyHostToDevice, t->stream));
    hipLaunchKernelGGL(k_pbo, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, t->stream, (uchar4 *)device_uchar4, (int)n, 1, t->d_denoised);
    PT_HC(hipGetLastError());
    PT_HC(hipStreamSynchronize(t->stream));            // host_rgb may be reused by the caller right away
    return PTX_OK;
}

float *ptx_device_image(ptx_tracer *t) { return t ? t->d_image : nullptr; }
void *ptx_stream(ptx_tracer *t) { return t ? (void *)t->stream : nullptr; }
int ptx_owned_pixels(const ptx_tracer *t) { return t ? t->tm.owned : 0; }

int ptx_write_pbo_device(ptx_tracer *t, int iter, void *device_uchar4) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    if (!device_uchar4) return PTX_OK;                    // NULL pbo => skip (the reference would fault)
    PT_HC(hipSetDevice(t->device));
    int n = t->cam.resx * t->cam.resy;
    hipLaunchKernelGGL(k_pbo, dim3((n + 255) / 256), dim3(256), 0, t->stream, (uchar4 *)device_uchar4, n, iter, t->d_image);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

int ptx_write_pbo(ptx_tracer *t, int iter, uint8_t *host_rgba) {
    if (!t || !host_rgba) return pt_fail(PTX_ERR_INVALID, "null argument");
    PT_HC(hipSetDevice(t->device));
    size_t n = (size_t)t->cam.resx * t->cam.resy;
    // the staging buffer stays with the tracer: hipFree would wait for the whole device, i.e. for work traced ahead
    if (!t->d_pbo) PT_HC(t->d_pbo.alloc(n));
    int rc = ptx_write_pbo_device(t, iter, t->d_pbo);
    if (rc == PTX_OK) {
        hipError_t e = hipMemcpyAsync(host_rgba, t->d_pbo, n * 4, hipMemcpyDeviceToHost, t->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
        if (e != hipSuccess) rc = pt_fail(PTX_ERR_HIP, hipGetErrorString(e));
    }
    return rc;
}

// ---- denoiser (pt_denoise.hip, pt_temporal.hip; definition in include/mi355x_pathtracer.h) --------------------------------------
// The G-buffer of the current camera on the tracer's stream, buffers allocated on first use
extern "C++" int pt_ensure_gbuffer(ptx_tracer *t) {
    const size_t n = (size_t)t->cam.resx * t->cam.resy;
    if (!t->d_gbuf) PT_HC(t->d_gbuf.alloc(3 * n + (n + 1) / 2));      // (+ the ids: an int2 per pixel)
    if (t->gbuf_valid) return PTX_OK;
    t->gbuf_serial = next_gbuf_serial();
    const DScene sc = t->scene();
    if (t->guide_bounces > 0) {                         // either mode followed through mirrors and glass (pt_guides_follow.hip): the same arrays
        const bool sampled = t->guide_count > 0;         // (the pixel-centre mode: one ray, no jitter, no lens -- k_gbuffer's ray)
        const int beff = std::max(std::min(t->guide_bounces, t->traceDepth - 1), 0);      // a path of depth d has at most d segments
        PT_HC(pt_guides_follow_enqueue(t->stream, sc, t->cam, t->traceDepth, sampled ? t->opt.antialiasing : 0, sampled ? t->opt.depth_of_field : 0,
                                          sampled ? t->guide_first : 1, sampled ? t->guide_count : 1, beff,
                                          t->d_gbuf, t->d_gbuf + n, t->d_gbuf + 2 * n, reinterpret_cast<int2 *>(t->d_gbuf + 3 * n)));
        t->gbuf_valid = true;
        return PTX_OK;
    }
    if (t->guide_count > 0) {                            // sampled guides (pt_guides.hip): the same arrays, the coverage in alb.w
        PT_HC(pt_guides_enqueue(t->stream, sc, t->cam, t->traceDepth, t->opt.antialiasing, t->opt.depth_of_field, t->guide_first, t->guide_count,
                                   t->d_gbuf, t->d_gbuf + n, t->d_gbuf + 2 * n, reinterpret_cast<int2 *>(t->d_gbuf + 3 * n)));
        t->gbuf_valid = true;
        return PTX_OK;
    }
    hipLaunchKernelGGL(k_gbuffer, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, t->stream, sc, t->cam, t->traceDepth,
                       t->d_gbuf, t->d_gbuf + n, t->d_gbuf + 2 * n, reinterpret_cast<int2 *>(t->d_gbuf + 3 * n));
    PT_HC(hipGetLastError());
    t->gbuf_valid = true;
    return PTX_OK;
}

static_assert(sizeof(DCamera) == sizeof(ptx_camera), "camera layout");

// ---- sampled guides (pt_guides.hip; definition in include/mi355x_pathtracer.h) ------------------------------------------------------
static const int GUIDE_SAMPLES_MAX = 4096;
int ptx_set_guide_samples(ptx_tracer *t, int iter_first, int count) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "ptx_set_guide_samples: null tracer");
    if (iter_first < 1) return pt_fail(PTX_ERR_INVALID, "ptx_set_guide_samples: iter_first must be >= 1 (iterations count from 1)");
    if (count < 0) return pt_fail(PTX_ERR_INVALID, "ptx_set_guide_samples: count must be >= 0 (0: the pixel-centre guides)");
    if (count > GUIDE_SAMPLES_MAX)
        return pt_fail(PTX_ERR_INVALID, "ptx_set_guide_samples: count " + std::to_string(count) + " exceeds the cap of " +
                                              std::to_string(GUIDE_SAMPLES_MAX) + " samples per pixel");
    if (iter_first > INT32_MAX - GUIDE_SAMPLES_MAX)
        return pt_fail(PTX_ERR_INVALID, "ptx_set_guide_samples: iter_first + count would pass the largest iteration number");
    if (const int rc = pt_whole_frame_problem("ptx_set_guide_samples", t)) return rc;
    if (count == t->guide_count && (count == 0 || iter_first == t->guide_first)) return PTX_OK;      // (the same guides: nothing is stale)
    t->guide_first = iter_first; t->guide_count = count;
    t->gbuf_valid = false;
    return PTX_OK;
}

int ptx_get_guide_samples(const ptx_tracer *t, int *iter_first, int *count) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "ptx_get_guide_samples: null tracer");
    if (iter_first) *iter_first = t->guide_first;
    if (count) *count = t->guide_count;
    return PTX_OK;
}

// ---- guides through mirrors and glass (pt_guides_follow.hip; definition in include/mi355x_pathtracer.h) -------------------------------
static const int GUIDE_BOUNCES_MAX = 64;
int ptx_set_guide_bounces(ptx_tracer *t, int bounces) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "ptx_set_guide_bounces: null tracer");
    if (bounces < 0) return pt_fail(PTX_ERR_INVALID, "ptx_set_guide_bounces: bounces must be >= 0 (0: the first surface)");
    if (bounces > GUIDE_BOUNCES_MAX)
        return pt_fail(PTX_ERR_INVALID, "ptx_set_guide_bounces: bounces " + std::to_string(bounces) + " exceeds the cap of " +
                                              std::to_string(GUIDE_BOUNCES_MAX) + " continuations per ray");
    if (const int rc = pt_whole_frame_problem("ptx_set_guide_bounces", t)) return rc;
    if (bounces == t->guide_bounces) return PTX_OK;      // (the same guides: nothing is stale)
    t->guide_bounces = bounces;
    t->gbuf_valid = false;
    return PTX_OK;
}

int ptx_get_guide_bounces(const ptx_tracer *t, int *bounces) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "ptx_get_guide_bounces: null tracer");
    if (bounces) *bounces = t->guide_bounces;
    return PTX_OK;
}

int ptx_write_denoised_pbo_from_device(ptx_tracer *t, void *device_uchar4) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    if (!t->dn_done) return pt_fail(PTX_ERR_INVALID, "ptx_write_denoised_pbo_from_device: no ptx_denoise on this tracer yet");
    if (!device_uchar4) return PTX_OK;                    // NULL pbo => skip, like ptx_write_pbo_device
    PT_HC(hipSetDevice(t->device));
    const int n = t->cam.resx * t->cam.resy;
    hipLaunchKernelGGL(k_pbo, dim3((n + 255) / 256), dim3(256), 0, t->stream, (uchar4 *)device_uchar4, n, 1, t->d_dn_out);   // iter = 1: no /iter
    PT_HC(hipGetLastError());
    return PTX_OK;
}

int ptx_read_gbuffer(ptx_tracer *t, float *pos3, float *nrm3, float *alb3, int32_t *ids2, float *t1, uint8_t *hit1) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    if (t->tm.tile_world > 1)
        return pt_fail(PTX_ERR_INVALID, "ptx_read_gbuffer: this tracer renders a row tile (tile_world > 1); the denoiser needs the whole frame");
    PT_HC(hipSetDevice(t->device));
    const int rc = pt_ensure_gbuffer(t);
    if (rc != PTX_OK) return rc;
    const size_t n = (size_t)t->cam.resx * t->cam.resy;
    std::vector<float4> g(3 * n);
    std::vector<int2> ids(n);
    PT_HC(hipMemcpyAsync(g.data(), t->d_gbuf, sizeof(float4) * 3 * n, hipMemcpyDeviceToHost, t->stream));
    PT_HC(hipMemcpyAsync(ids.data(), t->d_gbuf + 3 * n, sizeof(int2) * n, hipMemcpyDeviceToHost, t->stream));
    PT_HC(hipStreamSynchronize(t->stream));
    for (size_t i = 0; i < n; i++) {
        const float4 &nh = g[i], &xt = g[n + i], &al = g[2 * n + i];
        if (pos3) { pos3[3 * i] = xt.x; pos3[3 * i + 1] = xt.y; pos3[3 * i + 2] = xt.z; }
        if (nrm3) { nrm3[3 * i] = nh.x; nrm3[3 * i + 1] = nh.y; nrm3[3 * i + 2] = nh.z; }
        if (alb3) { alb3[3 * i] = al.x; alb3[3 * i + 1] = al.y; alb3[3 * i + 2] = al.z; }
        if (ids2) { ids2[2 * i] = ids[i].x; ids2[2 * i + 1] = ids[i].y; }
        if (t1) t1[i] = xt.w;
        if (hit1) hit1[i] = nh.w != 0.f ? 1 : 0;
    }
    return PTX_OK;
}

int ptx_read_guide_coverage(ptx_tracer *t, float *coverage1) {
    if (!t || !coverage1) return pt_fail(PTX_ERR_INVALID, "ptx_read_guide_coverage: null tracer or buffer");
    if (const int rc = pt_whole_frame_problem("ptx_read_guide_coverage", t)) return rc;
    PT_HC(hipSetDevice(t->device));
    if (const int rc = pt_ensure_gbuffer(t)) return rc;
    const size_t n = (size_t)t->cam.resx * t->cam.resy;
    // the fourth float of the albedo records; the pixel-centre guides write 0 there, their coverage is the hit flag: nh's fourth float
    std::vector<float4> a(n);
    PT_HC(hipMemcpyAsync(a.data(), t->d_gbuf + (t->guide_count > 0 ? 2 * n : 0), sizeof(float4) * n, hipMemcpyDeviceToHost, t->stream));
    PT_HC(hipStreamSynchronize(t->stream));
    for (size_t i = 0; i < n; i++) coverage1[i] = a[i].w;
    return PTX_OK;
}

double ptx_last_loop_ms(ptx_tracer *t) {
    if (!t) return 0.0;
    if (t->last_ahead_lane >= 0) {                       // a call served from a batch traced ahead: its share of that batch
        const ptx_tracer::Ahead &a = t->ahead[t->last_ahead_lane];
        float ms = 0.f;
        hipSetDevice(t->device);
        if (!a.count || hipEventSynchronize(t->ev_ahead1[t->last_ahead_lane]) != hipSuccess) return 0.0;
        if (hipEventElapsedTime(&ms, t->ev_ahead0[t->last_ahead_lane], t->ev_ahead1[t->last_ahead_lane]) != hipSuccess) return 0.0;
        return (double)ms / a.count;
    }
    if (!t->timing_valid) return 0.0;
    hipSetDevice(t->device);
    float ms = 0.f;
    if (hipEventSynchronize(t->ev_stop) != hipSuccess) return 0.0;
    if (hipEventElapsedTime(&ms, t->ev_start, t->ev_stop) != hipSuccess) return 0.0;
    return (double)ms;
}

int ptx_get_stats(ptx_tracer *t, ptx_stats *out) {
    if (!t || !out) return pt_fail(PTX_ERR_INVALID, "null argument");
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipStreamSynchronize(t->stream));
    int64_t h[69];
    PT_HC(hipMemcpy(h, t->d_stats, sizeof h, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->bounces = t->traceDepth;
    for (int b = 0; b < 64 && b < t->traceDepth; b++) out->rays_per_bounce[b] = h[b];
    out->rays_total = h[64];
    out->fenced = h[65];
    out->stored_paths = h[66]; out->stored_with_direction = h[67]; out->stored_with_normal_code = h[68];
    for (int l = 1; l < MAX_LANES; l++) ahead_fold_time(t, l);
    out->loop_ms_total = t->loop_ms_total + (t->last_ahead_lane >= 0 ? 0.0 : ptx_last_loop_ms(t));
    out->iterations = t->iterations;
    return PTX_OK;
}

int ptx_get_stats_sized(ptx_tracer *t, void *out, size_t out_bytes) {
    if (!t || !out) return pt_fail(PTX_ERR_INVALID, "null argument");
    ptx_stats s;
    const int rc = ptx_get_stats(t, &s);
    if (rc != PTX_OK) return rc;
    memset(out, 0, out_bytes);
    memcpy(out, &s, std::min(out_bytes, sizeof s));
    return PTX_OK;
}

int ptx_abi_version(void) { return PTX_ABI_VERSION; }
size_t ptx_sizeof_options(void) { return sizeof(ptx_options); }
size_t ptx_sizeof_stats(void) { return sizeof(ptx_stats); }

// ---- per-stage entry points -----------------------------------------------------------------------------------
#define KAT_PROLOGUE                                                        \
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");               \
    PT_HC(hipSetDevice(t->device));                                      \
    PT_HC(hipStreamSynchronize(t->stream));

// n rays against one geom, `width` floats out per ray: the whole intersection test (10) or its triangle part (8)
static int kat_rays(ptx_tracer *t, int geom, int n, const float *rays6, float *out, int width) {
    KAT_PROLOGUE
    if (geom < 0 || geom >= t->ngeoms) return pt_fail(PTX_ERR_INVALID, "geom index out of range");
    if (n <= 0) return PTX_OK;
    DevBuf<float> d_in, d_out;
    PT_HC(d_in.upload(rays6, 6 * (size_t)n));
    PT_HC(d_out.alloc(width * (size_t)n));
    { const DScene sc = t->scene(); (width == 10 ? t->ks->kat_geom : t->ks->kat_obj_tri)(dim3((n + 255) / 256), t->stream, &sc, geom, n, d_in, d_out); }
    PT_HC(hipStreamSynchronize(t->stream));
    PT_HC(d_out.download(out));
    return PTX_OK;
}
int ptx_kat_geom_test(ptx_tracer *t, int geom, int n, const float *rays6, float *out10) { return kat_rays(t, geom, n, rays6, out10, 10); }
int ptx_kat_obj_tri_test(ptx_tracer *t, int geom, int n, const float *rays6, float *out8) { return kat_rays(t, geom, n, rays6, out8, 8); }

int ptx_kat_jittered_hemisphere(ptx_tracer *t, int n, const float *normals3, const int32_t *seeds3, int max_iter, float *out3) {
    KAT_PROLOGUE
    if (n <= 0) return PTX_OK;
    if (max_iter < 1) return pt_fail(PTX_ERR_INVALID, "max_iter must be >= 1");
    DevBuf<float> d_n, d_o; DevBuf<int32_t> d_s;
    PT_HC(d_n.upload(normals3, 3 * (size_t)n)); PT_HC(d_o.alloc(3 * (size_t)n)); PT_HC(d_s.upload(seeds3, 3 * (size_t)n));
    t->ks->kat_jittered(dim3((n + 255) / 256), t->stream, n, d_n.p, d_s.p, max_iter, d_o.p);
    PT_HC(hipStreamSynchronize(t->stream));
    PT_HC(d_o.download(out3));
    return PTX_OK;
}

int ptx_kat_compute_intersections(ptx_tracer *t, int n, const void *paths44, void *isects32) {
    KAT_PROLOGUE
    if (n <= 0) return PTX_OK;
    DevBuf<HostPath> d_p; DevBuf<HostIsect> d_i;
    PT_HC(d_p.upload(paths44, (size_t)n));
    PT_HC(d_i.alloc((size_t)n));
    { const DScene sc = t->scene(); t->ks->kat_intersect(dim3((n + 255) / 256), t->stream, &sc, n, d_p.p, d_i.p); }
    PT_HC(hipStreamSynchronize(t->stream));
    PT_HC(d_i.download(isects32));
    return PTX_OK;
}

int ptx_kat_tile_intersect(ptx_tracer *t, int n, const void *paths44, void *isects32, int split) {
    KAT_PROLOGUE
    if (n <= 0) return PTX_OK;
    if (!t->cull || !t->tri_lds) return pt_fail(PTX_ERR_UNSUPPORTED, "this scene does not take the tile path (candidate masks / LDS tables are off)");
    if (split && !t->d_bvh_root) return pt_fail(PTX_ERR_UNSUPPORTED, "no mesh of this scene has a BVH: nothing for the split mesh search to do");
    DevBuf<HostPath> d_p; DevBuf<HostIsect> d_i;
    PT_HC(d_p.upload(paths44, (size_t)n));
    PT_HC(d_i.alloc((size_t)n));
    // the scene as enqueue_batch hands it to k_bounce (tables staged; split: without the triangle tables) and as k_mesh gets it
    DScene sc = t->scene();
    sc.tri_lds = t->tri_lds; sc.ntri_lds = (split || t->split_mesh) ? 0 : t->ntri_lds; sc.cull = t->cull ? 2 : 0;      // (the caller's rays can start anywhere: cullMask, FAR ORIGINS)
    sc.ldsblob = (split || t->split_mesh) == t->split_mesh ? t->d_ldsblob : nullptr;      // (the blob is laid out for the tracer's own choice)
    DScene scg = t->scene();
    scg.bvh_stack = t->bvh_stack;
    const size_t lds = sizeof(int32_t) * (bounceLdsWords(sceneTableWords(sc.ntri_lds, t->nmats, t->ngeoms), 1) + (split ? (size_t)t->bvh_stack * TILE : 0));
    {   // ptx_create sized k_bounce's LDS against the device (stepping the tables down where needed); this kernel adds the walks'
        // stacks on top of the same layout, so it is checked here, where the caller can be told, not at the launch
        int lim = 0;
        PT_HC(hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, t->device));
        if (lds > (size_t)lim)
            return pt_fail(PTX_ERR_UNSUPPORTED, "ptx_kat_tile_intersect needs " + std::to_string(lds) + " bytes of LDS per workgroup (scene tables + " +
                             std::to_string(t->bvh_stack) + " stack entries per lane), the device offers " + std::to_string(lim));
    }
    const dim3 grid((unsigned)std::min(1024, (n + TILE - 1) / TILE));
    t->ks->kat_tile(split ? 1 : 0, grid, lds, t->stream, &sc, &scg, n, d_p.p, d_i.p, t->uses_uv);
    PT_HC(hipGetLastError());
    PT_HC(hipStreamSynchronize(t->stream));
    PT_HC(d_i.download(isects32));
    return PTX_OK;
}

int ptx_kat_shade(ptx_tracer *t, int iter, int n, const int32_t *idx, const void *isects32, void *paths44) {
    KAT_PROLOGUE
    if (n <= 0) return PTX_OK;
    DevBuf<HostPath> d_p; DevBuf<HostIsect> d_i; DevBuf<int32_t> d_x;
    PT_HC(d_p.upload(paths44, (size_t)n)); PT_HC(d_i.upload(isects32, (size_t)n)); PT_HC(d_x.upload(idx, (size_t)n));
    { const DScene sc = t->scene(); t->ks->kat_shade(dim3((n + 255) / 256), t->stream, &sc, iter, n, d_x.p, d_i.p, d_p.p); }
    PT_HC(hipStreamSynchronize(t->stream));
    PT_HC(d_p.download(paths44));
    return PTX_OK;
}

int ptx_kat_generate(ptx_tracer *t, int iter, void *paths44) {
    KAT_PROLOGUE
    int n = t->cam.resx * t->cam.resy;
    DevBuf<HostPath> d_p;
    PT_HC(d_p.alloc((size_t)n));
    t->ks->kat_generate(dim3((n + 255) / 256), t->stream, &t->cam, iter, t->traceDepth, t->opt.antialiasing, t->opt.depth_of_field, d_p.p);
    PT_HC(hipStreamSynchronize(t->stream));
    PT_HC(d_p.download(paths44));
    return PTX_OK;
}

int ptx_kat_libm(ptx_tracer *t, int n, const float *x, float *sin_out, float *cos_out, const double *pw_in,
                 double *pow5_out, const float *powf_xy, float *powf_out) {
    KAT_PROLOGUE
    if (n <= 0) return PTX_OK;
    DevBuf<float> dx, ds, dc, dxy, dpo; DevBuf<double> dpw, dp5;
    PT_HC(dx.upload(x, (size_t)n)); PT_HC(ds.alloc((size_t)n)); PT_HC(dc.alloc((size_t)n));
    PT_HC(dxy.upload(powf_xy, 2 * (size_t)n)); PT_HC(dpo.alloc((size_t)n));
    PT_HC(dpw.upload(pw_in, (size_t)n)); PT_HC(dp5.alloc((size_t)n));
    t->ks->kat_libm(dim3((n + 255) / 256), t->stream, n, dx.p, ds.p, dc.p, dpw.p, dp5.p, dxy.p, dpo.p);
    PT_HC(hipStreamSynchronize(t->stream));
    PT_HC(ds.download(sin_out)); PT_HC(dc.download(cos_out)); PT_HC(dp5.download(pow5_out)); PT_HC(dpo.download(powf_out));
    return PTX_OK;
}

int ptx_kat_fast_exact(ptx_tracer *t, int64_t mismatches[3]) {
    KAT_PROLOGUE
    if (!mismatches) return pt_fail(PTX_ERR_INVALID, "null argument");
    DevBuf<unsigned long long> d;
    PT_HC(d.alloc(3));
    PT_HC(hipMemsetAsync(d.p, 0, 3 * sizeof(unsigned long long), t->stream));
    hipLaunchKernelGGL(k_kat_fast_exact, dim3(t->cus * 8), dim3(256), 0, t->stream, d.p);
    PT_HC(hipGetLastError());
    PT_HC(hipStreamSynchronize(t->stream));
    unsigned long long h[3];
    PT_HC(d.download(h));
    for (int k = 0; k < 3; k++) mismatches[k] = (int64_t)h[k];
    return PTX_OK;
}

int ptx_kat_unit_rsqrt(ptx_tracer *t, int exponent_reps, int64_t random_sets, int64_t counts[4]) {
    KAT_PROLOGUE
    if (!counts || exponent_reps < 0 || random_sets < 0) return pt_fail(PTX_ERR_INVALID, "bad argument");
    DevBuf<unsigned long long> d;
    PT_HC(d.alloc(4));
    PT_HC(hipMemsetAsync(d.p, 0, 4 * sizeof(unsigned long long), t->stream));
    launch_kat_unit_rsqrt(t->cus, t->stream, d.p, exponent_reps, (unsigned long long)random_sets);
    PT_HC(hipGetLastError());
    PT_HC(hipStreamSynchronize(t->stream));
    unsigned long long h[4];
    PT_HC(d.download(h));
    for (int k = 0; k < 4; k++) counts[k] = (int64_t)h[k];
    return PTX_OK;
}

int ptx_set_kernel_timing(ptx_tracer *t, int on) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipStreamSynchronize(t->stream));
    ahead_discard(t);
    t->ktiming = on != 0;
    t->kev_used = 0;
    return PTX_OK;
}

int ptx_get_kernel_times(ptx_tracer *t, double ms_by_kind[4], int64_t launches_by_kind[4]) {
    if (!t || !ms_by_kind || !launches_by_kind) return pt_fail(PTX_ERR_INVALID, "null argument");
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipStreamSynchronize(t->stream));
    for (int k = 0; k < 4; k++) { ms_by_kind[k] = 0.0; launches_by_kind[k] = 0; }
    for (size_t i = 0; i + 1 < t->kev_used; i += 2) {
        float ms = 0.f;
        PT_HC(hipEventElapsedTime(&ms, t->kev[i], t->kev[i + 1]));
        int kind = t->kev_kind[i / 2];
        ms_by_kind[kind] += ms; launches_by_kind[kind]++;
    }
    t->kev_used = 0;
    return PTX_OK;
}

// diagnostic build (-DPT_STAMPS): cycles per phase of k_bounce summed over waves: [0..4] first bounce, [8..12] later bounces
int ptx_debug_read_stamps(ptx_tracer *t, unsigned long long out48[48]) {
    if (!t || !out48) return pt_fail(PTX_ERR_INVALID, "null argument");
    memset(out48, 0, sizeof(unsigned long long) * 48);
    if (!t->d_stamps) return PTX_OK;
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipStreamSynchronize(t->stream));
    PT_HC(hipMemcpy(out48, t->d_stamps, sizeof(unsigned long long) * 48, hipMemcpyDeviceToHost));
    {   // -DPT_WGCLOCK: the per-workgroup wall-clock slots summed per kind into [32..36] (first bounce) and [40..44] (later bounces)
        std::vector<unsigned long long> w((size_t)2 * 64 * 4096 * 5);
        PT_HC(hipMemcpy(w.data(), t->d_stamps + 48, sizeof(unsigned long long) * w.size(), hipMemcpyDeviceToHost));
        for (int kind = 0; kind < 2; kind++)
            for (size_t k = 0; k < (size_t)64 * 4096; k++)
                for (int f = 0; f < 5; f++) out48[32 + kind * 8 + f] += w[((size_t)kind * 64 * 4096 + k) * 5 + f];
    }
    PT_HC(hipMemset(t->d_stamps, 0, sizeof(unsigned long long) * (48 + 2 * 64 * 4096 * 5)));
    return PTX_OK;
}

// Debug: how many workgroups of the specialised later-bounce kernel the runtime says fit a CU with `lds_bytes` of dynamic LDS each
// (0 = what this tracer launches it with); negative = error.
int ptx_debug_bounce_occupancy(ptx_tracer *t, int lds_bytes) {
    if (!t) return -1;
    if (hipSetDevice(t->device) != hipSuccess) return -1;
    const int ntri_lds = t->split_mesh ? 0 : t->ntri_lds;
    const int triWords = t->tri_lds ? sceneTableWords(ntri_lds, t->nmats, t->ngeoms) : 0;
    size_t lds = lds_bytes > 0 ? (size_t)lds_bytes : sizeof(int32_t) * (bounceLdsWords(triWords, t->nbins) - (17 - REC_ROWS_FAST0) * TILE);
    const KernelSet *ks = nullptr; const LastKernelSet *ksl = nullptr;      // (the exact level's, whatever the tracer's)
    if (kernel_tables(PTX_ARITH_EXACT, false, &ks, &ksl)) return -1;
    return ks->bounce_occupancy(lds);
}

// Host-only: what pt_prepare_scene decided for one mesh geom, and which walk each caller of the mesh search takes for it -- the rules of
// k_mesh's set-up (pt_kernels.hip: wideok), of meshKey (pt_device.h: wideok / ordered) and of ptx_create's bvh_stack, restated on the host copies.
int ptx_debug_mesh_plan(ptx_tracer *t, int geom, int32_t out8[8]) {
    if (!t || !out8) return pt_fail(PTX_ERR_INVALID, "null argument");
    if (geom < 0 || geom >= t->ngeoms || (size_t)geom >= t->h_roots.size()) return pt_fail(PTX_ERR_INVALID, "geom index out of range");
    if (t->h_geom_type[geom] != G_OBJ) return pt_fail(PTX_ERR_INVALID, "ptx_debug_mesh_plan: the geom is not a mesh");
    const int root = t->h_roots[geom], depth = t->h_depths[geom], wroot = t->h_wroots[geom], wneed = t->h_wneeds[geom];
    // (the four-wide tables reach the device only when some tree has four-wide nodes: ptx_create, step 7)
    const bool wide = root >= 0 && wroot >= 0 && t->d_bvh_wroot && wneed <= t->bvh_stack;
    const bool ordered = root >= 0 && depth < t->bvh_stack;
    out8[0] = root; out8[1] = depth; out8[2] = wroot; out8[3] = wneed; out8[4] = t->bvh_stack; out8[5] = t->split_mesh ? 1 : 0;
    out8[6] = root < 0 ? PTX_WALK_LOOP : (t->split_mesh && wide) ? PTX_WALK_WIDE_REFILL : PTX_WALK_SKIP;
    out8[7] = root < 0 ? PTX_WALK_LOOP : wide ? PTX_WALK_WIDE : ordered ? PTX_WALK_ORDERED : PTX_WALK_SKIP;
    return PTX_OK;
}

// Host-only: the layout of the local index this tracer's launches use (pt_plan.h, IndexPlan) -- what the tests of both forms assert the
// code path by.
int ptx_debug_index_plan(ptx_tracer *t, int64_t out8[8]) {
    if (!t || !out8) return pt_fail(PTX_ERR_INVALID, "null argument");
    const IndexPlan &x = t->ix;
    out8[0] = x.loop ? 1 : 0; out8[1] = x.n2_log2; out8[2] = x.words; out8[3] = (int64_t)x.entries; out8[4] = (int64_t)x.seg_words;
    out8[5] = x.bytes_per_path; out8[6] = t->cap; out8[7] = x.why_code;
    return PTX_OK;
}

int ptx_debug_aux_nonzero(ptx_tracer *t, int64_t out3[3]) {
    if (!t || !out3) return pt_fail(PTX_ERR_INVALID, "null argument");
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipStreamSynchronize(t->stream));
    for (int l = 1; l < MAX_LANES; l++) if (t->lane_stream[l]) PT_HC(hipStreamSynchronize(t->lane_stream[l]));
    const size_t nseg = (size_t)t->kmax * t->lanes, words = (size_t)t->cap / 32;
    std::vector<int32_t> tot(t->seg_totals * nseg);
    std::vector<uint32_t> planes(t->d_part ? words * nseg : 0);
    PT_HC(hipMemcpy(tot.data(), t->d_totals, t->totals_bytes, hipMemcpyDeviceToHost));
    if (t->d_part)
        PT_HC(hipMemcpy2D(planes.data(), sizeof(uint32_t) * words, t->d_part + 3 * (size_t)t->cap, sizeof(float) * t->seg_part,
                             sizeof(uint32_t) * words, nseg, hipMemcpyDeviceToHost));
    int64_t nz_planes = 0, nz_totals = 0, dirty = 0;
    for (int l = 0; l < t->lanes; l++) {
        if (t->aux_dirty[l]) { dirty++; continue; }
        const ptx_tracer::Ahead &a = t->ahead[l];
        for (int j = 0; j < t->kmax; j++) {
            if (a.valid && j >= a.next - a.first) continue;      // traced ahead, not gathered yet
            const size_t sg = (size_t)l * t->kmax + j;
            for (size_t k = 0; k < t->seg_totals; k++) nz_totals += tot[sg * t->seg_totals + k] != 0;
            if (t->d_part) for (size_t k = 0; k < words; k++) nz_planes += planes[sg * words + k] != 0;
        }
    }
    out3[0] = nz_planes; out3[1] = nz_totals; out3[2] = dirty;
    return PTX_OK;
}

int ptx_debug_set_capture(ptx_tracer *t, int bounce) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    PT_HC(hipSetDevice(t->device));
    t->capture_bounce = bounce;
    t->cap_filled = false;
    if (bounce >= 0 && !t->d_cap) {
        // pix, stream index, material|geom [cap each], the bounce's totals [nbins], run prefixes of the capture [2][nbins x grid_seg + 1]
        PT_HC(t->d_cap.alloc(3 * (size_t)t->cap + (size_t)t->nbins + 2 * ((size_t)t->nbins * t->grid_seg + 1)));
        PT_HC(t->d_cap_f.alloc(SOA_LOGICAL_FLOATS * (size_t)t->cap));
    }
    return PTX_OK;
}

int ptx_debug_read_stream(ptx_tracer *t, int *n_out, int32_t *pixel_index, int32_t *stream_idx, int32_t *material,
                          float *fields14, int cap) {
    if (!t || !n_out) return pt_fail(PTX_ERR_INVALID, "null argument");
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipStreamSynchronize(t->stream));
    *n_out = 0;
    if (!t->cap_filled) return pt_fail(PTX_ERR_INVALID, "nothing captured");
    std::vector<int32_t> tot((size_t)t->nbins);
    PT_HC(hipMemcpy(tot.data(), t->d_cap + 3 * (size_t)t->cap, sizeof(int32_t) * tot.size(), hipMemcpyDeviceToHost));
    int n = 0;
    for (int v : tot) n += v;
    *n_out = n;
    int m = n < cap ? n : cap;
    if (m > 0) {
        PT_HC(hipMemcpy(pixel_index, t->d_cap, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
        if (t->tm.tile_world > 1)             // paths carry their slot among the owned pixels: report the pixel (x + y*W)
            for (int k = 0; k < m; k++) {
                const int slot = pixel_index[k] & 0x0fffffff, r = slot / t->tm.W, x = slot - r * t->tm.W, blk = r / t->tm.tile_rows;
                pixel_index[k] = x + ((blk * t->tm.tile_world + t->tm.tile_rank) * t->tm.tile_rows + (r - blk * t->tm.tile_rows)) * t->tm.W;
            }
        PT_HC(hipMemcpy(stream_idx, t->d_cap + t->cap, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
        std::vector<int32_t> mg((size_t)m);
        PT_HC(hipMemcpy(mg.data(), t->d_cap + 2 * (size_t)t->cap, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
        for (int k = 0; k < m; k++) material[k] = mg[k] & 0xffff;
        if (fields14)       // 14 rows of m floats: px py pz dx dy dz cr cg cb nx ny nz u v
            for (int f = 0; f < SOA_LOGICAL_FLOATS; f++)
                PT_HC(hipMemcpy(fields14 + (size_t)f * m, t->d_cap_f + (size_t)f * t->cap, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
    }
    return PTX_OK;
}

}  // extern "C"
