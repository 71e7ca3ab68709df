// pt_kernels.hip -- the kernels of the MI355X (gfx950) path-tracing engine behind include/mi355x_pathtracer.h whose results depend on
// the arithmetic level: k_bounce in all variants, k_mesh, k_finish and the per-stage test kernels (k_kat_*), with the table of
// launchers (KernelSet, pt_kernels.h) through which the host reaches them.
//
// What belongs here: device code that does path arithmetic, and its launchers -- nothing else.  This file exists at EVERY level: the
// Makefile compiles it three times, with -DPT_ARITH=0 (EXACT: bit-identical to the CPU oracle, the level every headline number and
// every parity claim is made at), 1 (CONTRACTED: -ffp-contract=fast) and 2 (FAST: also -fno-hip-fp32-correctly-rounded-divide-sqrt);
// see pt_device.h for what each level means and include/mi355x_pathtracer.h (ptx_options.arith) for how a caller asks for one.  All a
// compilation adds to the library is ONE symbol, ptx_arith_kernels_<level>().  Host code, scene upload, buffers, launch plans and the
// kernels that are the same at every level (capture, gather, statistics, preview, G-buffer) are pt_engine.hip's, compiled once at the
// exact level: a kernel put here becomes level-dependent, a host helper put here is compiled three times.
//
// Replaces the device side of the reference's src/pathtrace.cu.  Design (see DESIGN.md for the full account):
//
//  * Streams are SoA (one fp32/int32 array per field, coalesced 256-B wave accesses), not the reference's 44-B
//    PathSegment / 32-B ShadeableIntersection AoS records: 15 words per stored path (17 with texcoords).
//  * One bounce = ONE launch: the fused kernel, whose tail and whose next launch's head together are the stable multi-bin
//    partition (round 3; rounds 1-2 ran it as a second kernel, k_move):
//      k_bounce : shade(b-1) [src/pathtrace.cu:355-404 + interactions.h scatterRay] immediately followed by
//                 computeIntersections(b) [:261-344] of the scattered ray, for every path still alive; bounce 0
//                 fuses generateRayFromCamera [:206-255] instead of a shade.  Paths that end at bounce b (miss,
//                 light, last bounce, emissive texel) add their radiance to the image right there, which is
//                 what finalGather [:407-416] would do later (each pixel exactly once per iteration), and are
//                 dropped -- only paths that will scatter again are stored.
//                 Every workgroup owns a contiguous chunk of tiles and keeps running per-material counts, so a
//                 tile's prefix = (totals of earlier workgroups) + (running count inside the chunk): no scan pass.
//      the sort : the reference's stable_partition [:541] followed by the next bounce's stable sort_by_key by material [:518] is
//                 ONE order: bin (material descending), then workgroup chunk, then tile, then rank in the tile.  It is never
//                 materialised.  TAIL of k_bounce ("local move"): every workgroup sorts the stored paths of ITS chunk of tiles
//                 by (bin, tile, rank) into a chunk-local index (8 B per path: stage slot + the path's rank among all survivors of
//                 its bin inside the chunk) -- no other workgroup's data is needed for that -- and leaves the chunk's per-bin
//                 counts in a flat [bin][workgroup] "run" table.  HEAD of the next k_bounce: a workgroup that will shade sorted
//                 positions [A, B) finds the run holding A by three 64-wide scans (bins -> groups of 64 workgroups -> workgroups),
//                 keeps a window of the next 64 runs' prefixes in LDS, and every position becomes (run, offset) by a 6-step search
//                 in LDS, hence a slot of the chunk-local index, hence the record and its RNG stream index [:373] (which counts the
//                 dropped survivors too and must be the reference's).  The 60-byte records stay where k_bounce put them.
//  * The live count never visits the host: kernels read it from device memory and use grid-stride tile loops,
//    so a batch of iterations is a fixed sequence of launches (depth + 2 of them); K iterations ride in every launch as segments
//    (blockIdx.y), and three such batches are in flight on three streams so that their kernels fill each other's tails.
//  * Intersection is tile-cooperative (tileIntersect): candidate masks from conservative world boxes, the (ray, geom)
//    pairs of a 256-path tile pooled in LDS and worked off by dense waves with a 64-bit LDS minimum per ray.  Scenes
//    with BVH meshes run the mesh search as kernels of their own (k_mesh: the search, refilling waves; k_finish: the parked rays'
//    finishing) between two halves of k_bounce.
//  * Scene tables (materials, per-geom matrices, small meshes' triangles, tabulated normals) are staged in LDS; the
//    world boxes are read through the scalar cache.
//
// `ptd` is renamed for the translation units of levels 1 and 2, before pt_device.h is seen: every inline function of pt_device.h /
// pt_bvh.h compiled with those flags gets a symbol of its own, so the linker can never hand an exact translation unit a contracted
// copy (or the other way round).
// PT_PLAIN (Makefile: with -DPT_UNIT_RSQRT=0 -DPT_SHARED_RCP=0, levels 0 and 1): the same once more without those two routines of
// pt_device.h, exported as ptx_arith_kernels_<level>p / ptx_arith_last_<level>p (PTX_DEBUG_NO_UNIT_RSQRT).
#if defined(PT_PLAIN) && PT_PLAIN && !defined(PT_ARITH)
#error "PT_PLAIN needs PT_ARITH"
#endif
#if defined(PT_PLAIN) && PT_PLAIN && PT_ARITH == 0
#define ptd ptd_plain0
#define PT_ARITH_TAG 0p
#elif defined(PT_PLAIN) && PT_PLAIN && PT_ARITH == 1
#define ptd ptd_plain1
#define PT_ARITH_TAG 1p
#elif defined(PT_PLAIN) && PT_PLAIN
#error "PT_PLAIN: levels 0 and 1 only"
#elif PT_ARITH == 1
#define ptd ptd_arith1
#elif PT_ARITH == 2
#define ptd ptd_arith2
#elif defined(PT_ARITH) && PT_ARITH != 0
#error "PT_ARITH must be 0, 1 or 2"
#endif
#ifndef PT_ARITH_TAG
#define PT_ARITH_TAG PT_ARITH
#endif
#include <string.h>

#include "pt_kernels.h"

namespace {

// stage key: bin | rank among all survivors of the tile << 16 | rank among the stored ones << 24 (ranks < 256)
__device__ __forceinline__ int32_t stage_key(int bin, int r_all, int r_scat) { return (int32_t)((uint32_t)bin | ((uint32_t)r_all << BIN_BITS) | ((uint32_t)r_scat << (BIN_BITS + RANK_BITS))); }
__device__ __forceinline__ void fence_report(const BounceParams &p) { atomicAdd(p.fenced, 1ull); }

__device__ __forceinline__ int sum_totals(const int32_t *t, int n) {
    int s = 0;
    for (int b = 0; b < n; b++) s += t[b];
    return s;
}

// computeIntersections for a whole tile, cooperatively.  Every ray lists the geoms whose conservative world box it
// reaches (cullMask); the (ray, geom) pairs of the tile are pooled in LDS -- cubes and spheres first, meshes after --
// and worked off by dense waves, each pair folding its result into its ray's 64-bit minimum with an LDS atomic
// (primKey / meshKey / packKey: min key = nearest t, lowest geom index on ties, i.e. the reference's answer).  In a
// wave of incoherent rays this replaces "every lane waits for all 7 geoms" by "about 1.3 pairs per ray, packed".
// Must be called by all threads of the workgroup (barriers inside); `scratch` = TILE*17 words of LDS.
constexpr int ITEMS_PER_PASS = 4;                      // pairs a ray may contribute per pass (1024-entry list)
#ifdef PT_STAMPS
#define TI_STAMP(k) do { unsigned long long t1_ = __builtin_amdgcn_s_memtime(); st_acc[k] += t1_ - st_t0; st_t0 = t1_; } while (0)
#define TI_ARGS , unsigned long long *st_acc, unsigned long long &st_t0
#define TI_PASS , st_acc, st_t0
#else
#define TI_STAMP(k) do { } while (0)
#define TI_ARGS
#define TI_PASS
#endif
// DEFER: the mesh pairs are not worked off here; the caller gets the best key over cubes and spheres and the ray's
// mesh candidates (split mesh search, see k_mesh), and `hit` is left alone.
// !DECODE: the caller wants the winning key only (the light-only last bounce: its geom's material is all that matters); `hit` is left alone.
__device__ __forceinline__ int waveInclusiveScan(int v, int lane);      // (below)
template <bool DEFER, bool PARK = false, bool SUBSET = false, bool DECODE = true>
__device__ __forceinline__ void tileIntersect(const DScene &sc, bool alive, Ray ray, bool need_uv, Hit &hit, int32_t *scratch,
                                              int32_t *tcnt, int &q, int tid, int lane, int wave, unsigned long long &key_out,
                                              uint32_t &mesh_out TI_ARGS, uint32_t subset = 0xffffffffu) {
    const float *gtab = reinterpret_cast<const float *>(pt_lds) + sc.ntri_lds * 24 + sc.nmats * 11;
    float *rayb = reinterpret_cast<float *>(scratch);                              // [6][TILE]
    unsigned long long *best = reinterpret_cast<unsigned long long *>(scratch + 6 * TILE);   // [TILE]
    uint16_t *list = reinterpret_cast<uint16_t *>(scratch + 8 * TILE);             // [CAP] ray | geom << RANK_BITS: cubes from the front,
    uint16_t *listM = list + ITEMS_PER_PASS * TILE;                                // spheres from the back; [CAP] meshes
    constexpr int CAP = ITEMS_PER_PASS * TILE;
    uint32_t cube_mask = 0, sph_mask = 0, mesh_mask = 0, m_all = 0;
    if (alive) {
        m_all = cullMask<SUBSET>(sc, ray, subset);
        cube_mask = m_all & sc.cube_bits; sph_mask = m_all & sc.sphere_bits; mesh_mask = m_all & sc.mesh_bits;
    }
    mesh_out = mesh_mask;
    if (DEFER) mesh_mask = 0;
    // Camera rays (SUBSET): the 64 rays of a wave are neighbouring pixels of a row and very often reach the same boxes -- the back wall
    // alone, say.  Such a wave (every lane alive, every mask lane 0's, at most ITEMS_PER_PASS candidates: one pass) needs no prefix: with n
    // entries of a kind per lane, lane l's start at l * n and the wave has 64 * n.  (All threads of the workgroup are here: exec is full.)
    bool uniform_wave = false;
    if (SUBSET && PT_WAVE_UNIFORM) {
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)m_all);
        uniform_wave = __ballot(alive && m_all == m0) == ~0ull && __popc(m0 & (DEFER ? ~sc.mesh_bits : 0xffffffffu)) <= ITEMS_PER_PASS;
    }
    rayb[0 * TILE + tid] = ray.o.x; rayb[1 * TILE + tid] = ray.o.y; rayb[2 * TILE + tid] = ray.o.z;
    rayb[3 * TILE + tid] = ray.d.x; rayb[4 * TILE + tid] = ray.d.y; rayb[5 * TILE + tid] = ray.d.z;
    best[tid] = KEY_NONE;
    for (;;) {
        // this pass: up to ITEMS_PER_PASS pairs per ray -- cubes, then spheres, then meshes, each kind in a run of
        // its own so that the waves working the list off run one kind of test.  Slots: prefix inside the wave from ONE scan of
        // the three capped counts (<= ITEMS_PER_PASS each, a wave's total <= 256: 10-bit fields of one word), one LDS atomic per wave
        // and kind for its base (tcnt[4q..]: cube, sphere and
        // mesh pairs, "some ray has more"; the other parity's counters are cleared meanwhile for the next pass).
        const int cc = (int)__popc(cube_mask), cs = (int)__popc(sph_mask), cm = (int)__popc(mesh_mask);
        const int nc = cc < ITEMS_PER_PASS ? cc : ITEMS_PER_PASS;
        const int ns = cs < ITEMS_PER_PASS - nc ? cs : ITEMS_PER_PASS - nc;
        const int nm = cm < ITEMS_PER_PASS - nc - ns ? cm : ITEMS_PER_PASS - nc - ns;
        int base[3], tot[3];
        unsigned long long left = 0ull;
        if (SUBSET && PT_WAVE_UNIFORM && uniform_wave) {                 // (wave-uniform branch; one pass, nothing is left over)
            const int u0 = __builtin_amdgcn_readfirstlane(nc), u1 = __builtin_amdgcn_readfirstlane(ns), u2 = __builtin_amdgcn_readfirstlane(nm);
            base[0] = lane * u0; base[1] = lane * u1; base[2] = lane * u2;
            tot[0] = 64 * u0; tot[1] = 64 * u1; tot[2] = 64 * u2;
        } else {
#if PT_PACKED_SLOTS
            const int packed = nc | (ns << 10) | (nm << 20);
            const int inc = waveInclusiveScan(packed, lane), exc = inc - packed;
            const int all = __builtin_amdgcn_readlane(inc, 63);
            base[0] = exc & 1023; base[1] = (exc >> 10) & 1023; base[2] = exc >> 20;
            tot[0] = all & 1023; tot[1] = (all >> 10) & 1023; tot[2] = all >> 20;
#else
            const int cnt3[3] = {nc, ns, nm};
#pragma unroll
            for (int kind = 0; kind < 3; kind++) {
                const unsigned long long b0 = __ballot(cnt3[kind] & 1), b1 = __ballot(cnt3[kind] & 2), b2 = __ballot(cnt3[kind] & 4);
                base[kind] = wavePrefix(b0, lane) + 2 * wavePrefix(b1, lane) + 4 * wavePrefix(b2, lane);
                tot[kind] = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
            }
#endif
            left = __ballot(cc + cs + cm > nc + ns + nm);
        }
        int wb0 = 0, wb1 = 0, wb2 = 0;
        if (lane == 0) {
            if (tot[0]) wb0 = atomicAdd(&tcnt[4 * q + 0], tot[0]);
            if (tot[1]) wb1 = atomicAdd(&tcnt[4 * q + 1], tot[1]);
            if (tot[2]) wb2 = atomicAdd(&tcnt[4 * q + 2], tot[2]);
            if (left) tcnt[4 * q + 3] = 1;
        }
        base[0] += __builtin_amdgcn_readfirstlane(wb0);
        base[1] += __builtin_amdgcn_readfirstlane(wb1);
        base[2] += __builtin_amdgcn_readfirstlane(wb2);
        for (int j = 0; j < nc; j++) {
            const int g = __ffs((int)cube_mask) - 1;
            cube_mask &= cube_mask - 1;
            list[base[0] + j] = (uint16_t)(tid | (g << RANK_BITS));
        }
        for (int j = 0; j < ns; j++) {
            const int g = __ffs((int)sph_mask) - 1;
            sph_mask &= sph_mask - 1;
            list[CAP - 1 - (base[1] + j)] = (uint16_t)(tid | (g << RANK_BITS));
        }
        for (int j = 0; j < nm; j++) {
            const int g = __ffs((int)mesh_mask) - 1;
            mesh_mask &= mesh_mask - 1;
            listM[base[2] + j] = (uint16_t)(tid | (g << RANK_BITS));
        }
        __syncthreads();
        const int totC = tcnt[4 * q + 0], totS = tcnt[4 * q + 1], totM = tcnt[4 * q + 2], more = tcnt[4 * q + 3];
        if (tid < 4) tcnt[4 * (q ^ 1) + tid] = 0;
        TI_STAMP(5);
#ifdef PT_STAMPS
        if (tid == 0) { st_acc[8] += totC + totS; st_acc[9] += totM; st_acc[10] += 1; }
#endif
        // each kind starts on a wave boundary: cubes [0, totC), spheres from roundup64(totC), meshes after them
        // small meshes (no BVH in the scene): every (ray, mesh) pair becomes mesh_chunks entries, one per group of
        // MESH_CHUNK faces, chunk-major so that a wave reads the same faces
        const int startS = (totC + 63) & ~63, startM = startS + ((totS + 63) & ~63);
        const int nch = sc.mesh_chunks > 1 ? sc.mesh_chunks : 1;
        for (int k = tid; k < startM + totM * nch; k += TILE) {
            int item = -1, chunk = -1;
            if (k < totC) item = list[k];
            else if (k >= startS && k < startS + totS) item = list[CAP - 1 - (k - startS)];
            else if (k >= startM) {
                int kk = k - startM;
                if (nch > 1) { chunk = 0; while (kk >= totM) { kk -= totM; chunk++; } }
                item = listM[kk];
            }
            if (item >= 0) {
                const int src = item & (TILE - 1), g = item >> RANK_BITS;
                Ray r;
                r.o = V3(rayb[0 * TILE + src], rayb[1 * TILE + src], rayb[2 * TILE + src]);
                r.d = V3(rayb[3 * TILE + src], rayb[4 * TILE + src], rayb[5 * TILE + src]);
                // (tileIntersect runs with the tables staged; the triangle tables too unless the scene's meshes are too big)
                // (DEFER: the mesh list stays empty, so its tests are not compiled into that kernel at all)
                const unsigned long long key = (DEFER || k < startM) ? primKey(gtab, g, r)
                    : ((sc.tri_lds == 2 || sc.ntri_lds) ? meshKey<true>(sc, gtab, g, r, chunk) : meshKey<false>(sc, gtab, g, r, chunk));
                if (key != KEY_NONE) atomicMin(&best[src], key);
            }
        }
        __syncthreads();
        q ^= 1;
        TI_STAMP(6);
        // another pass only if some ray still has candidates (rare: more than ITEMS_PER_PASS boxes along one ray)
        if (!more) break;
    }
    // no barrier here: the caller passes at least two before it touches `scratch` again
    key_out = best[tid];
    if (PARK) {                                    // the ray was not kept in registers across the pair tests: take the LDS copy
        asm volatile("" ::: "memory");
        ray.o = V3(rayb[0 * TILE + tid], rayb[1 * TILE + tid], rayb[2 * TILE + tid]);
        ray.d = V3(rayb[3 * TILE + tid], rayb[4 * TILE + tid], rayb[5 * TILE + tid]);
    }
    if (!DEFER && DECODE) decodeKey(sc, gtab, key_out, ray, need_uv, hit);
    TI_STAMP(7);
}

// What pass 1 of the split bounce (and k_finish, for the rays pass 1 parked) tells pass 2 about ray i: one word, lsrc[i] of the stage
// until the tail overwrites it.  CAND = parked with mesh candidates in slot (bits 16-23) of its tile, k_finish will replace the
// word; otherwise the ray is finished -- alive / stored flags, its bin (bits 0-15) and, if stored, the slot its record lies in.
constexpr int32_t K1_CAND = (int32_t)0x80000000u, K1_ALIVE = 0x40000000, K1_PEND = 0x20000000;

// The terminal cases of shadeFakeMaterial(b) for a path whose nearest hit is known (src/pathtrace.cu:380-390, :400): light =>
// radiance, miss or last bounce => black, otherwise the path is stored for the next bounce (pending); also the path's material bin.
template <bool FIRST>
__device__ __forceinline__ void classifyPath(const BounceParams &p, int iter, float *part, bool batched, const Hit &hit, vec3 color, int pix,
                                             int &bin, bool &pending) {
    bin = p.sort ? (p.sc.nmats - 1 - hit.mat) : 0;           // material descending; a miss carries id 0
    if (FIRST && p.albedo && iter == 1) write_albedo(p.sc, hit, p.albedo + (size_t)slot_to_pixel(p.tm, pix) * 3);
    bool lit = false;
    if (hit.t > 0.0f) {
        const DMaterial m = getMaterial(p.sc, hit.mat);
        if (m.emittance > 0.0f) {                           // src/pathtrace.cu:380-383
            lit = true;
            vec3 c = mul(color, scale(V3(m.color[0], m.color[1], m.color[2]), m.emittance));
            deposit(p.tm, p.image, part, batched, pix, c, p.apps, p.fence_slots_cap);
            if (FIRST && p.emit_count) {
                const vec3 cd = p.apps ? scale(c, 3.14159265358f) : c;
                int k = atomicAdd(p.emit_count, 1);
                p.emit_pix[k] = pix;
                p.emit_rgb[k * 3 + 0] = cd.x; p.emit_rgb[k * 3 + 1] = cd.y; p.emit_rgb[k * 3 + 2] = cd.z;
            }
        } else if (p.traceDepth - p.bounce != 1) {         // :387-390 (last bounce => black)
            pending = true;
        }
    }
    // a miss or a last-bounce hit ends the path with colour 0 (:388, :400): nothing to add to the image -- and, since round 5, nothing to
    // store in batched mode either (the pixel's "lit" flag of this iteration stays clear: k_gather skips the slot)
    (void)lit;
}

// inclusive prefix sum over the lanes of a wave, in the vector ALU's own lane network (DPP): four shifted adds inside the rows of 16
// lanes, then lane 15 of a row broadcast to the next row (rows 1 and 3) and lane 31 to the upper half -- six dependent vector
// instructions.  (__shfl_up goes through the LDS crossbar: six ds_bpermute round trips, 0.3 us on a tile's critical path each time.)
__device__ __forceinline__ int waveInclusiveScan(int v, int lane) {
    (void)lane;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);      // row_shr:1 (lanes without a source add 0)
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);      // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);      // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);      // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
    return v;
}

// ---- where a sorted position lies (head of the sort, see the file comment) --------------------------------------------------
// The previous bounce left its stored paths as RUNS: run r = bin * gx + workgroup holds cs[r] stored paths (of ca[r] survivors)
// and starts at cbase[r] in the chunk-local index; in run order (bin-major) the runs ARE the sorted stream.  Position P of that
// stream lies in the first run whose inclusive prefix of cs exceeds P.
//
// scanFind: one wave walks n entries of (stored, survivors) counts 64 at a time, adding them to the running prefixes pre_s /
// pre_a, and stops at the first entry whose inclusive stored-prefix exceeds A; returns its index (-1: none), with pre_s / pre_a
// the prefixes in FRONT of it.  All arguments and results are wave-uniform.
__device__ __forceinline__ int scanFind(const int32_t *cs, const int32_t *ca, int n, int A, int &pre_s, int &pre_a, int lane) {
    for (int base = 0; base < n; base += 64) {
        const int k = base + lane;
        const int vs = k < n ? cs[k] : 0, va = k < n ? ca[k] : 0;
        const int is = waveInclusiveScan(vs, lane), ia = waveInclusiveScan(va, lane);
        const unsigned long long m = __ballot(k < n && pre_s + is > A);
        if (m) {
            const int l = __ffsll((long long)m) - 1;
            pre_s += __builtin_amdgcn_readlane(is - vs, l);
            pre_a += __builtin_amdgcn_readlane(ia - va, l);
            return base + l;
        }
        pre_s += __builtin_amdgcn_readlane(is, 63);
        pre_a += __builtin_amdgcn_readlane(ia, 63);
    }
    return -1;
}
// The same search with EIGHT consecutive entries per lane: 512 entries per memory round trip instead of 64 (the loads of a trip are
// all requested before the first is used).  The tables searched this way are short (bins x groups of 64 workgroups).
__device__ __forceinline__ int scanFind8(const int32_t *cs, const int32_t *ca, int n, int A, int &pre_s, int &pre_a, int lane) {
    for (int base = 0; base < n; base += 512) {
        int vs[8], va[8];
        const int k0 = base + lane * 8;
#pragma unroll
        for (int j = 0; j < 8; j++) { vs[j] = k0 + j < n ? cs[k0 + j] : 0; va[j] = k0 + j < n ? ca[k0 + j] : 0; }
        int ss = 0, sa = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) { ss += vs[j]; sa += va[j]; }
        const int is = waveInclusiveScan(ss, lane), ia = waveInclusiveScan(sa, lane);
        const unsigned long long m = __ballot(pre_s + is > A);
        if (m) {
            const int l = __ffsll((long long)m) - 1;                 // the lane whose eight entries hold the answer
            pre_s += __builtin_amdgcn_readlane(is - ss, l);
            pre_a += __builtin_amdgcn_readlane(ia - sa, l);
            int found = -1;
#pragma unroll
            for (int j = 0; j < 8; j++) {                            // (uniform: every lane walks lane l's entries)
                const int es = __builtin_amdgcn_readlane(vs[j], l), ea = __builtin_amdgcn_readlane(va[j], l);
                if (found < 0) {
                    if (pre_s + es > A) found = base + l * 8 + j;
                    else { pre_s += es; pre_a += ea; }
                }
            }
            return found;
        }
        pre_s += __builtin_amdgcn_readlane(is, 63);
        pre_a += __builtin_amdgcn_readlane(ia, 63);
    }
    return -1;
}

// The window: runs [r0, r0 + WIN) of the table with their exclusive prefixes, in LDS (one wave; the caller brackets it with
// barriers).  win[0 .. WIN] = first sorted position of each run and of what follows the window, win[WIN+1 .. 2*WIN+1] = the same
// for the survivor counts (= the RNG stream index of a run's first survivor), then the runs' starts in the local index, then r0 + WIN.
__device__ __forceinline__ void windowLoad(int32_t *win, const int32_t *chunk, int chunk_cap, int nruns, int r0, int gs0, int ga0, int lane) {
    const int r = r0 + lane;
    int ca = 0, cs = 0, cb = 0;
    if (r < nruns && lane < WIN) { ca = chunk[r]; cs = chunk[chunk_cap + r]; cb = chunk[2 * chunk_cap + r]; }
    const int is = waveInclusiveScan(cs, lane), ia = waveInclusiveScan(ca, lane);
    if (lane < WIN) {
        win[lane] = gs0 + is - cs;
        win[WIN + 1 + lane] = ga0 + ia - ca;
        win[2 * (WIN + 1) + lane] = cb;
    }
    if (lane == WIN - 1) { win[WIN] = gs0 + is; win[2 * WIN + 1] = ga0 + ia; win[2 * (WIN + 1) + WIN] = r0 + WIN; }
}

// One bounce.  FIRST: generate camera rays; otherwise shade the stored paths of the previous bounce.
// MODE 1: LDS queue -> global queue of the segment (all threads of the workgroup; uniform call)
__device__ __forceinline__ void flushQueue(const BounceParams &p, int seg, const uint32_t *qbuf, int32_t *qcnt, int32_t *qbase, int tid) {
    const int n = *qcnt;
    if (tid == 0) *qbase = atomicAdd(p.item_count + seg, n);
    __syncthreads();
    uint32_t *dst = p.items + p.seg_items * seg + *qbase;
    for (int k = tid; k < n; k += TILE) dst[k] = qbuf[k];
    __syncthreads();
    if (tid == 0) *qcnt = 0;
    __syncthreads();
}

// MODE 0: the whole bounce.  Scenes with BVH meshes split it so that the mesh search -- few rays of a tile, each a long
// chain of dependent node visits -- does not hold the tile's other waves at a barrier: MODE 1 does the whole bounce for the
// rays that reach no mesh's box and, for the others, everything up to the best hit among cubes and spheres; those it parks
// (origin, direction, colour, pixel, candidate mask in a stage slot at the top of the tile, the key in `keys`) with one queue
// entry each; k_mesh's waves draw rays from the queue and search their meshes, k_finish finishes them, one dense lane per ray;
// MODE 2 ranks all rays of the tile (the order needs every ray's bin) and writes the sort keys.  Same arithmetic, same bits.
// FAST: the options that are run-time values in the general kernel are compile-time constants for the common case -- no
// textures, material sort on, candidate masks and all scene tables in LDS, no BVH mesh, no bump map, no depth
// of field, batched radiance buffers, not the cache-filling pass -- so that every test of them, and the code behind the
// untaken side, is gone (C4: k_bounce -6 %, the first bounce -11 %, fewer registers).  The host picks the variant per launch
// (enqueue_batch); everything else takes the general kernel, same results.  For the two halves of the split bounce (MODE 1, 2)
// FAST bakes only the subset that textured scenes with BVH meshes satisfy as well.
// LAST (later bounce, MODE 0 only): the launch is the paths' last intersection (bounce traceDepth - 1), where classifyPath
// never stores a path: it ends with radiance if its nearest hit emits, and black -- nothing written at all -- otherwise.  No later launch
// reads a rank, a key, a record, a prefix or a run table of this bounce.  So, behind the unchanged head (run search, gather,
// scatterRay with the stored stream index): only the rays that reach the inflated box of some emitting geom (sc.light_bits; the same
// slab test as the candidate masks, so a miss there is a miss of the geom in the full test too) go on, to the pair tests against ALL
// their candidates -- an occluder must win -- and the winner's material alone decides: emissive => the deposit classifyPath makes,
// otherwise nothing.  No normal, no ranking, no epilogue, no tail; the bounce's ray count, which k_stats sums over the bins, goes to bin 0.
// The specialised variant pools those rays over the workgroup's tiles and tests them a full tile at a time (see the LAST branch of the tile loop).
// It is MODE_ 3 of this template (MODE_LAST) and MODE 0 in everything but the above: the other instantiations do not see it.  It is
// instantiated by pt_kernels_last.hip alone (this source with PT_KERNELS_LAST_UNIT, see the end of the file), one more code object per level.
constexpr int MODE_LAST = 3;
template <bool FIRST, int MODE_, bool FAST = false>
__global__ __launch_bounds__(TILE, !FAST ? PT_BOUNCE_WAVES : MODE_ == 1 ? PT_FAST_WAVES_SPLIT : MODE_ == 2 ? PT_FAST_WAVES_SPLIT2 : FIRST ? PT_FAST_WAVES_FIRST : PT_FAST_WAVES) void k_bounce(const BounceParams p_in) {      // (the camera-ray
                                                                                   // variant needs 65 registers: seven waves without spilling)
    constexpr bool LAST = MODE_ == MODE_LAST;
    constexpr int MODE = LAST ? 0 : MODE_;
    static_assert(MODE_ >= 0 && MODE_ <= MODE_LAST && !(LAST && FIRST), "modes 0-2, and the light-only variant of a later unsplit bounce");
#ifdef PT_WGCLOCK
    const unsigned long long wg_t0 = wall_clock64();       // 100 MHz: latency of the workgroup's phases (prologue, tile loop, tail)
#endif
    BounceParams p = p_in;
    if (FAST && MODE != 0) {             // the two halves of the split bounce: the subset that holds for textured BVH scenes too
        p.sort = 1; p.albedo = nullptr; p.emit_count = nullptr; p.sc.cull = 1; p.sc.tri_lds = 1;
    }
    if (FAST && MODE == 0) {
        p.uses_uv = 0; p.sort = 1; p.albedo = nullptr; p.emit_count = nullptr; p.dof = 0;
        p.sc.cull = 1; p.sc.tri_lds = 2; p.sc.bump_bits = 0; p.sc.ntri_lds = p.sc.ntri; p.sc.bvh_root = nullptr;
    }
    // dynamic LDS (pt_lds): [scene tables when staged: triangles, materials][2][WAVES][nbins] ranking histogram [2][nbins] running prefix
    // [nbins] tile counts [nbins+1] tile offsets [17][TILE] records being sorted
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = p.nbins;
    const int triWords = (MODE != 2 && p.sc.tri_lds) ? sceneLdsWords(p.sc) : 0;      // (pass 2 of the split bounce only ranks: no scene tables)
    int32_t *lds = pt_lds + triWords;
    int32_t *w_all = lds, *w_scat = lds + WAVES * nb;
    int32_t *run_all = lds + 2 * WAVES * nb, *run_scat = run_all + nb;
    int32_t *tcs = run_scat + nb, *toff = tcs + nb;                 // stored-path count per bin of this tile, its prefix
    int32_t *tcnt = toff + nb + 1;                                  // tileIntersect's list counters [2][4], zero between uses
    int32_t *win = tcnt + 8;                                        // window over the input's run tables [WIN_WORDS] (windowLoad)
    int tq = 0;
    int32_t *rec = lds + ldsHeadWords(nb);                  // [17][TILE] record transpose buffer / tileIntersect scratch,
                                                                    // 16-byte aligned (64-bit LDS atomics live in it)
    constexpr int R_PIX = (FAST && MODE == 0 ? REC_ROWS_FAST0 : 17) - 3, R_MG = R_PIX + 1, R_KEY = R_PIX + 2;      // rows of the record buffer (12 floats, [u, v,] these)
    uint32_t *qbuf = reinterpret_cast<uint32_t *>(rec + REC_WORDS);   // MODE 1: LDS stage of the queue of parked rays, [QCAP], kept
    int32_t *qcnt = rec + REC_WORDS + QCAP, *qbase = qcnt + 1;        // across tiles (so not inside the record buffer)
    if (MODE == 1 && tid == 0) *qcnt = 0;
    for (int k = tid; k < 2 * nb; k += TILE) run_all[k] = 0;
    if (tid < 8) tcnt[tid] = 0;
    if (LAST && tid == 0) tcs[0] = 0;                               // (the pool of the light-only bounce, see there)
    __syncthreads();
    const int seg = blockIdx.y;
    const int iter = p.iter + seg * p.iter_stride;
    const PathSoA in_k = soa_offset(p.in, p.seg_in * seg), stage_k = soa_offset(p.stage, p.seg_stage * seg);
    int32_t *counts_all = p.counts_all + p.seg_counts * seg, *counts_scat = p.counts_scat + p.seg_counts * seg;
    // stored paths per tile (a third block behind the two prefix tables): the tail reads only that many keys of a tile -- slots beyond hold
    // no record and, since round 5, no "no record" key either (4 B written and 4 B read per ended path of a 256-path tile saved)
    int32_t *tile_np = counts_all + 2 * (size_t)nb * p.maxTiles;
    // The tile epilogue without LDS (PT_DIRECT_STORE; up to 64 bins: lane b of EVERY wave owns bin b).  Until round 5 the stored paths of a
    // tile were written into an LDS record buffer at their slots, and read back in slot order for dense stores, behind wave 0's scan of
    // the per-bin counts: three barriers (counts ready, records in LDS, buffer free again) after the ranking's own, every one of them a
    // wait for the slowest of four waves -- 18 % of k_bounce's wave cycles sat in "ranking" and 8 % in "sort + write" for ~230 vector
    // instructions.  Now every wave sums the four waves' counts and scans them itself (the same ~20 instructions, nobody waits for wave
    // 0), a lane fetches its bin's offset from lane `bin` (ds_bpermute) and stores its record's quads straight to slot offset + rank:
    // lanes of one bin are consecutive slots, a wave's store is a handful of contiguous runs.  What is left per tile: the two barriers
    // of the pair test and the ranking's one.  The histogram rows a wave zeroes are now its OWN, after the pair test's barriers (every
    // wave has then left the previous tile): no other wave can still be reading them.
    const bool direct = PT_DIRECT_STORE && MODE != 2 && (FAST || nb <= 64);      // (the specialised variants are only launched with <= 64 bins: fast_violation)
    // The local index in its bin-major form (BounceParams::loop_idx), unsplit bounce only.  loop_w: a pending lane of the direct epilogue
    // stores its index word beside its quads -- no stage key, no per-tile prefix tables, no stored count per tile, and no pass over the
    // keys in the tail.  in_loop: `in` was written that way.  Both are compile-time false in the split bounce's kernels.
    const bool loop_w = MODE == 0 && !LAST && direct && (p.loop_idx & 1), in_loop = MODE == 0 && !FIRST && (p.loop_idx & 2);
    const uint32_t n2s = (uint32_t)(p.loop_idx >> 8) & 31u;                                   // log2 N2
    const size_t ix_seg = ((size_t)nb << n2s) << ((p.loop_idx >> 2) & 1);                       // words of one segment's index
    int32_t *ix_out = p.stage.i + (p.seg_stage ? ix_seg * seg : 0);
    const int32_t *ix_in = p.in.i + (p.seg_in ? ix_seg * seg : 0);
    int32_t *chunk_out = p.chunk + p.seg_chunk * seg;
    int32_t *super_all = p.super_all + p.seg_totals * seg, *super_scat = p.super_scat + p.seg_totals * seg;
    int32_t *totals_all = p.totals_all + p.seg_totals * seg, *totals_scat = p.totals_scat + p.seg_totals * seg;
    float *part = (FAST || p.part) ? p.part + p.seg_part * seg : nullptr;
    const bool batched = FAST || part != nullptr;
    const int32_t *in_totals = FIRST ? nullptr : p.in_totals + p.seg_in_totals * seg;
    const int32_t *in_chunk = FIRST ? nullptr : p.in_chunk + p.seg_in_chunk * seg;
    const int in_nruns = nb * p.in_gx;
    // the input's stored paths per bin: lane b of every wave holds bin b's (ONE load instead of a chain of scalar ones -- a small launch's
    // workgroup lives 30 us, and this prologue is a third of it); more than 64 bins: the scalar loop
    int v_tot = 0;
    if (!FIRST && nb <= 64 && lane < nb) v_tot = in_totals[nb + lane];
    const int n_in = FIRST ? p.tm.owned : nb <= 64 ? __builtin_amdgcn_readlane(waveInclusiveScan(v_tot, lane), 63) : sum_totals(in_totals + nb, nb);
    const int ntiles = (n_in + TILE - 1) / TILE;
    // every workgroup owns a contiguous chunk of tiles, so that the prefix of a tile is (prefix of its chunk) +
    // (running sum inside the chunk) and no separate scan pass over the tiles is needed
    const int chunk = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int tile0 = min((int)blockIdx.x * chunk, ntiles), tile1 = min(tile0 + chunk, ntiles);
    // Which sorted positions hold records WITH an incoming direction (dir_bins: scatterRay reads it for reflective and refractive materials
    // and on OBJ geoms; a diffuse hit on a cube or sphere -- most of a Cornell scene -- never does, and its record's three direction
    // words are neither stored nor loaded: 24 B of the 120 a stored path moves).  The stream is sorted by bin: up to two ranges of
    // positions, from the input's per-bin totals.  In the same way the records of a material that only cubes have carry a 3-bit code of the
    // cube's tabulated normal (in pix's bits 28-30) instead of the normal: another 24 B; a diffuse wall's record is 32 B instead of 56.
    // (ptx_create leaves at most two runs of set bits in either mask, so two ranges always do: empty bins only merge them)
    auto binRanges = [&](unsigned long long mask, int &lo0, int &len0, int &lo1, int &len1) {
        int lo[2] = {0, 0}, hi[2] = {0, 0}, nr = 0, pos = 0;
        bool open = false;
        for (int b = 0; b < nb; b++) {
            const int tot = __builtin_amdgcn_readlane(v_tot, b);      // (masks are only in use with <= 64 bins)
            if (tot > 0) {
                const bool set = (mask >> b) & 1ull;
                if (set && !open) { if (nr < 2) lo[nr] = pos; open = true; }
                else if (!set && open) { if (nr < 2) hi[nr] = pos; nr++; open = false; }
            }
            pos += tot;
        }
        if (open) { if (nr < 2) hi[nr] = pos; nr++; }
        lo0 = lo[0]; len0 = hi[0] - lo[0]; lo1 = lo[1]; len1 = hi[1] - lo[1];
    };
    const bool masks_on = MODE != 2 && nb <= 64;
    const bool dir_some = masks_on && p.dir_bins != ~0ull;        // (uniform: the writer's side of the same rules.  Split bounce: the rays pass 1
    const bool ntab_some = masks_on && p.ntab_bins != 0ull;       // parks keep their direction -- k_mesh walks with it -- whatever their bin turns out to be)
    int dir_lo0 = 0, dir_len0 = 0x7fffffff, dir_lo1 = 0, dir_len1 = 0;      // sorted positions whose records carry a direction: all, unless ...
    int ntab_lo0 = 0, ntab_len0 = 0, ntab_lo1 = 0, ntab_len1 = 0;           // ... whose records carry a normal code instead of a normal: none, unless ...
    if (!FIRST && masks_on && p.in_dir_bins != ~0ull) binRanges(p.in_dir_bins, dir_lo0, dir_len0, dir_lo1, dir_len1);
    if (!FIRST && masks_on && p.in_ntab_bins != 0ull) binRanges(p.in_ntab_bins, ntab_lo0, ntab_len0, ntab_lo1, ntab_len1);
#ifdef PT_STAMPS
    unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, st_t0, st_t1;
#define STAMP(k) do { st_t1 = __builtin_amdgcn_s_memtime(); st_acc[k] += st_t1 - st_t0; st_t0 = st_t1; } while (0)
#else
#define STAMP(k) do { } while (0)
#endif
    // Head of the sort: the run that holds this workgroup's first sorted position, found by wave 0 in TWO memory round trips while
    // the other waves stage the scene tables (the short kernels of a small tile are chains of such round trips: the prologue was
    // a third of a workgroup's life there).  Trip 1: the flat [bin][group of 64 workgroups] table, eight entries per lane -> the
    // group.  Trip 2: that group's 64 runs and the 64 after them, three tables -> the run, and from the same registers the window
    // of the 64 runs from it on (what windowLoad would fetch in a third trip).
    if (!FIRST && MODE != 2 && tile0 < tile1) {
        if (wave == 0) {
            const int32_t *in_super = p.in_super + p.seg_in_totals * seg;
            const int A = tile0 * TILE;
            int pre_s = 0, pre_a = 0;
            // (rows of the group table are nsuper wide, entries past a bin's last group are zero: scanned as one flat array)
            int bs = scanFind8(in_super + (size_t)nb * p.nsuper, in_super, nb * p.nsuper, A, pre_s, pre_a, lane);      // A < n_in: there is one
            bs = bs < 0 ? 0 : bs;      // (cannot happen while the tables are what a k_bounce leaves; no address may depend on that)
            const int b = bs / p.nsuper, sg = bs - b * p.nsuper;
            const int rs = b * p.in_gx + sg * 64;                     // first run of the group; its 64 runs hold position A
            int cs[2], ca[2], cb[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int r = rs + h * 64 + lane;
                // (a bin's last group may hold fewer than 64 runs: what follows in the flat table is the next bin's first runs, which
                // are also what follows in sorted order; position A itself lies in the group, i.e. in the first 64)
                const bool in = r < in_nruns;
                ca[h] = in ? in_chunk[r] : 0; cs[h] = in ? in_chunk[p.chunk_cap + r] : 0; cb[h] = in ? in_chunk[2 * p.chunk_cap + r] : 0;
            }
            int xs[2], xa[2];                                         // exclusive prefixes of the 128 entries
            const int is0 = waveInclusiveScan(cs[0], lane), ia0 = waveInclusiveScan(ca[0], lane);
            const int is1 = waveInclusiveScan(cs[1], lane), ia1 = waveInclusiveScan(ca[1], lane);
            const int t0s = __builtin_amdgcn_readlane(is0, 63), t0a = __builtin_amdgcn_readlane(ia0, 63);
            xs[0] = pre_s + is0 - cs[0]; xa[0] = pre_a + ia0 - ca[0];
            xs[1] = pre_s + t0s + is1 - cs[1]; xa[1] = pre_a + t0a + ia1 - ca[1];
            const unsigned long long m = __ballot(pre_s + is0 > A);
            const int w = m ? __ffsll((long long)m) - 1 : 0;          // the run, as an offset into the group
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int e = h * 64 + lane - w;                      // this entry's place in the window that starts at run rs + w
                if (e >= 0 && e < WIN) { win[e] = xs[h]; win[WIN + 1 + e] = xa[h]; win[2 * (WIN + 1) + e] = cb[h]; }
                if (e == WIN) { win[WIN] = xs[h]; win[2 * WIN + 1] = xa[h]; win[2 * (WIN + 1) + WIN] = rs + w + WIN; }
            }
        } else if (p.sc.tri_lds) stageSceneToLds(p.sc, tid - 64, TILE - 64);
        __syncthreads();
    } else if (MODE != 2 && tile0 < tile1 && p.sc.tri_lds) {      // (a workgroup without tiles shades nothing and needs no tables; nor does pass 2)
        stageSceneToLds(p.sc, tid, TILE);
        __syncthreads();
    }
#ifdef PT_WGCLOCK
    const unsigned long long wg_t1 = wall_clock64();
#endif
    struct InRec { float f[14]; int32_t pix, mg, idx; float tf[6]; int32_t has_tf; uint32_t tf4; };      // (tf: the hit's tangent frame where has_tf, at byte tf4 of the table: fetch, fetchFrame)
    // sorted position -> (entry of the local index, RNG stream index of its run's first survivor).  Uniform call: the window
    // moves on (barriers) when the tile's last position lies beyond it -- a few times per workgroup at most.
    auto locate = [&](int tile_, uint32_t &li4, int &idx_base) {
        const int jp = min(tile_ * TILE + tid, n_in - 1), last = min(tile_ * TILE + TILE - 1, n_in - 1);
        bool done = false;
        for (;;) {
            const int wend = win[WIN];
            if (!done && jp < wend) {
                int k = 0;
#pragma unroll
                for (int st = WIN / 2; st; st >>= 1) k += win[k + st] <= jp ? st : 0;      // last run that starts at or before jp
                // (the clamp cannot bite while the tables are consistent: it is there so that no gather address depends on that)
                const uint32_t li = (uint32_t)(win[2 * (WIN + 1) + k] + (jp - win[k]));
                // (an entry of the bin-major index is checked against ITS words, nbins * N2; the slot it names against fence_slots, in fetch)
                const uint32_t li_lim = in_loop ? (uint32_t)nb << n2s : p.fence_slots;
                if (__builtin_expect(li >= li_lim, 0)) fence_report(p);
                li4 = min(li, li_lim - 1u) << 2;
                idx_base = win[WIN + 1 + k];
                done = true;
            }
            // (uniform: every thread reads the same window; the second test cannot hold while the tables are what a k_bounce
            // leaves -- position < n_in lies in some run -- it is there so that the loop ends whatever they hold)
            if (last < wend || win[2 * (WIN + 1) + WIN] >= in_nruns) break;
            __syncthreads();
            if (wave == 0) windowLoad(win, in_chunk, p.chunk_cap, in_nruns, win[2 * (WIN + 1) + WIN], wend, win[2 * WIN + 1], lane);
            __syncthreads();
        }
    };
    auto fetch = [&](uint32_t li4, int idx_base, InRec &r, int jp) -> bool {
        const PathSoA in = soa_fresh(in_k);
        // the sorted stream is not materialised: its position is entry li of the previous bounce's local index, which names the
        // slot of that bounce's stage and the path's rank inside its run
        // (bin-major form: the entry's place in its bin's row is the position inside the writer's chunk the distance counts from)
        const uint32_t w = (uint32_t)ld_u(in_loop ? ix_in : in.lsrc(), li4);
        uint32_t j;
        if (p.in_idx16) { j = (in_loop ? (li4 >> 2) & ((1u << n2s) - 1u) : li4 >> 2) + (uint32_t)(int32_t)(int16_t)(w & 0xffffu); r.idx = idx_base + (int)(w >> 16); }
        else { j = w; r.idx = idx_base + ld_u(in_loop ? ix_in + ((p.loop_idx & 4) ? (size_t)nb << n2s : 0) : in.lidx(), li4); }
        if (__builtin_expect(j >= p.fence_slots, 0)) fence_report(p);
        const uint32_t j4 = min(j, p.fence_slots - 1u) << 2;
        const bool with_dir = (uint32_t)(jp - dir_lo0) < (uint32_t)dir_len0 || (uint32_t)(jp - dir_lo1) < (uint32_t)dir_len1;
        const bool coded_n = (uint32_t)(jp - ntab_lo0) < (uint32_t)ntab_len0 || (uint32_t)(jp - ntab_lo1) < (uint32_t)ntab_len1;
        typedef float quad __attribute__((ext_vector_type(4)));
        const uint32_t j16 = j4 << 2;
        const quad A = ld_u(reinterpret_cast<const quad *>(in.quadA()), j16), B = ld_u(reinterpret_cast<const quad *>(in.quadB()), j16);
        r.f[0] = A.x; r.f[1] = A.y; r.f[2] = A.z; r.pix = __float_as_int(A.w);
        r.f[6] = B.x; r.f[7] = B.y; r.f[8] = B.z; r.mg = __float_as_int(B.w);
        r.f[3] = r.f[4] = r.f[5] = 0.f; r.f[9] = r.f[10] = r.f[11] = 0.f; r.f[12] = r.f[13] = 0.f;
        r.tf[0] = r.tf[1] = r.tf[2] = r.tf[3] = r.tf[4] = r.tf[5] = 0.f; r.has_tf = 0; r.tf4 = 0u;
        // (texcoords matter on OBJ geoms only, whose records have both a normal and a direction: where a part is not read they are the 0 it would hold)
        if (with_dir) { const quad D = ld_u(reinterpret_cast<const quad *>(in.quadD()), j16); r.f[3] = D.x; r.f[4] = D.y; r.f[5] = D.z; if (p.uses_uv) r.f[13] = D.w; }
        if (!coded_n) { const quad C = ld_u(reinterpret_cast<const quad *>(in.quadC()), j16); r.f[9] = C.x; r.f[10] = C.y; r.f[11] = C.z; if (p.uses_uv) r.f[12] = C.w; }
        if (coded_n) {      // the cube's tabulated normal, the words decodeKey took it from (the tile path: the tables are staged)
            // (the geom index comes out of the same untrusted record as the pixel slot below: clamped before it indexes the tables)
            const int g = (int)min((uint32_t)(r.mg >> 16), (uint32_t)(p.sc.ngeoms - 1));
            const vec3 n = cubeNormalByCode(p.sc, reinterpret_cast<const float *>(pt_lds) + p.sc.ntri_lds * 24 + p.sc.nmats * 11, g, (r.pix >> 28) & 7);
            r.f[9] = n.x; r.f[10] = n.y; r.f[11] = n.z;
            // ... and, where the code names a face, the place of the tangent frame the diffuse sampler would build from that normal (DScene::ctan,
            // computed at upload by the sampler's own tangentFrame; requested by fetchFrame below).  The address is made of the clamped geom and
            // a side 0-5, nothing else.
            const int code = (r.pix >> 28) & 7;
            if (p.sc.ctan && (code & 3)) {
                r.tf4 = (uint32_t)(g * CTAN_WORDS + (((code & 3) - 1) * 2 + ((code & 4) ? 1 : 0)) * 6) << 2;
                r.has_tf = 1;
            }
            r.pix &= 0x0fffffff;
        }
        // (fence: the pixel slot becomes the address of the path's radiance when it ends -- found by a record read with other masks than
        // it was written with, end of round 4: a normal code taken for part of the slot.  A fenced record is a DEAD path, as in k_finish:
        // it is counted, and it neither scatters nor adds light to a pixel that is not its own)
        if (__builtin_expect((uint32_t)r.pix >= (uint32_t)p.tm.owned, 0)) { fence_report(p); r.pix = 0; return false; }
        return true;
    };
    // The request of a tabulated frame, the tail of fetch: issued once the record's quads have arrived (`mat` comes out of quad B), so that the
    // three loads do not sit in front of the wait for every load in flight where coded and uncoded records join; read at the end of the sampler.
    auto fetchFrame = [&](InRec &r, int mat) {
        int32_t has = r.has_tf;
        asm volatile("" : "+v"(has) : "v"(mat));      // (opaque, and behind the material index: the block below stays where it is written)
        if (has) {
            typedef float pair __attribute__((ext_vector_type(2)));
            const pair T0 = ld_u(reinterpret_cast<const pair *>(p.sc.ctan), r.tf4), T1 = ld_u(reinterpret_cast<const pair *>(p.sc.ctan), r.tf4 + 8u),
                       T2 = ld_u(reinterpret_cast<const pair *>(p.sc.ctan), r.tf4 + 16u);
            r.tf[0] = T0.x; r.tf[1] = T0.y; r.tf[2] = T1.x; r.tf[3] = T1.y; r.tf[4] = T2.x; r.tf[5] = T2.y;
        }
    };
    auto classifyRay = [&](const Hit &hit, const PathState &ps, int pix, int &bin, bool &pending) {
        classifyPath<FIRST>(p, iter, part, batched, hit, ps.color, pix, bin, pending);
    };
    int32_t *ccnt = qcnt + 2;                                   // MODE 1: candidates of the tile so far (LDS)
    int n_last = 0;                                             // LAST: rays of this wave's tiles that entered the intersection (wave-uniform)
    int32_t *pool_n = tcs;                                      // LAST: rays in the pool of light-box survivors (LDS; the per-bin tile counts are not in use there)
    int32_t k1_next = 0;                                        // MODE 2: the next tile's word, requested one tile ahead
    // The ranking pass (MODE 2) has three barriers per tile: counts by wave 0, keys scattered to their slots through LDS.
    // MEASURED AND NOT KEPT, code removed (round 5, -DPT_RANK_ONE_BARRIER; last in commit 77f3d5a): the pass with ONE barrier per tile --
    // every stored path's key written straight to the slot named in the word pass 1 / k_finish left, no "-1" for slots without a record
    // (the tail read a tile's keys only where records can lie, k_finish marked the parked rays that ended), the per-bin counts as
    // bookkeeping of their owner thread, the histogram alternating between two buffers.  tools/runs/r5f.sh, one box, Lit = three barriers / Rank1 = that
    // form: the pass alone 0.147 -> 0.140 ms per iteration of C5, the wall 0.893 -> 0.904.  The pass is not a chain of barriers after
    // all -- at 4K it moves 0.45 GB per launch in 0.2 ms -- and keys scattered 4 B at a time cost the three launch sets more than its
    // barriers did.
    if (MODE == 2) {                                            // (its histogram: zeroed here once, then after every tile's ranking)
        for (int k = tid; k < 2 * WAVES * nb; k += TILE) lds[k] = 0;
        __syncthreads();
    }
    if (MODE == 2 && !FIRST && tile0 < tile1 && tile0 * TILE + tid < n_in) k1_next = ld_u(soa_fresh(stage_k).lsrc(), (uint32_t)(tile0 * TILE + tid) << 2);
    for (int tile = tile0; tile < tile1; tile++) {
#ifdef PT_STAMPS
        st_t0 = __builtin_amdgcn_s_memtime();
#endif
        const int i = tile * TILE + tid;
        bool alive = i < n_in;
        // camera rays: the geoms this tile's 256 pixels can see at all (host, update_tile_geoms: conservative screen rectangles of the
        // geoms' world boxes): the per-ray candidate masks test only these -- most tiles see two or three of a Cornell scene's seven
        uint32_t tile_subset = 0xffffffffu;
        if (FIRST && MODE != 2 && p.tile_geoms) tile_subset = ((const __attribute__((address_space(4))) uint32_t *)p.tile_geoms)[tile];
        InRec cur;
        uint32_t li4 = 0;
        int idx_base = 0;
        if (!FIRST && MODE != 2) locate(tile, li4, idx_base);
        const PathSoA stage = soa_fresh(stage_k);      // field addresses are formed where they are used
        PathState ps;
        int pix = 0;                 // slot among the owned pixels: what the path carries instead of the pixel index
        // ranking histogram (read after later barriers).  The ranking pass (MODE 2) has no intersection whose barriers would separate
        // this from the ballots' writes: it zeroes the histogram right after a tile's LAST read of it instead (below), and once before
        // its first tile -- three barriers per tile instead of five for a kernel that is a chain of barriers and little else.
        if (MODE != 2 && !direct && !LAST) for (int k = tid; k < 2 * WAVES * nb; k += TILE) lds[k] = 0;      // (the light-only bounce ranks nothing)
        ps.o = ps.d = ps.color = V3(0.f, 0.f, 0.f);
        unsigned long long key = KEY_NONE;
        int32_t k1 = 0;
        if (MODE == 2 && !FIRST) {
            // the word of the NEXT tile is requested before this tile's is used: the ranking pass is otherwise one exposed memory
            // round trip per tile (pass 2 at 4K: 110 -> 85 us per launch; not on the first bounce, most of whose tiles pass 1 finished)
            k1 = k1_next;
            if (tile + 1 < tile1 && i + TILE < n_in) k1_next = ld_u(soa_fresh(stage_k).lsrc(), (uint32_t)(i + TILE) << 2);
        }
        if (MODE == 2 && FIRST && p.tile_done && (p.tile_done + (size_t)p.maxTiles * seg)[tile]) {
            // pass 1 finished this tile (records and keys are in the stage): only its per-bin counts, which pass 1 left in
            // the prefix tables, are folded into this workgroup's running prefix
            for (int b = tid; b < nb; b += TILE) {
                const int ca = counts_all[(size_t)b * p.maxTiles + tile], cs = counts_scat[(size_t)b * p.maxTiles + tile];
                counts_all[(size_t)b * p.maxTiles + tile] = run_all[b];
                counts_scat[(size_t)b * p.maxTiles + tile] = run_scat[b];
                run_all[b] += ca;
                run_scat[b] += cs;
            }
            __syncthreads();      // (thread b is bin b's owner in every tile: nobody else reads the running prefixes before the tail)
            continue;
        }
        int bin = -1;
        bool pending = false, pass1_partial = false;
        int myslot = 0;                  // split bounce: the slot (inside the tile) of this ray's parked state / stored record
        if (MODE == 1 && tid == 0) *ccnt = 0;           // (first touched after tileIntersect's barriers)
        if (MODE == 2) {                 // pass 1 left one word per ray; only the rays with mesh candidates were parked
            alive = false;
            // (every ray is finished by now: by pass 1, or -- the ones with mesh candidates -- by k_finish)
            if (i < n_in) {
                if (FIRST) k1 = ld_u(stage.lsrc(), (uint32_t)i << 2);
                myslot = (k1 >> 16) & (TILE - 1);
                alive = (k1 & K1_ALIVE) != 0; pending = (k1 & K1_PEND) != 0; bin = k1 & 0xffff;
            }
        } else if (alive) {
            if (FIRST) {
                int x, y;
                owned_pixel(p.tm, i, x, y);
                pix = i;                 // the slot; the pixel is (x, y)
                // (a tile that sees no geom at all: its rays miss whatever they are -- none is generated, none is tested)
                if (tile_subset != 0u) generateRay(p.cam, iter, p.traceDepth, p.aa != 0, p.dof != 0, x, y, ps);
            } else {
                // shadeFakeMaterial for a path that is known to scatter (src/pathtrace.cu:391-394)
                const bool rec_ok = fetch(li4, idx_base, cur, min(i, n_in - 1));
                const vec3 intersect = V3(cur.f[0], cur.f[1], cur.f[2]);           // stored as origin + t * direction
                ps.d = V3(cur.f[3], cur.f[4], cur.f[5]);
                ps.color = V3(cur.f[6], cur.f[7], cur.f[8]);
                pix = cur.pix;
                Hit h;
                h.t = 1.f;
                h.n = V3(cur.f[9], cur.f[10], cur.f[11]);
                h.u = cur.f[12]; h.v = cur.f[13];
                const int mg = cur.mg;
                h.mat = mg & 0xffff; h.geom = mg >> 16;
                const int sidx = cur.idx;
                fetchFrame(cur, h.mat);
#ifdef PT_STAMPS
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                STAMP(11);
#endif
                Rng rng; rng.seed(iter, sidx, 0);
                TanFrame tf;
                tf.perp1 = V3(cur.tf[0], cur.tf[1], cur.tf[2]); tf.perp2 = V3(cur.tf[3], cur.tf[4], cur.tf[5]); tf.has = cur.has_tf;
                bool ended = (FAST && MODE == 0) ? scatterRayT<false, true>(p.sc, ps, intersect, h, getMaterial(p.sc, h.mat), rng, tf)
                                                 : scatterRayT<true, true>(p.sc, ps, intersect, h, getMaterial(p.sc, h.mat), rng, tf);
                if (ended && rec_ok) deposit(p.tm, p.image, part, batched, pix, ps.color, p.apps, p.fence_slots_cap);      // emissive texel: remainingBounces 1 -> 0, colour goes to the image
                if (ended || !rec_ok) alive = false;
            }
        }
        STAMP(0);        // load + shade (or ray generation)
        if (LAST) {
            n_last += __popcll(__ballot(alive));              // rays that enter this bounce's intersection (rays_per_bounce)
            if (p.sc.light_bits == 0u) continue;                 // (uniform) nothing in the scene emits: every path ends black
            Ray ray; ray.o = ps.o; ray.d = ps.d;
            const bool reach = alive && cullMask<true>(p.sc, ray, p.sc.light_bits) != 0u;
            // The few rays that reach a light's box (a 3 x 3 lamp on a 10 x 10 ceiling: a few per cent of a tile) are not tested where they
            // are -- the pair machinery would run on every tile for a handful of lanes per wave -- but POOLED over the workgroup's tiles in
            // the record buffer (this launch stores no record): origin and direction in the rows tileIntersect keeps its copy of the rays in
            // (0-5), throughput colour and pixel slot behind its scratch (rows 12-15).  A slot = the pool's count + the ray's place among the
            // tile's survivors (ballot prefix, one LDS atomic per wave, as MODE 1's `ccnt`); the slot index is computed by ALL lanes, in
            // front of the branch (a readfirstlane inside a divergent branch reads the first ACTIVE lane).  When TILE rays are pooled, or
            // after the workgroup's last tile, the pool is DRAINED: thread t takes pooled ray t through tileIntersect, once, and the winner's
            // material decides the deposit with the POOLED colour and pixel slot.  Rays of the tile that found the pool full wait in their
            // registers and go in behind the drain.  Which lane makes a deposit changes no sum: a pixel has one path per iteration and
            // segment, and a path deposits once.  p.last_inplace (debug): every tile is drained by itself, ray t in slot t -- the in-place form.
            // The general kernel (!FAST) keeps that form: the rays that wait across a drain cost it seven registers, 92 -> 99, one wave of five.
            const bool inplace = !FAST || p.last_inplace != 0;
            const unsigned long long rb = __ballot(reach);
            int pbase = 0;
            if (!inplace && lane == 0 && rb) pbase = atomicAdd(pool_n, __popcll(rb));
            int slot = inplace ? tid : __builtin_amdgcn_readfirstlane(pbase) + wavePrefix(rb, lane);
            float *poolf = reinterpret_cast<float *>(rec);
            auto pool_put = [&](int s) {                                      // (s < TILE: the caller's test)
                poolf[0 * TILE + s] = ray.o.x; poolf[1 * TILE + s] = ray.o.y; poolf[2 * TILE + s] = ray.o.z;
                poolf[3 * TILE + s] = ray.d.x; poolf[4 * TILE + s] = ray.d.y; poolf[5 * TILE + s] = ray.d.z;
                poolf[12 * TILE + s] = ps.color.x; poolf[13 * TILE + s] = ps.color.y; poolf[14 * TILE + s] = ps.color.z;
                rec[15 * TILE + s] = pix;
            };
            if (reach && (uint32_t)slot < (uint32_t)TILE) pool_put(slot);
            __syncthreads();
            int total = inplace ? TILE : *pool_n;                      // (uniform; every count since the last drain)
            while (total >= TILE || (tile == tile1 - 1 && total > 0)) {
                const int n = min(max(total, 0), TILE);                        // (a bad count costs pixels, never an address)
                const bool pa = tid < n && (!inplace || reach);
                Ray pr;
                pr.o = V3(poolf[0 * TILE + tid], poolf[1 * TILE + tid], poolf[2 * TILE + tid]);
                pr.d = V3(poolf[3 * TILE + tid], poolf[4 * TILE + tid], poolf[5 * TILE + tid]);
                Hit none;                                         // (never read: no decode)
                uint32_t mesh_cand = 0;
                tileIntersect<false, false, false, false>(p.sc, pa, pr, false, none, rec, tcnt, tq, tid, lane, wave, key, mesh_cand TI_PASS);
                if (tid == 0) *pool_n = total - n;                // (everybody read the count before tileIntersect's barriers)
                if (pa && key != KEY_NONE) {
                    // the winner's material; classifyPath with a hit that holds what it reads (t > 0: the key functions accept nothing else)
                    const float *G = reinterpret_cast<const float *>(pt_lds) + p.sc.ntri_lds * 24 + p.sc.nmats * 11 + (int)((key >> 24) & 0xff) * GTAB_WORDS;
                    Hit lh;
                    lh.t = 1.f; lh.n = V3(0.f, 0.f, 0.f); lh.u = lh.v = 0.f; lh.geom = 0; lh.ncode = 0;
                    lh.mat = __float_as_int(G[37]);
                    PathState pps;
                    pps.o = pr.o; pps.d = pr.d;
                    pps.color = V3(poolf[12 * TILE + tid], poolf[13 * TILE + tid], poolf[14 * TILE + tid]);
                    const int ppix = rec[15 * TILE + tid];
                    int lbin = 0;
                    bool lpend = false;
                    // (the pooled slot went through LDS: checked again before it becomes the address of a deposit)
                    if ((uint32_t)ppix < (uint32_t)p.tm.owned) classifyRay(lh, pps, ppix, lbin, lpend);
                    else fence_report(p);
                }
                total -= n;
                if (!FAST) break;                                 // (in place, known at compile time: no ray waits)
                __syncthreads();                                  // the pool's rows are free: the rays that waited go in
                slot -= TILE;
                if (reach && (uint32_t)slot < (uint32_t)TILE) pool_put(slot);
                __syncthreads();
            }
            STAMP(1);
            continue;
        }
        // computeIntersections(b) + the terminal cases of shadeFakeMaterial(b)
        Hit hit;
        hit.t = -1.f; hit.n = V3(0.f, 0.f, 0.f); hit.u = hit.v = 0.f; hit.geom = 0; hit.mat = 0; hit.ncode = 0;
        if (FIRST && MODE == 0 && tile_subset == 0u) {
            // Camera rays of a tile into which no geom's box projects (the wide margins of the Cornell frames: a third of C4's tiles):
            // every ray misses.  Nothing is generated, tested, ranked or stored -- the paths end black (their slot of the radiance buffer is
            // written), the tile's keys say "no record", and what moves on is the count of survivors in the miss bin (material 0), which
            // the stream indices of the next bounce and the ray statistics are made of.  (The per-tile prefix tables are only ever read
            // for stored paths: this tile has none.)
            int mbin = 0;
            bool mpend = false;
            if (alive) classifyRay(hit, ps, pix, mbin, mpend);
            if (!loop_w && tid == 0) tile_np[tile] = 0;
            if (tid == 0) run_all[p.sort ? p.sc.nmats - 1 : 0] += min(TILE, n_in - tile * TILE);
            continue;
        }
        if (FIRST && MODE == 1 && tile_subset == 0u && p.tile_done) {
            // the same in pass 1 of the split bounce: the tile is "finished in pass 1" (tile_done) with nothing stored; its per-bin counts --
            // all survivors in the miss bin -- go into the prefix tables as they are, pass 2 folds them into its running prefix
            int mbin = 0;
            bool mpend = false;
            if (alive) classifyRay(hit, ps, pix, mbin, mpend);
            if (tid == 0) tile_np[tile] = 0;
            const int missbin = p.sort ? p.sc.nmats - 1 : 0, nalive = min(TILE, n_in - tile * TILE);
            for (int b = tid; b < nb; b += TILE) {
                counts_all[(size_t)b * p.maxTiles + tile] = b == missbin ? nalive : 0;
                counts_scat[(size_t)b * p.maxTiles + tile] = 0;
            }
            if (tid == 0) (p.tile_done + (size_t)p.maxTiles * seg)[tile] = 1;
            continue;
        }
        {
            Ray ray; ray.o = ps.o; ray.d = ps.d;
            uint32_t mesh_cand = 0;
            if (MODE == 1) {
                if (FIRST && tile_subset == 0u) __syncthreads();      // (the histogram is zeroed: what tileIntersect's barriers see to otherwise)
                else tileIntersect<true, false, FIRST>(p.sc, alive, ray, p.uses_uv != 0, hit, rec, tcnt, tq, tid, lane, wave, key, mesh_cand TI_PASS, tile_subset);
                // Camera rays are coherent: most tiles of the first bounce (256 neighbouring pixels of a row) hold no ray that
                // reaches a mesh's box at all.  Such a tile is finished right here -- winner's normal, terminal cases,
                // ranking, in-tile sort, stage write, as in the unsplit kernel -- instead of being parked and picked up again;
                // its per-bin counts go into the prefix tables as they are, pass 2 folds them into its running prefix.
                bool finish_here = false;
                if (FIRST && p.tile_done) {
                    finish_here = !__syncthreads_or(mesh_cand != 0u);
                    if (tid == 0) (p.tile_done + (size_t)p.maxTiles * seg)[tile] = finish_here ? 1 : 0;
                }
                if (finish_here) {
                    if (alive) decodeKey<true>(p.sc, reinterpret_cast<const float *>(pt_lds) + p.sc.ntri_lds * 24 + p.sc.nmats * 11, key, ray,
                                         p.uses_uv != 0, hit);
                    goto classify;
                }
                // A ray WITH mesh candidates is parked -- origin, direction, colour, pixel, best key so far, in a slot of its own
                // counted down from the top of the tile -- and its candidates are queued with that slot.  A ray without -- 93 % of
                // them past the first bounce -- is finished right here like the unsplit kernel would: nearest hit, terminal cases,
                // ranked and sorted by bin among its like, record written to the bottom of the tile; pass 2 gets ONE word about it
                // (round 3; rounds 1-2 parked every ray: 48 B out and 48 B back in for each, which is what bounded the two passes).
                // What pass 2 still does for all is the ranking that defines the order: it needs every ray's bin, and the
                // candidates' are not known before k_mesh / k_finish.
                pass1_partial = true;
                {
                    const bool is_cand = mesh_cand != 0u;                        // (implies alive)
                    const unsigned long long cb = __ballot(is_cand);
                    int cbase = 0;
                    if (lane == 0 && cb) cbase = atomicAdd(ccnt, __popcll(cb));
                    myslot = TILE - 1 - (__builtin_amdgcn_readfirstlane(cbase) + wavePrefix(cb, lane));
                    const int sa = tile * TILE + myslot;
                    if (is_cand) {
                        stage.px()[sa] = ray.o.x; stage.py()[sa] = ray.o.y; stage.pz()[sa] = ray.o.z;
                        stage.dx()[sa] = ray.d.x; stage.dy()[sa] = ray.d.y; stage.dz()[sa] = ray.d.z;
                        stage.cr()[sa] = ps.color.x; stage.cg()[sa] = ps.color.y; stage.cb()[sa] = ps.color.z;
                        stage.pix()[sa] = pix;
                        stage.mg()[sa] = i;                                      // whose ray this is: k_finish writes the verdict to lsrc[i]
                        stage.nx()[sa] = __int_as_float((int)mesh_cand);         // the meshes whose boxes it reaches (bit per geom)
                        (p.keys + p.seg_keys * seg)[sa] = key;
                        k1 = K1_CAND | (myslot << 16);
                    }
                    // one queue entry per parked ray -- its slot; which meshes it is a candidate for travels with the ray -- through an
                    // LDS buffer (behind the record buffer) to the global queue in blocks: one global atomic per ~50 tiles instead of
                    // one per wave (a single hot counter)
                    int base = 0;
                    if (lane == 0 && cb) base = atomicAdd(qcnt, __popcll(cb));
                    const int qi = __builtin_amdgcn_readfirstlane(base) + wavePrefix(cb, lane);      // (lane 0's value: read by all lanes)
                    if (is_cand) qbuf[qi] = (uint32_t)sa;
                    if (is_cand) alive = false;                                  // not part of pass 1's ranking and records
                }
                if (alive) decodeKey<true>(p.sc, reinterpret_cast<const float *>(pt_lds) + p.sc.ntri_lds * 24 + p.sc.nmats * 11, key, ray,
                                     p.uses_uv != 0, hit);
                goto classify;
            } else if (MODE == 2) {
                rec[tid] = -1;                                    // this slot's key, until a stored path claims the slot (keybuf below;
                                                                  // the barriers of the ranking lie between this and the claims)
            } else if (p.sc.cull) {
                // The specialised kernel is compiled for PT_FAST_WAVES waves per SIMD, i.e. 72 registers.  The thread's own state
                // that is only needed again after the intersection -- throughput colour and pixel slot; the ray itself is in
                // tileIntersect's LDS copy anyway -- therefore waits in a free part of the record buffer instead of in
                // registers: the pair tests are where the register demand peaks.  (MODE 1 needs more than parking frees and
                // stays at 4 waves, where parking only costs LDS traffic; MODE 2 fits 96 registers as it is.)
                constexpr bool PARK = FAST && PT_PARK_STATE;
                float *park = reinterpret_cast<float *>(rec) + 12 * TILE;
                {
                    if (PARK) {
                        park[0 * TILE + tid] = ps.color.x; park[1 * TILE + tid] = ps.color.y; park[2 * TILE + tid] = ps.color.z;
                        rec[15 * TILE + tid] = pix;
                    }
                    tileIntersect<false, PARK, FIRST>(p.sc, alive, ray, p.uses_uv != 0, hit, rec, tcnt, tq, tid, lane, wave, key, mesh_cand TI_PASS, tile_subset);
                    if (PARK) {
                        asm volatile("" ::: "memory");
                        const float *rb = reinterpret_cast<const float *>(rec);
                        ps.o = V3(rb[0 * TILE + tid], rb[1 * TILE + tid], rb[2 * TILE + tid]);
                        ps.d = V3(rb[3 * TILE + tid], rb[4 * TILE + tid], rb[5 * TILE + tid]);
                        ps.color = V3(park[0 * TILE + tid], park[1 * TILE + tid], park[2 * TILE + tid]);
                        pix = rec[15 * TILE + tid];
                    }
                }
            }
            else {
                if (alive) intersectScene(p.sc, ray, hit);
                __syncthreads();                                  // histogram zeroed (tileIntersect has barriers of its own)
            }
        }
        STAMP(1);        // intersect
    classify:
        // (direct epilogue: this wave's rows of the ranking histogram -- every path to here has passed a barrier of THIS tile, so no wave
        // is still summing the previous tile's)
        if (MODE != 2 && direct && lane < nb) { w_all[wave * nb + lane] = 0; w_scat[wave * nb + lane] = 0; }
        if (MODE != 2 && alive) classifyRay(hit, ps, pix, bin, pending);
        // Bin-major index: the chunk's survivors / stored paths of this path's bin BEFORE this tile -- what the tail used to gather back from
        // counts_all / counts_scat.  Ordering: run_all / run_scat are written (a) by wave 0 in the epilogue of a tile, behind that tile's
        // ranking barrier below, and (b) by thread 0 in the camera bounce's empty-tile shortcut, which has no barrier of its own but which
        // thread 0 can only reach behind the ranking barrier of the tile before it.  Every path to here has passed a barrier of THIS tile
        // (the pair test's, or the one in its place), which every write of an earlier tile precedes in its writer's program order; and this
        // tile's write (a) lies behind the ranking barrier, which no wave passes before every wave has made this read.  So the read sees
        // exactly the earlier tiles' sums, in every wave.
        int pre_all = 0, pre_scat = 0;
        if (loop_w && pending) { pre_all = run_all[bin]; pre_scat = run_scat[bin]; }
        STAMP(2);        // classify + deposit
        // stable rank of this path inside its tile, per material bin: among all alive paths (-> RNG stream
        // index) and among the stored ones (-> storage position)
        int r_all = 0, r_scat = 0;
        {
            // a lane's bin as ONE integer per question (-1: not part of it): a bin's lanes are then a single v_cmp_eq into a scalar pair
            // (a ballot of `flag && bin == b` makes the compiler materialise the flag first), and the rank among them two v_mbcnt: 15
            // vector instructions per bin that occurs in the wave instead of 28.  (Visiting EVERY bin in turn instead -- no readlane,
            // no find-first -- is 13 per bin and loses: camera rays see two or three of the eight bins.)
            const int abin = alive ? bin : -1, pbin = pending ? bin : -1;
            if (PT_RANK_SLICED && MODE != 2 && !FIRST && nb <= 16) {
                // Up to 16 bins, later bounces (a wave of scattered rays sees four or five of the bins): bit-sliced.  Four ballots give the
                // lanes whose bin has bit k set; a lane ANDs together, per bit of its OWN bin, that mask or its complement -- the lanes of
                // its bin, as a 64-bit value of its own -- and ranks itself with v_mbcnt on it: ~30 vector instructions whatever the number
                // of bins, where the loop below costs ~15 per bin that occurs.  (Camera rays see two or three bins: they keep the loop.)
                const unsigned long long A = __builtin_amdgcn_uicmp((uint32_t)abin, 0xffffffffu, 33), P = __builtin_amdgcn_uicmp((uint32_t)pbin, 0xffffffffu, 33);
                uint32_t slo = 0xffffffffu, shi = 0xffffffffu;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (k && (nb - 1) >> k == 0) break;                       // (uniform: bins below 2^k need no more bits)
                    const unsigned long long Bk = __builtin_amdgcn_uicmp((uint32_t)bin & (1u << k), 0u, 33);
                    const bool set = (bin >> k) & 1;
                    slo &= set ? (uint32_t)Bk : ~(uint32_t)Bk;
                    shi &= set ? (uint32_t)(Bk >> 32) : ~(uint32_t)(Bk >> 32);
                }
                const uint32_t alo = slo & (uint32_t)A, ahi = shi & (uint32_t)(A >> 32), plo = slo & (uint32_t)P, phi = shi & (uint32_t)(P >> 32);
                const int ra = (int)__builtin_amdgcn_mbcnt_hi(ahi, __builtin_amdgcn_mbcnt_lo(alo, 0u));
                const int rs = (int)__builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
                if (alive) {
                    r_all = ra; r_scat = rs;
                    if (ra == 0) {                                              // the first lane of its bin in this wave: the wave's counts
                        w_all[wave * nb + bin] = __popc(alo) + __popc(ahi);
                        w_scat[wave * nb + bin] = __popc(plo) + __popc(phi);
                    }
                }
            } else if (PT_WAVE_UNIFORM && FIRST && MODE != 2 && __builtin_amdgcn_uicmp((uint32_t)abin, (uint32_t)__builtin_amdgcn_readfirstlane(abin), 32) == ~0ull &&
                       __builtin_amdgcn_readfirstlane(abin) >= 0) {
                // Camera rays: a wave of 64 neighbouring pixels that all hit the same material (every lane alive, one bin) -- most waves of a
                // Cornell frame.  The rank among all is the lane, the wave's count 64; among the stored ones the same if all are stored, nothing
                // if none is, and one prefix otherwise: the loop below with its single turn spelt out, minus what is known.
                const int b = __builtin_amdgcn_readfirstlane(abin);
                const unsigned long long m_scat = __builtin_amdgcn_uicmp((uint32_t)pbin, (uint32_t)b, 32);
                r_all = lane;
                r_scat = m_scat == ~0ull ? lane : m_scat == 0ull ? 0 : wavePrefix(m_scat, lane);
                if (lane == 0) {
                    w_all[wave * nb + b] = 64;
                    w_scat[wave * nb + b] = __popcll(m_scat);
                }
            } else {
                unsigned long long remaining = __builtin_amdgcn_uicmp((uint32_t)abin, 0xffffffffu, 33);       // (alive lanes)
                while (remaining) {
                    int leader = __ffsll((long long)remaining) - 1;
                    int b = __builtin_amdgcn_readlane(abin, leader);      // (leader is wave-uniform: no LDS round trip as __shfl would make)
                    const unsigned long long m_all = __builtin_amdgcn_uicmp((uint32_t)abin, (uint32_t)b, 32), m_scat = __builtin_amdgcn_uicmp((uint32_t)pbin, (uint32_t)b, 32);
                    const int ra = wavePrefix(m_all, lane), rs = wavePrefix(m_scat, lane);
                    if (abin == b) { r_all = ra; r_scat = rs; }
                    if (lane == leader) {
                        w_all[wave * nb + b] = __popcll(m_all);
                        w_scat[wave * nb + b] = __popcll(m_scat);
                    }
                    remaining &= ~m_all;
                }
            }
        }
        STAMP(12);       // (ranking: ballots)
        __syncthreads();
        STAMP(13);       // (ranking: wait at its first barrier)
        if (alive) {
            for (int w = 0; w < wave; w++) { r_all += w_all[w * nb + bin]; r_scat += w_scat[w * nb + bin]; }
        }
        int toff_bin = 0, npend_r = 0;       // direct epilogue: this path's bin's offset in the tile, the tile's stored paths
        if (direct) {
            int ln = lane;                   // (opaque, see below)
            asm volatile("" : "+v"(ln));
            int ca = 0, cs = 0;
            if (ln < nb) for (int w = 0; w < WAVES; w++) { ca += w_all[w * nb + ln]; cs += w_scat[w * nb + ln]; }
            if (wave == 0 && ln < nb) {      // the tile's place in the chunk: one wave's business, as before
                if (!loop_w) {               // (bin-major index: nobody reads the tables, every pending lane took its prefix from LDS above)
                    counts_all[(size_t)ln * p.maxTiles + tile] = MODE == 1 ? ca : run_all[ln];
                    counts_scat[(size_t)ln * p.maxTiles + tile] = MODE == 1 ? cs : run_scat[ln];
                }
                run_all[ln] += ca;
                run_scat[ln] += cs;
            }
            const int inc = waveInclusiveScan(cs, ln);
            npend_r = __builtin_amdgcn_readlane(inc, 63);              // (lanes >= nb add 0)
            toff_bin = __builtin_amdgcn_ds_bpermute((bin < 0 ? 0 : bin) << 2, inc - cs);
            STAMP(14);
        } else if (nb <= 64) {
            // wave 0: lane b owns bin b -- tile counts, running prefixes and the in-tile offsets by a wave scan
            if (wave == 0) {
                // `ln` = lane, but opaque to the optimiser: otherwise the per-lane addresses below are loop invariants,
                // get hoisted out of the tile loop, and -- the kernel being at its register limit -- are spilled to
                // scratch, whose reloads (memory latency, one after the other) then sit on every tile's critical path
                int ln = lane;
                asm volatile("" : "+v"(ln));
                int ca = 0, cs = 0;
                if (ln < nb) {
                    for (int w = 0; w < WAVES; w++) { ca += w_all[w * nb + ln]; cs += w_scat[w * nb + ln]; }
                    // (MODE 1 finishing a tile: the tile's own counts, for pass 2 to fold in)
                    counts_all[(size_t)ln * p.maxTiles + tile] = MODE == 1 ? ca : run_all[ln];
                    counts_scat[(size_t)ln * p.maxTiles + tile] = MODE == 1 ? cs : run_scat[ln];
                    run_all[ln] += ca;
                    run_scat[ln] += cs;
                }
                const int inc = waveInclusiveScan(cs, ln);
                if (ln < nb) toff[ln] = inc - cs;
                if (ln == nb - 1) toff[nb] = inc;
            }
            STAMP(14);   // (ranking: counts, wave 0's scan)
            __syncthreads();
        } else {
            for (int b = tid; b < nb; b += TILE) {
                int ca = 0, cs = 0;
                for (int w = 0; w < WAVES; w++) { ca += w_all[w * nb + b]; cs += w_scat[w * nb + b]; }
                counts_all[(size_t)b * p.maxTiles + tile] = MODE == 1 ? ca : run_all[b];
                counts_scat[(size_t)b * p.maxTiles + tile] = MODE == 1 ? cs : run_scat[b];
                run_all[b] += ca;
                run_scat[b] += cs;
                tcs[b] = cs;
            }
            __syncthreads();
            if (tid == 0) {
                int o = 0;
                for (int b = 0; b < nb; b++) { toff[b] = o; o += tcs[b]; }
                toff[nb] = o;
            }
            __syncthreads();
        }
        STAMP(3);        // ranking + counts
        if (MODE == 2) {                 // the records lie in their slots already (pass 1, or above): only the keys are left,
            int32_t *keybuf = rec;       // one per SLOT (through LDS: a path's slot is not its thread), -1 where no record lies
            for (int k = tid; k < 2 * WAVES * nb; k += TILE) lds[k] = 0;      // (w_all / w_scat were last read before the barriers above;
                                                                               // the barrier below is in front of the next tile's ballots)
            if (pending) keybuf[myslot] = stage_key(bin, r_all, r_scat);
            __syncthreads();
            // (stored paths fill the slots from the bottom -- pass 1's records and k_finish's parked ones are not contiguous: keys for every slot)
            st_u(soa_fresh(stage_k).idx(), (uint32_t)i << 2, keybuf[tid]);
            if (FIRST && tid == 0) tile_np[tile] = TILE;          // (this form writes a key for every slot; the camera bounce's tail looks the counts
                                                                  // up -- the tiles pass 1 finished have fewer keys --, a later bounce's knows)
            continue;
        }
        if (direct) {
            const PathSoA stage = soa_fresh(stage_k);
            const bool partial = MODE == 1 && pass1_partial;         // (pass 2 writes such a tile's keys and its count)
            if (partial && i < n_in) {
                if (alive) k1 = K1_ALIVE | bin | (pending ? K1_PEND | ((toff_bin + r_scat) << 16) : 0);
                st_u(stage.lsrc(), (uint32_t)i << 2, k1);
            }
            if (pending) {
                const uint32_t g4 = (uint32_t)(tile * TILE + toff_bin + r_scat) << 2, g16 = g4 << 2;
                const vec3 sp = add(ps.o, scale(ps.d, hit.t));      // the point shadeFakeMaterial will shade (:392)
                const bool with_dir = !dir_some || ((p.dir_bins >> bin) & 1ull);
                const bool coded_n = ntab_some && ((p.ntab_bins >> bin) & 1ull);
                typedef float quad __attribute__((ext_vector_type(4)));
                quad A, B;
                A.x = sp.x; A.y = sp.y; A.z = sp.z; A.w = __int_as_float(coded_n ? (pix | (hit.ncode << 28)) : pix);
                B.x = ps.color.x; B.y = ps.color.y; B.z = ps.color.z; B.w = __int_as_float(hit.mat | (hit.geom << 16));
                st_u(reinterpret_cast<quad *>(stage.quadA()), g16, A);
                st_u(reinterpret_cast<quad *>(stage.quadB()), g16, B);
                if (with_dir) {
                    quad D;
                    D.x = ps.d.x; D.y = ps.d.y; D.z = ps.d.z; D.w = p.uses_uv ? hit.v : 0.f;
                    st_u(reinterpret_cast<quad *>(stage.quadD()), g16, D);
                }
                if (!coded_n) {
                    quad C;
                    C.x = hit.n.x; C.y = hit.n.y; C.z = hit.n.z; C.w = p.uses_uv ? hit.u : 0.f;
                    st_u(reinterpret_cast<quad *>(stage.quadC()), g16, C);
                }
                if (loop_w) {
                    // the path's word of the local index, at bin * N2 + (its position in the chunk): both operands of the distance lie in
                    // the chunk's slot range (pos <= slot: a bin's stored paths of the earlier tiles are at most those tiles' slots), so
                    // it fits wherever idx16 holds today, and so does the rank.  The entry is checked against the index's words before it
                    // is an address.
                    const uint32_t pos = (uint32_t)(tile0 * TILE + pre_scat + r_scat), e = ((uint32_t)bin << n2s) + pos, slot = g4 >> 2;
                    const uint32_t rank = (uint32_t)(pre_all + r_all);
                    if (__builtin_expect(e >= (uint32_t)nb << n2s, 0)) fence_report(p);
                    else if (p.idx16) st_u(ix_out, e << 2, (int32_t)(((slot - pos) & 0xffffu) | (rank << 16)));
                    else if (p.loop_idx & 4) {      // (the second table exists: the host's plan, not this launch, says so)
                        st_u(ix_out, e << 2, (int32_t)slot);
                        st_u(ix_out + ((size_t)nb << n2s), e << 2, (int32_t)rank);
                    } else fence_report(p);
                } else if (!partial) st_u(stage.idx(), g4, stage_key(bin, r_all, r_scat));
            }
            // stored paths of the tile: pass 1's own lie in slots [0, n); a partial tile's parked rays in the top *ccnt slots.  (The top
            // count is vestigial: only the removed one-barrier ranking pass let the tail read it -- the ranking pass that is left writes a key for
            // every slot and overwrites this word with TILE, or the tail takes TILE as known, so the tail's top-of-tile test never bites.  It
            // stays so that the kernels' instruction streams are the ones measured.)
            if (!loop_w && tid == 0) tile_np[tile] = npend_r | (partial ? *ccnt << 16 : 0);
            STAMP(4);
            if (MODE == 1 && *qcnt > QCAP - TILE) flushQueue(p, seg, qbuf, qcnt, qbase, tid);      // (uniform: the tile's last atomic on it lies before the ranking's barrier)
            continue;
        }
        if (MODE == 1 && pass1_partial && i < n_in) {
            if (alive) k1 = K1_ALIVE | bin | (pending ? K1_PEND | ((toff[bin] + r_scat) << 16) : 0);
            st_u(soa_fresh(stage_k).lsrc(), (uint32_t)i << 2, k1);
        }
        // Stored paths go to the stage sorted by bin inside the tile (through LDS), so that both this write and
        // the tail's read are dense and coalesced and the next bounce's gather reads per-bin runs.
        if (pending) {
            const int slot = toff[bin] + r_scat;
            const vec3 sp = add(ps.o, scale(ps.d, hit.t));      // the point shadeFakeMaterial will shade (:392)
            float *rf = reinterpret_cast<float *>(rec);
            rf[0 * TILE + slot] = sp.x; rf[1 * TILE + slot] = sp.y; rf[2 * TILE + slot] = sp.z;
            if (!dir_some || ((p.dir_bins >> bin) & 1ull)) { rf[3 * TILE + slot] = ps.d.x; rf[4 * TILE + slot] = ps.d.y; rf[5 * TILE + slot] = ps.d.z; }
            rf[6 * TILE + slot] = ps.color.x; rf[7 * TILE + slot] = ps.color.y; rf[8 * TILE + slot] = ps.color.z;
            const bool coded_n = ntab_some && ((p.ntab_bins >> bin) & 1ull);
            if (!coded_n) { rf[9 * TILE + slot] = hit.n.x; rf[10 * TILE + slot] = hit.n.y; rf[11 * TILE + slot] = hit.n.z; }
            if (p.uses_uv) { rf[12 * TILE + slot] = hit.u; rf[13 * TILE + slot] = hit.v; }
            rec[R_PIX * TILE + slot] = coded_n ? (pix | (hit.ncode << 28)) : pix;
            rec[R_MG * TILE + slot] = hit.mat | (hit.geom << 16);
            rec[R_KEY * TILE + slot] = stage_key(bin, r_all, r_scat);
        }
        __syncthreads();
        {
            const PathSoA stage = soa_fresh(stage_k);
            const int npend = toff[nb];
            const uint32_t gi4 = (uint32_t)(tile * TILE + tid) << 2;
            if (tid < npend) {
                const float *rf = reinterpret_cast<const float *>(rec);
                const int32_t skey = rec[R_KEY * TILE + tid];
                // (this slot's record carries a direction iff its bin says so: the reader decides by the same bins, from the sorted position)
                const bool with_dir = !dir_some || ((p.dir_bins >> (skey & ((1 << BIN_BITS) - 1))) & 1ull);
                const bool coded_n = ntab_some && ((p.ntab_bins >> (skey & ((1 << BIN_BITS) - 1))) & 1ull);
                typedef float quad __attribute__((ext_vector_type(4)));
                const uint32_t gi16 = gi4 << 2;
                quad A, B;
                A.x = rf[0 * TILE + tid]; A.y = rf[1 * TILE + tid]; A.z = rf[2 * TILE + tid]; A.w = rf[R_PIX * TILE + tid];
                B.x = rf[6 * TILE + tid]; B.y = rf[7 * TILE + tid]; B.z = rf[8 * TILE + tid]; B.w = rf[R_MG * TILE + tid];
                st_u(reinterpret_cast<quad *>(stage.quadA()), gi16, A);
                st_u(reinterpret_cast<quad *>(stage.quadB()), gi16, B);
                if (with_dir) {
                    quad D;
                    D.x = rf[3 * TILE + tid]; D.y = rf[4 * TILE + tid]; D.z = rf[5 * TILE + tid]; D.w = p.uses_uv ? rf[13 * TILE + tid] : 0.f;
                    st_u(reinterpret_cast<quad *>(stage.quadD()), gi16, D);
                }
                if (!coded_n) {
                    quad C;
                    C.x = rf[9 * TILE + tid]; C.y = rf[10 * TILE + tid]; C.z = rf[11 * TILE + tid]; C.w = p.uses_uv ? rf[12 * TILE + tid] : 0.f;
                    st_u(reinterpret_cast<quad *>(stage.quadC()), gi16, C);
                }
                st_u(stage.idx(), gi4, skey);
            } else {
                st_u(stage.idx(), gi4, (int32_t)-1);
            }
            if (tid == 0) tile_np[tile] = npend | ((MODE == 1 && pass1_partial) ? *ccnt << 16 : 0);
        }
        __syncthreads();
        STAMP(4);        // sort through LDS + stage write
        if (MODE == 1 && *qcnt > QCAP - TILE) flushQueue(p, seg, qbuf, qcnt, qbase, tid);      // (uniform: read after a barrier)
    }
#ifdef PT_STAMPS
    if (lane == 0 && p.stamps && (blockIdx.x & 15) == 0)           // (a sample of the workgroups: atomics of all of them on 16 words outlast a short kernel)
        for (int k = 0; k < 16; k++) atomicAdd(&p.stamps[(FIRST ? 0 : 16) + k], st_acc[k]);
#endif
#ifdef PT_WGCLOCK
    const unsigned long long wg_t2 = wall_clock64();
#endif
    if (LAST) {                          // nothing was stored: no tail.  The rays counted, one atomic per wave (every lane holds the wave's sum)
        if (lane == 0 && n_last) atomicAdd(&totals_all[0], n_last);
        return;
    }
    if (MODE == 1) {                     // counts belong to MODE 2; what is left in the LDS queue goes out now
        if (*qcnt > 0) flushQueue(p, seg, qbuf, qcnt, qbase, tid);
        return;
    }
    // Tail of the sort ("local move").  run_all / run_scat now hold this chunk's survivors / stored paths per bin.  The chunk's
    // stored paths get their place in (bin, tile, rank) order INSIDE the chunk -- cbb[bin] = stored paths of the chunk in earlier
    // bins, + the tile's prefix inside the chunk, + the rank in the tile -- and at that place of the chunk's region of the local
    // index go the path's stage slot and its rank among all survivors of its bin in the chunk.  Nothing of another workgroup is
    // needed, so there is no wait; what IS global (the position of a run in the whole stream) the next launch derives from the
    // run table below.
    // Bin-major index (loop_w): the words were written in the tile loop; a run starts at bin * N2 + the chunk's first slot, so neither the
    // scan over the bins nor the pass over the keys is left -- only the run table and the totals.  (The barrier stays: thread b reads
    // what wave 0 and, in the camera bounce's empty tiles, thread 0 added.)
    int32_t *cbb = toff;                                              // (free after the tile loop)
    if (!loop_w && nb <= 64) {
        if (wave == 0) {
            const int v = lane < nb ? run_scat[lane] : 0;
            const int inc = waveInclusiveScan(v, lane);
            if (lane < nb) cbb[lane] = inc - v;
        }
    } else if (!loop_w && tid == 0) {
        int o = 0;
        for (int b = 0; b < nb; b++) { cbb[b] = o; o += run_scat[b]; }
    }
    __syncthreads();
    for (int b = tid; b < nb; b += TILE) {
        const int ca = run_all[b], cs = run_scat[b];
        const size_t r = (size_t)b * gridDim.x + blockIdx.x;
        chunk_out[r] = ca;
        chunk_out[(size_t)p.chunk_cap + r] = cs;
        chunk_out[2 * (size_t)p.chunk_cap + r] = loop_w ? (int32_t)(((uint32_t)b << n2s) + (uint32_t)(tile0 * TILE)) : tile0 * TILE + cbb[b];
        if (ca) { atomicAdd(&super_all[b * p.nsuper + (blockIdx.x >> 6)], ca); atomicAdd(&totals_all[b], ca); }
        if (cs) { atomicAdd(&super_scat[b * p.nsuper + (blockIdx.x >> 6)], cs); atomicAdd(&totals_scat[b], cs); }
    }
    if (!loop_w) {
        const PathSoA stage = soa_fresh(stage_k);
        const int32_t *keys = stage.idx();
        constexpr int MOVE_U = 4;                                     // tiles per step: their keys are requested before the first is used
        // (only the slots that hold a record are read: the tile's stored count, left by whoever finished the tile -- requested one step
        // ahead, so that the keys stay ONE round trip per step; the ranking pass of a later bounce wrote a key for every slot itself)
        // (the ranking pass of a later bounce wrote a key for every slot of every tile: nothing to look up)
        constexpr bool NP_ALL = MODE == 2 && !FIRST;
        int np_next[MOVE_U];                                          // (stored paths at the bottom of the tile | parked rays at its top << 16)
#pragma unroll
        for (int u = 0; u < MOVE_U; u++) np_next[u] = tile0 + u < tile1 ? (NP_ALL ? TILE : tile_np[tile0 + u]) : 0;
        for (int tbase = tile0; tbase < tile1; tbase += MOVE_U) {
            int32_t key[MOVE_U];
            int np_cur[MOVE_U];
#pragma unroll
            for (int u = 0; u < MOVE_U; u++) {
                np_cur[u] = np_next[u];
                np_next[u] = tbase + MOVE_U + u < tile1 ? (NP_ALL ? TILE : tile_np[tbase + MOVE_U + u]) : 0;
            }
#pragma unroll
            for (int u = 0; u < MOVE_U; u++)
                key[u] = (tid < (np_cur[u] & 0xffff) || tid >= TILE - (np_cur[u] >> 16)) ? ld_u(keys, (uint32_t)((tbase + u) * TILE + tid) << 2) : -1;
#pragma unroll
            for (int u = 0; u < MOVE_U; u++) {
                if (key[u] == -1) continue;
                const int tile = tbase + u;
                const int bin = key[u] & ((1 << BIN_BITS) - 1), r_all = (key[u] >> BIN_BITS) & (TILE - 1), r_scat = (int)((uint32_t)key[u] >> (BIN_BITS + RANK_BITS));
                const uint32_t c4 = (uint32_t)(bin * p.maxTiles + tile) << 2;      // (a segment's table is below 4 GiB: ptx_create)
                const int pos = tile0 * TILE + cbb[bin] + ld_u(counts_scat, c4) + r_scat;
                const int slot = tile * TILE + tid, rank = ld_u(counts_all, c4) + r_all;
                if (p.idx16) st_u(stage.lsrc(), (uint32_t)pos << 2, (int32_t)(((uint32_t)(slot - pos) & 0xffffu) | ((uint32_t)rank << 16)));
                else {
                    st_u(stage.lsrc(), (uint32_t)pos << 2, (int32_t)slot);
                    st_u(stage.lidx(), (uint32_t)pos << 2, (int32_t)rank);
                }
            }
        }
    }
#ifdef PT_WGCLOCK
    // (diagnostic build -DPT_WGCLOCK: a slot of its own per (kind, segment of the first 64, workgroup) -- plain adds, no shared address)
    if (tid == 0 && p.stamps && tile1 > tile0 && seg < 64 && blockIdx.x < 4096) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long wg_t3 = wall_clock64();
        unsigned long long *w = p.stamps + 48 + ((size_t)((FIRST ? 0 : 1) * 64 + seg) * 4096 + blockIdx.x) * 5;
        w[0] += wg_t1 - wg_t0; w[1] += wg_t2 - wg_t1; w[2] += wg_t3 - wg_t2; w[3] += 1ull; w[4] += (unsigned long long)(tile1 - tile0);
    }
#endif
}

// Split mesh search, middle part (round 4: refilling waves).  The queue holds one entry per PARKED ray (its stage slot); which
// meshes' boxes the ray reaches travels with it as a bit per geom.  The search of one ray is a walk of unpredictable length -- 9 wide
// nodes and 6 triangles on average on the 20 448-triangle stand-in, the longest of 64 consecutive rays 3-5 times that -- and rounds 2-3
// gave every lane ONE ray: a wave then issues for its slowest lane, 19 % of the lanes active per vector instruction (round 3's
// counters; tools/mesh_walk_sim.cpp reproduces 16 % on the CPU from the walks' step sequences).  Ordering the queue by direction
// octant / entry cell so that neighbouring lanes walk alike buys 5-10 % (same simulator: the spread is in the LENGTHS, not in the
// paths).  So a wave now keeps its lanes busy instead: it draws chunks of the queue (one global atomic per PT_MESHQ_CHUNK entries and
// wave, on a per-segment cursor), every lane holds the walk state of one ray (WideWalk, pt_device.h), and the wave alternates
//   * a NODE round  -- the lanes whose walk holds an inner node do one four-wide node step -- while at least PT_MESH_NMIN lanes do, or
//                      no lane holds a leaf;
//   * a LEAF round  -- the lanes that hold a leaf test its triangles, all of them (ONE triangle per round, -DPT_MESH_ONE_TRI, measured
//                      0.61 against 0.54 ms per iteration at 4K -- the kernel waits for memory more than it issues, and a leaf's
//                      triangles share cache lines; that switch was last in commit 77f3d5a);
//   * a TURNOVER    -- once PT_MESH_REFILL lanes have nothing to walk (or nothing else is left to do): walks that ended fold their
//                      key into the ray's (minimum of the meshes' keys and the key pass 1 left: cubes and spheres), rays with another
//                      candidate mesh set up its walk, finished rays store their key, free lanes take the next queue entries.
// Same steps on the same data per ray -- wideNodeStep / wideLeafStep are what bvhNearestWide runs -- so the same keys (every mesh test
// green on either schedule); per 64 rays the simulator counts 7.0 k instead of 16.7 k instruction slots (with 220 per turnover and 25
// per round of scheduling), 42 % of the lanes active.  The finishing of the rays (hit decode, terminal cases, record) is k_finish
// again, one dense lane per queue entry: its code and registers do not ride along with the walks.
// Exit: every wave ends when the cursor has passed the queue's end and none of its lanes holds a ray -- each round advances every lane
// it runs, each turnover consumes queue entries or retires rays, so the loop ends for any queue content (bad entries are fenced).
template <bool FIRST>
__global__ __launch_bounds__(256, PT_MESH_WAVES) void k_mesh(const BounceParams p_in, int bvh_stack) {
    const BounceParams &p = p_in;
    const int seg = blockIdx.y;
    const int n = p.item_count[seg];
    const int lane = threadIdx.x & 63;
    const PathSoA st = soa_offset(p.stage, p.seg_stage * seg);
    const uint32_t *items = p.items + p.seg_items * seg;
    unsigned long long *keys = p.keys + p.seg_keys * seg;
    int32_t *cursor = p.item_cursor + seg;
    const uint32_t slots = p.fence_slots;
    const int ngeoms = p.sc.ngeoms < 32 ? p.sc.ngeoms : 32;
    const uint32_t geom_mask = ngeoms >= 32 ? 0xffffffffu : (1u << ngeoms) - 1u;
    // dynamic LDS: [bvh_stack][256] the walks' stacks, then what a walk's set-up needs per geom -- one LDS read where the geom table, the
    // three per-geom tree tables and the root node were a chain of dependent global loads in front of every walk
    int32_t *stack = pt_lds + threadIdx.x;
    float *gl = reinterpret_cast<float *>(pt_lds + (size_t)bvh_stack * 256);
    if ((int)threadIdx.x < ngeoms) {
        const int gi = threadIdx.x;
        float *o = gl + gi * MESH_GEOM_WORDS;
        const float *G = p.sc.gtab + gi * GTAB_WORDS;
        for (int k = 0; k < 12; k++) o[k] = G[k];
        const int root = p.sc.bvh_root ? p.sc.bvh_root[gi] : -1;
        const bool wideok = root >= 0 && p.sc.bvh_wroot && p.sc.bvh_wroot[gi] >= 0 && p.sc.bvh_wneed[gi] <= bvh_stack;
        BvhQuad A, B;
        A.x = A.y = A.z = B.x = B.y = B.z = 0.f; A.w = B.w = 0;
        if (wideok) { A = p.sc.bvh_nodes[2 * root]; B = p.sc.bvh_nodes[2 * root + 1]; }
        o[12] = A.x; o[13] = A.y; o[14] = A.z; o[15] = B.x; o[16] = B.y; o[17] = B.z;
        o[18] = __int_as_float(wideok ? p.sc.bvh_wroot[gi] : -1); o[19] = 0.f;
    }
    __syncthreads();
    constexpr int32_t IDLE = (int32_t)0x80000001;             // (no leaf reference looks like this either: count 0)
    // per-lane state: the ray in hand (sa: its stage slot; < 0: none), the meshes still to search, the ones left to k_finish, the best
    // key so far, the walk
    int32_t sa = -1, g = 0;
    uint32_t mask = 0, rest = 0;
    unsigned long long key = KEY_NONE;
    WideWalk w;
    w.n = IDLE; w.sp = 0; w.tmin = 0.f; w.face = -1; w.b0 = w.b1 = 0.f;
    w.o = w.d = V3(0.f, 0.f, 0.f); w.ix = w.iy = w.iz = w.enx = w.eny = w.enz = w.efx = w.efy = w.efz = 0.f;
    int cur = 0, end = 0;                                    // (wave-uniform) the chunk of the queue this wave is drawing from
    bool more = n > 0;                                       // (wave-uniform) the queue may still hold entries for this wave
    for (;;) {
        const int n_node = __popcll(__ballot(w.n >= 0)), n_done = __popcll(__ballot(w.n == WIDE_DONE)), n_idle = __popcll(__ballot(w.n == IDLE));
        const int n_leaf = 64 - n_node - n_done - n_idle;
        // lanes a turnover would retire or give a walk: walks that ended, and -- while the queue still has entries -- lanes without a ray
        const int n_wait = more ? n_done + n_idle : n_done;
        if (n_node + n_leaf == 0 || n_wait >= PT_MESH_REFILL) {
            // ---- turnover -----------------------------------------------------------------------------------------------------
            if (w.n == WIDE_DONE) {                          // a walk ended: its key (meshKey's packing: object-space distance, geom, face)
                const float t = w.face >= 0 ? w.tmin : -1.f;
                if (t > 0.0f && t < 3.402823466e+38f) { const unsigned long long km = packKey(t, g, (uint32_t)w.face); key = km < key ? km : key; }
                w.n = IDLE;
            }
            if (more) {                                      // free lanes take the next queue entries
                const unsigned long long m_free = __ballot(w.n == IDLE && !mask);      // (no walk, no mesh left: the ray in hand, if any, retires below)
                if (cur >= end && m_free) {
                    int b = 0;
                    if (lane == 0) b = atomicAdd(cursor, PT_MESHQ_CHUNK);
                    cur = __builtin_amdgcn_readfirstlane(b);
                    end = min(cur + PT_MESHQ_CHUNK, n);
                    if (cur >= n) { more = false; cur = end = 0; }
                }
                const int take = min(__popcll(m_free), end - cur);
                const int mine = wavePrefix(m_free, lane);
                if (w.n == IDLE && !mask) {
                    if (sa >= 0) {                           // every candidate mesh of the ray in hand is searched (or left to k_finish): its key is final here
                        keys[sa] = key;
                        st.nx()[sa] = __int_as_float((int)rest);
                        sa = -1;
                    }
                    if (mine < take) {
                        const uint32_t e = items[cur + mine];
                        if (e < slots) {                     // (fence: a queue entry is a slot of the stage, whatever wrote it)
                            sa = (int32_t)e;
                            key = keys[sa];
                            mask = (uint32_t)__float_as_int(st.nx()[sa]) & geom_mask;
                            rest = 0;
                        } else fence_report(p);
                    }
                }
                cur += take;
            } else if (w.n == IDLE && !mask && sa >= 0) {
                keys[sa] = key;
                st.nx()[sa] = __int_as_float((int)rest);
                sa = -1;
            }
            if (sa >= 0 && w.n == IDLE) {                    // (mask != 0 here) set up the walk of the ray's next candidate mesh
                const vec3 ro = V3(st.px()[sa], st.py()[sa], st.pz()[sa]), rd = V3(st.dx()[sa], st.dy()[sa], st.dz()[sa]);
                while (mask && w.n == IDLE) {
                    g = __ffs((int)mask) - 1;
                    mask &= mask - 1;
                    const float *L = gl + g * MESH_GEOM_WORDS;
                    const int wroot = __float_as_int(L[18]);
                    if (wroot >= 0) {
                        float inv[12];
#pragma unroll
                        for (int k = 0; k < 12; k++) inv[k] = L[k];
                        // (= multiplyMV(geom.inverseTransform, ., .) of meshTestCore: same products, same sums)
                        const vec3 qo = mulRows(inv, ro, 1.0f), qd = normalize(mulRows(inv, rd, 0.0f));
                        BvhQuad A, B;
                        A.x = L[12]; A.y = L[13]; A.z = L[14]; A.w = 0; B.x = L[15]; B.y = L[16]; B.z = L[17]; B.w = 0;
                        wideStart(w, A, B, wroot, qo, qd);
                        if (w.n == WIDE_DONE) w.n = IDLE;    // the root box is missed: no key from this mesh, on to the next
                    } else rest |= 1u << g;                  // a mesh without a four-wide tree (too small for one, or its walk would not fit the
                                                             // stack): k_finish searches it, with the loop or the stackless walk
                }
            }
            if (!more && !__ballot(sa >= 0)) break;
            continue;
        }
        if (n_node >= PT_MESH_NMIN || n_leaf == 0) {
            if (w.n >= 0) wideNodeStep(w, p.sc.bvh_wide, stack, 256);
        } else {
            if (w.n != WIDE_DONE && w.n != IDLE && w.n < 0) wideLeafStep<false>(w, p.sc.bvh_tris, stack, 256);
        }
    }
}

// Split mesh search, last part: one lane per parked ray finishes it -- nearest hit decoded from the final key, terminal cases, the
// record completed in the slot the ray was parked in if it goes on, and the one word pass 2 needs left in lsrc[owner].  Dense lanes
// that all do the same thing: the dependent face / texel loads of a textured mesh hit hide behind the other waves.
template <bool FIRST>
__global__ __launch_bounds__(256) void k_finish(const BounceParams p_in) {
    BounceParams p = p_in;
    p.sc.tri_lds = 0; p.sc.ntri_lds = 0;
    const int seg = blockIdx.y;
    const int iter = p.iter + seg * p.iter_stride;
    const int n = p.item_count[seg];
    const PathSoA st = soa_offset(p.stage, p.seg_stage * seg);
    const uint32_t *items = p.items + p.seg_items * seg;
    const unsigned long long *keys = p.keys + p.seg_keys * seg;
    float *part = p.part ? p.part + p.seg_part * seg : nullptr;
    const bool batched = part != nullptr;
    const uint32_t slots = p.fence_slots;
    const uint32_t geom_mask = p.sc.ngeoms >= 32 ? 0xffffffffu : (1u << p.sc.ngeoms) - 1u;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const int sa = (int)items[k];
        if ((uint32_t)sa >= slots) { fence_report(p); continue; }      // (fence: a queue entry is a slot of the stage, whatever wrote it)
        Ray ray;
        ray.o = V3(st.px()[sa], st.py()[sa], st.pz()[sa]);
        ray.d = V3(st.dx()[sa], st.dy()[sa], st.dz()[sa]);
        unsigned long long key = keys[sa];
        // the candidate meshes k_mesh did not search (no four-wide tree: small meshes of a split scene, trees too deep for the walks' stack):
        // the plain loop or the stackless walk, same keys, same minimum
        for (uint32_t m = (uint32_t)__float_as_int(st.nx()[sa]) & geom_mask; m; m &= m - 1) {
            const unsigned long long km = meshKey(p.sc, p.sc.gtab, __ffs((int)m) - 1, ray);
            key = km < key ? km : key;
        }
        const int owner = st.mg()[sa], pix = st.pix()[sa];
        if ((uint32_t)owner >= slots || (uint32_t)pix >= (uint32_t)p.tm.owned) { fence_report(p); continue; }
        const vec3 color = V3(st.cr()[sa], st.cg()[sa], st.cb()[sa]);
        Hit hit;
        decodeKey(p.sc, p.sc.gtab, key, ray, p.uses_uv != 0, hit);
        int bin = 0;
        bool pending = false;
        classifyPath<FIRST>(p, iter, part, batched, hit, color, pix, bin, pending);
        if (pending) {
            const vec3 sp = add(ray.o, scale(ray.d, hit.t));          // the point shadeFakeMaterial will shade (:392)
            st.px()[sa] = sp.x; st.py()[sa] = sp.y; st.pz()[sa] = sp.z;
            // (direction, colour and pixel are in place; a record of a cubes-only material carries its normal as a code in the pixel word)
            if (p.nbins <= 64 && ((p.ntab_bins >> bin) & 1ull)) st.pix()[sa] = pix | (hit.ncode << 28);
            else { st.nx()[sa] = hit.n.x; st.ny()[sa] = hit.n.y; st.nz()[sa] = hit.n.z; }
            if (p.uses_uv) { st.u()[sa] = hit.u; st.v()[sa] = hit.v; }
            st.mg()[sa] = hit.mat | (hit.geom << 16);
        }
        st.lsrc()[owner] = K1_ALIVE | (pending ? K1_PEND : 0) | bin | ((sa & (TILE - 1)) << 16);
    }
}

#ifndef PT_KERNELS_LAST_UNIT
// ---- per-stage kernels for the parity tests (AoS records of the reference in, same out) ----------------------
__global__ void k_kat_geom(DScene sc, int gi, int n, const float *rays, float *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DGeom &g = sc.geoms[gi];
    Ray r; r.o = ld3(rays + i * 6); r.d = ld3(rays + i * 6 + 3);
    vec3 p = V3(0, 0, 0), nrm = V3(0, 0, 0);
    float u = 0.f, v = 0.f;
    bool outside = true;
    float t = -1.f;
    if (g.type == G_CUBE) t = boxIntersectionTest(g, r, p, nrm, outside);
    else if (g.type == G_SPHERE) t = sphereIntersectionTest(g, r, p, nrm, outside);
    else if (g.type == G_OBJ) t = meshIntersectionTest(sc, g, r, p, nrm, u, v, outside, sc.bvh_root ? sc.bvh_root[gi] : -1);
    float *o = out + i * 10;
    o[0] = t; o[1] = p.x; o[2] = p.y; o[3] = p.z; o[4] = nrm.x; o[5] = nrm.y; o[6] = nrm.z; o[7] = u; o[8] = v;
    o[9] = outside ? 1.f : 0.f;
}

// the reference's dead objTriIntersectionTest (src/intersections.h:284-315) on an OBJ geom: out per ray = t, point, normal, outside
__global__ void k_kat_obj_tri(DScene sc, int gi, int n, const float *rays, float *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DGeom &g = sc.geoms[gi];
    Ray r; r.o = ld3(rays + i * 6); r.d = ld3(rays + i * 6 + 3);
    vec3 p = V3(0, 0, 0), nrm = V3(0, 0, 0);
    bool outside = true;
    const float t = g.type == G_OBJ ? objTriTest(sc, g, r, p, nrm, outside) : -1.f;
    float *o = out + i * 8;
    o[0] = t; o[1] = p.x; o[2] = p.y; o[3] = p.z; o[4] = nrm.x; o[5] = nrm.y; o[6] = nrm.z; o[7] = outside ? 1.f : 0.f;
}

// the reference's dead calculateJitteredDirectionHemisphere (src/interactions.h:46-85): normal + (iter, index, depth) -> direction
__global__ void k_kat_jittered(int n, const float *normals, const int32_t *seeds, int max_iter, float *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rng; rng.seed(seeds[i * 3], seeds[i * 3 + 1], seeds[i * 3 + 2]);
    const vec3 d = jitteredDirectionInHemisphere(ld3(normals + i * 3), rng, seeds[i * 3], max_iter);
    out[i * 3] = d.x; out[i * 3 + 1] = d.y; out[i * 3 + 2] = d.z;
}

__global__ void k_kat_intersect(DScene sc, int n, const HostPath *paths, HostIsect *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r; r.o = ld3(paths[i].o); r.d = ld3(paths[i].d);
    Hit h;
    intersectScene(sc, r, h);
    HostIsect o;
    memset(&o, 0, sizeof o);
    if (h.t > 0.f) {
        o.t = h.t; o.n[0] = h.n.x; o.n[1] = h.n.y; o.n[2] = h.n.z; o.materialId = h.mat; o.uv[0] = h.u; o.uv[1] = h.v;
        o.geomId = h.geom;
    } else {
        o.t = -1.f;
    }
    out[i] = o;
}

// computeIntersections as PRODUCTION runs it, on arbitrary rays: candidate masks from the world boxes (cullMask), the tile's (ray, geom)
// pairs pooled in LDS and tested by primKey / meshKey, 64-bit LDS minimum, winner decoded by decodeKey -- tileIntersect itself, with
// the scene tables staged as k_bounce stages them.  SPLIT: the three pieces of the split mesh search instead -- tileIntersect<DEFER>
// (pass 1), meshKey with the stack traversal for every mesh of the ray's candidate mask, folded in by minimum, and decodeKey (k_mesh).
// A named test for the functions that the frame-level parity tests only reach through whole bounces.
template <bool SPLIT>
__global__ __launch_bounds__(TILE) void k_kat_tile(DScene sc, DScene scg, int n, const HostPath *paths, HostIsect *out, int uses_uv) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t *lds = pt_lds + sceneLdsWords(sc);
    int32_t *tcnt = lds;                                             // [8] (the rest of the head is unused here)
    int32_t *rec = lds + ldsHeadWords(1);
    int32_t *stack = rec + REC_WORDS;                                // SPLIT: [bvh_stack][TILE]
    stageSceneToLds(sc, tid, TILE);
    if (tid < 8) tcnt[tid] = 0;
    __syncthreads();
    int tq = 0;
    const float *gtab_lds = reinterpret_cast<const float *>(pt_lds) + sc.ntri_lds * 24 + sc.nmats * 11;
    for (int base = blockIdx.x * TILE; base < n; base += gridDim.x * TILE) {
        const int i = base + tid;
        const bool alive = i < n;
        Ray ray; ray.o = ray.d = V3(0.f, 0.f, 0.f);
        if (alive) { ray.o = ld3(paths[i].o); ray.d = ld3(paths[i].d); }
        Hit h;
        h.t = -1.f; h.n = V3(0.f, 0.f, 0.f); h.u = h.v = 0.f; h.geom = 0; h.mat = 0;
        unsigned long long key = KEY_NONE;
        uint32_t mesh_cand = 0;
#ifdef PT_STAMPS
        unsigned long long st_acc[16] = {0}, st_t0 = 0;        // (the phase-timing build: this kernel's stamps go nowhere)
#endif
        if (!SPLIT) {
            tileIntersect<false>(sc, alive, ray, uses_uv != 0, h, rec, tcnt, tq, tid, lane, wave, key, mesh_cand TI_PASS);
        } else {
            tileIntersect<true>(sc, alive, ray, uses_uv != 0, h, rec, tcnt, tq, tid, lane, wave, key, mesh_cand TI_PASS);
            for (uint32_t m = mesh_cand; m; m &= m - 1) {
                const unsigned long long k = meshKey(scg, scg.gtab, __ffs((int)m) - 1, ray, -1, stack + tid, TILE);
                key = k < key ? k : key;
            }
            if (alive) decodeKey(sc, gtab_lds, key, ray, uses_uv != 0, h);
        }
        if (alive) {
            HostIsect o;
            memset(&o, 0, sizeof o);
            if (h.t > 0.f) { o.t = h.t; o.n[0] = h.n.x; o.n[1] = h.n.y; o.n[2] = h.n.z; o.materialId = h.mat; o.uv[0] = h.u; o.uv[1] = h.v; o.geomId = h.geom; }
            else o.t = -1.f;
            out[i] = o;
        }
        __syncthreads();                                             // (tileIntersect's scratch is reused by the next tile)
        __syncthreads();
    }
}

// shadeFakeMaterial in full (src/pathtrace.cu:365-403), one path per thread, idx[] = RNG stream indices
__global__ void k_kat_shade(DScene sc, int iter, int n, const int32_t *idx, const HostIsect *isects, HostPath *paths) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    HostIsect is = isects[i];
    HostPath seg = paths[i];
    if (is.t > 0.0f) {
        const DMaterial &m = sc.mats[is.materialId];
        if (m.emittance > 0.0f) {
            vec3 c = mul(ld3(seg.c), scale(V3(m.color[0], m.color[1], m.color[2]), m.emittance));
            seg.c[0] = c.x; seg.c[1] = c.y; seg.c[2] = c.z;
            seg.remainingBounces = 0;
        } else if (seg.remainingBounces == 1) {
            seg.c[0] = seg.c[1] = seg.c[2] = 0.f;
            seg.remainingBounces = 0;
        } else {
            PathState ps; ps.o = ld3(seg.o); ps.d = ld3(seg.d); ps.color = ld3(seg.c);
            Hit h; h.t = is.t; h.n = ld3(is.n); h.u = is.uv[0]; h.v = is.uv[1]; h.mat = is.materialId; h.geom = is.geomId;
            Rng rng; rng.seed(iter, idx[i], 0);
            vec3 intersect = add(ps.o, scale(ps.d, h.t));
            bool ended = scatterRay(sc, ps, intersect, h, m, rng);
            seg.o[0] = ps.o.x; seg.o[1] = ps.o.y; seg.o[2] = ps.o.z;
            seg.d[0] = ps.d.x; seg.d[1] = ps.d.y; seg.d[2] = ps.d.z;
            seg.c[0] = ps.color.x; seg.c[1] = ps.color.y; seg.c[2] = ps.color.z;
            if (ended) seg.remainingBounces = 1;
            seg.remainingBounces -= 1;
        }
    } else {
        seg.c[0] = seg.c[1] = seg.c[2] = 0.f;
        seg.remainingBounces = 0;
    }
    paths[i] = seg;
}

__global__ void k_kat_generate(DCamera cam, int iter, int traceDepth, int aa, int dof, HostPath *paths) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int n = cam.resx * cam.resy;
    if (i >= n) return;
    int y = i / cam.resx, x = i - y * cam.resx;
    PathState ps;
    generateRay(cam, iter, traceDepth, aa != 0, dof != 0, x, y, ps);
    HostPath seg;
    seg.o[0] = ps.o.x; seg.o[1] = ps.o.y; seg.o[2] = ps.o.z;
    seg.d[0] = ps.d.x; seg.d[1] = ps.d.y; seg.d[2] = ps.d.z;
    seg.c[0] = ps.color.x; seg.c[1] = ps.color.y; seg.c[2] = ps.color.z;
    seg.pixelIndex = i; seg.remainingBounces = traceDepth;
    paths[i] = seg;
}

__global__ void k_kat_libm(int n, const float *x, float *s, float *c, const double *pw, double *p5,
                           const float *pxy, float *pout) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float sn, cs;
    sincos_pt(x[i], &sn, &cs);          // (the routine the samplers call: sincos_own at the exact level)
    s[i] = sn; c[i] = cs;
    p5[i] = pow5_own(pw[i]);
    pout[i] = powf_own(pxy[2 * i], pxy[2 * i + 1]);
}

// ---- the launchers (KernelSet, pt_kernels.h) ------------------------------------------------------------------------------------
template <bool FIRST, int MODE>
void launch_bounce_variant(bool fast, dim3 grid, size_t lds, hipStream_t stream, const BounceParams &bp) {
    if (fast) hipLaunchKernelGGL((k_bounce<FIRST, MODE, true>), grid, dim3(TILE), lds - (MODE == 0 ? sizeof(int32_t) * (17 - REC_ROWS_FAST0) * TILE : 0), stream, bp);
    else hipLaunchKernelGGL((k_bounce<FIRST, MODE, false>), grid, dim3(TILE), lds, stream, bp);
}
void ks_bounce(int first, int mode, int fast, dim3 grid, size_t lds, hipStream_t stream, const void *params) {
    const BounceParams &bp = *static_cast<const BounceParams *>(params);
    if (first) {
        if (mode == 0) launch_bounce_variant<true, 0>(fast != 0, grid, lds, stream, bp);
        else if (mode == 1) launch_bounce_variant<true, 1>(fast != 0, grid, lds, stream, bp);
        else launch_bounce_variant<true, 2>(fast != 0, grid, lds, stream, bp);
    } else {
        if (mode == 0) launch_bounce_variant<false, 0>(fast != 0, grid, lds, stream, bp);
        else if (mode == 1) launch_bounce_variant<false, 1>(fast != 0, grid, lds, stream, bp);
        else launch_bounce_variant<false, 2>(fast != 0, grid, lds, stream, bp);
    }
}
void ks_mesh(int first, dim3 grid, size_t lds, hipStream_t stream, const void *params, int bvh_stack) {
    const BounceParams &bp = *static_cast<const BounceParams *>(params);
    if (first) hipLaunchKernelGGL(k_mesh<true>, grid, dim3(256), lds, stream, bp, bvh_stack);
    else hipLaunchKernelGGL(k_mesh<false>, grid, dim3(256), lds, stream, bp, bvh_stack);
}
void ks_finish(int first, dim3 grid, hipStream_t stream, const void *params) {
    const BounceParams &bp = *static_cast<const BounceParams *>(params);
    if (first) hipLaunchKernelGGL(k_finish<true>, grid, dim3(256), 0, stream, bp);
    else hipLaunchKernelGGL(k_finish<false>, grid, dim3(256), 0, stream, bp);
}
void ks_kat_geom(dim3 grid, hipStream_t st, const void *scene, int gi, int n, const float *rays, float *out) {
    hipLaunchKernelGGL(k_kat_geom, grid, dim3(256), 0, st, *static_cast<const DScene *>(scene), gi, n, rays, out);
}
void ks_kat_obj_tri(dim3 grid, hipStream_t st, const void *scene, int gi, int n, const float *rays, float *out) {
    hipLaunchKernelGGL(k_kat_obj_tri, grid, dim3(256), 0, st, *static_cast<const DScene *>(scene), gi, n, rays, out);
}
void ks_kat_jittered(dim3 grid, hipStream_t st, int n, const float *normals, const int32_t *seeds, int max_iter, float *out) {
    hipLaunchKernelGGL(k_kat_jittered, grid, dim3(256), 0, st, n, normals, seeds, max_iter, out);
}
void ks_kat_intersect(dim3 grid, hipStream_t st, const void *scene, int n, const void *paths, void *out) {
    hipLaunchKernelGGL(k_kat_intersect, grid, dim3(256), 0, st, *static_cast<const DScene *>(scene), n, static_cast<const HostPath *>(paths), static_cast<HostIsect *>(out));
}
void ks_kat_tile(int split, dim3 grid, size_t lds, hipStream_t st, const void *sc, const void *scg, int n, const void *paths, void *out, int uses_uv) {
    const DScene &a = *static_cast<const DScene *>(sc), &b = *static_cast<const DScene *>(scg);
    if (split) hipLaunchKernelGGL(k_kat_tile<true>, grid, dim3(TILE), lds, st, a, b, n, static_cast<const HostPath *>(paths), static_cast<HostIsect *>(out), uses_uv);
    else hipLaunchKernelGGL(k_kat_tile<false>, grid, dim3(TILE), lds, st, a, b, n, static_cast<const HostPath *>(paths), static_cast<HostIsect *>(out), uses_uv);
}
void ks_kat_shade(dim3 grid, hipStream_t st, const void *scene, int iter, int n, const int32_t *idx, const void *isects, void *paths) {
    hipLaunchKernelGGL(k_kat_shade, grid, dim3(256), 0, st, *static_cast<const DScene *>(scene), iter, n, idx, static_cast<const HostIsect *>(isects), static_cast<HostPath *>(paths));
}
void ks_kat_generate(dim3 grid, hipStream_t st, const void *cam, int iter, int traceDepth, int aa, int dof, void *paths) {
    hipLaunchKernelGGL(k_kat_generate, grid, dim3(256), 0, st, *static_cast<const DCamera *>(cam), iter, traceDepth, aa, dof, static_cast<HostPath *>(paths));
}
void ks_kat_libm(dim3 grid, hipStream_t st, int n, const float *x, float *s, float *c, const double *pw, double *p5, const float *pxy, float *pout) {
    hipLaunchKernelGGL(k_kat_libm, grid, dim3(256), 0, st, n, x, s, c, pw, p5, pxy, pout);
}
int ks_bounce_occupancy(size_t lds) {
    int n = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_bounce<false, 0, true>, TILE, lds) == hipSuccess ? n : -2;
}
const KernelSet g_kernels_here = {PT_ARITH, ks_bounce, ks_mesh, ks_finish, ks_kat_geom, ks_kat_intersect, ks_kat_obj_tri, ks_kat_jittered, ks_kat_tile, ks_kat_shade, ks_kat_generate, ks_kat_libm, ks_bounce_occupancy};

}  // namespace

// all this translation unit exports: its table
#define PT_ARITH_EXPORT_(n) ptx_arith_kernels_##n
#define PT_ARITH_EXPORT(n) PT_ARITH_EXPORT_(n)
extern "C" const void *PT_ARITH_EXPORT(PT_ARITH_TAG)(void) { return &g_kernels_here; }

#else   // PT_KERNELS_LAST_UNIT
// pt_kernels_last.hip: this source again, per level, for ONE thing -- the light-only last bounce (k_bounce<false, MODE_LAST, .>), a code
// object of its own beside the level's pt_kernels.hip one.  Nothing else is instantiated here (k_mesh, k_finish are templates nobody
// names; the test kernels and the launcher table are compiled out), and pt_kernels.hip itself does not instantiate this mode: the
// kernels of that unit are exactly the ones they were.
void ks_bounce_last(int fast, dim3 grid, size_t lds, hipStream_t stream, const void *params) {
    const BounceParams &bp = *static_cast<const BounceParams *>(params);
    // (launched in place of k_bounce<false, 0, fast> where last_violation (pt_engine.hip) allows it, with the same grid and the same LDS)
    if (fast) hipLaunchKernelGGL((k_bounce<false, MODE_LAST, true>), grid, dim3(TILE), lds - sizeof(int32_t) * (17 - REC_ROWS_FAST0) * TILE, stream, bp);
    else hipLaunchKernelGGL((k_bounce<false, MODE_LAST, false>), grid, dim3(TILE), lds, stream, bp);
}
const LastKernelSet g_last_here = {PT_ARITH, ks_bounce_last};

}  // namespace

// all this translation unit exports: its launcher
#define PT_LAST_EXPORT_(n) ptx_arith_last_##n
#define PT_LAST_EXPORT(n) PT_LAST_EXPORT_(n)
extern "C" const void *PT_LAST_EXPORT(PT_ARITH_TAG)(void) { return &g_last_here; }
#endif
