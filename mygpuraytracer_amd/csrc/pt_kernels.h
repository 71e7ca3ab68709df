// pt_kernels.h -- what the kernel unit (pt_kernels.hip, one code object per arithmetic level) and the host unit (pt_engine.hip, exact
// level only) must agree on, and nothing else: every compile-time tunable with its default (`make EXTRA=-D...` reaches both units),
// the constants derived from them, the LDS layout, the plain structs that cross a launch (PathSoA, TileMap, BounceParams, the test
// kernels' records, the launcher table KernelSet) and the small device helpers that kernels on both sides call.  A kernel, or a
// helper only one side uses, does not belong here.  Compiled at every level: included after `ptd` has its name for the translation
// unit (pt_kernels.hip renames it), so DScene -- and with it BounceParams -- is that level's type; everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_device.h"
#include "pt_bvh.h"

using namespace ptd;

namespace {

#ifndef PT_TILE
#define PT_TILE 256
#endif
#ifndef PT_MESH_WAVES
#define PT_MESH_WAVES 5       // waves per SIMD k_mesh is compiled for
#endif
#ifndef PT_PARK_STATE
#define PT_PARK_STATE 1       // specialised unsplit k_bounce: state that is idle during the pair tests waits in LDS, not in registers
#endif
#ifndef PT_PACKED_SLOTS
#define PT_PACKED_SLOTS 1
#endif
#ifndef PT_WAVE_UNIFORM
#define PT_WAVE_UNIFORM 1     // camera bounce: pair-list slots and ranks in closed form for a wave whose 64 lanes agree (0: A/B builds)
#endif
#ifndef PT_FAST_WAVES
#define PT_FAST_WAVES 8       // waves per SIMD the specialised k_bounce variants are compiled for (<= 64 registers; 8 workgroups'
                              // LDS is also what a CU holds with the Cornell tables since the record buffer lost a row and the window half its runs)
#endif
#ifndef PT_FAST_WAVES_FIRST
#define PT_FAST_WAVES_FIRST (PT_FAST_WAVES - 1)      // the specialised camera-ray variant: 64-66 registers.  (Compiled for 8 waves it fits 64 with two
                                    // values spilled to scratch: the kernel alone +3 %, the wall with three launch sets in flight -0.8 %, three runs
                                    // each on one box -- not taken: no kernel of the path spills, tests/test_build_resources.py)
#endif
#ifndef PT_FAST_WAVES_SPLIT
#define PT_FAST_WAVES_SPLIT 4 // same for the specialised MODE 1 variant, which carries the mesh candidate queue as well
#endif
#ifndef PT_FAST_WAVES_SPLIT2
#define PT_FAST_WAVES_SPLIT2 5 // and for MODE 2 (fits 6-7 as it is; a tighter bound measured 1-2 % slower on C5)
#endif
#ifndef PT_BOUNCE_WAVES
#define PT_BOUNCE_WAVES 4     // waves per SIMD k_bounce is compiled for (register budget 512 / this)
#endif
constexpr int TILE = PT_TILE;      // paths per tile = threads per workgroup (PT_TILE / 64 waves)
constexpr int WAVES = TILE / 64;
// a path's rank inside its tile takes RANK_BITS; the stage key packs bin | rank among all << BIN_BITS | rank among the stored << (BIN_BITS + RANK_BITS)
constexpr int RANK_BITS = TILE <= 256 ? 8 : 9, BIN_BITS = 32 - 2 * RANK_BITS;
static_assert(TILE <= 512 && (TILE & (TILE - 1)) == 0, "tile size: a power of two up to 512 (9-bit ranks)");
// words of per-tile LDS in front of the 16-byte aligned record buffer: ranking histogram, running prefix, tile counts/offsets,
// tileIntersect's 2 x 4 list counters
// + the window over the input's run tables (locate): 65 start positions, 65 stream-index bases, 64 local-index bases, next run
#ifndef PT_WIN
#define PT_WIN 32
#endif
constexpr int WIN = PT_WIN, WIN_WORDS = 2 * (WIN + 1) + WIN + 2;      // (a power of two <= 64: one wave loads a window; 32 since round 4 -- with the
                                                                 // record rows below what lets EIGHT workgroups' LDS fit a CU for the Cornell tables)
constexpr int ldsHeadWords(int nb) { return ((2 * WAVES * nb + 4 * nb + 1 + 8 + WIN_WORDS) + 3) & ~3; }
// k_bounce's dynamic LDS, in words: [scene tables][head][17 x TILE records].  The record buffer doubles as tileIntersect's
// scratch, whose 64-bit minimum keys (best[], at word 6*TILE of it) are the target of ds_min_u64: a 4-byte-misaligned
// 64-bit LDS atomic is a memory aperture violation (that is the fault of round 1's first benchmark run: a head of
// 2*WAVES*nb + 4*nb + 1 words put the records on an odd word, group_seg_size 20596 B = 5149 words).  Hence every part is a
// multiple of 4 words, the layout has this one definition for host and device, and the asserts below pin it.
constexpr int REC_WORDS = 17 * TILE;
// (the specialised fused kernel carries no texcoords: its pixel / material / key rows move up over one of their two, 16 rows -- what
// tileIntersect's scratch with the parked state needs anyway)
#ifndef PT_REC_ROWS_FAST0
#define PT_REC_ROWS_FAST0 16
#endif
constexpr int REC_ROWS_FAST0 = PT_REC_ROWS_FAST0;
static_assert(WIN <= 64 && (WIN & (WIN - 1)) == 0, "window of runs: one wave, binary search");
__host__ __device__ constexpr size_t bounceLdsWords(int tableWords, int nb) { return (size_t)tableWords + (size_t)ldsHeadWords(nb) + REC_WORDS; }
static_assert(ldsHeadWords(1) % 4 == 0 && ldsHeadWords(2) % 4 == 0 && ldsHeadWords(3) % 4 == 0 && ldsHeadWords(7) % 4 == 0 &&
              ldsHeadWords(45) % 4 == 0 && ldsHeadWords(65535) % 4 == 0, "record buffer must start 16-byte aligned");
static_assert(sceneTableWords(1, 1, 1) % 4 == 0 && sceneTableWords(12, 7, 7) % 4 == 0 && sceneTableWords(0, 3, 5) % 4 == 0, "scene tables end 16-byte aligned");
static_assert((6 * TILE) % 2 == 0 && (8 * TILE) % 2 == 0, "tileIntersect's 64-bit keys and lists must be 8-byte aligned inside the record buffer");

#ifndef PT_QCAP
#define PT_QCAP (4 * TILE)
#endif
#ifndef PT_DIRECT_STORE
#define PT_DIRECT_STORE 1      // round 5: a tile's stored paths go from registers to their stage slots (no transposition through LDS), every wave
                               // derives the tile's in-tile offsets itself, keys are written for stored slots only: three barriers per tile instead of six
#endif
#ifndef PT_RANK_SLICED
#define PT_RANK_SLICED 1       // later bounces, <= 16 bins: the in-wave ranking bit-sliced instead of one pass per bin that occurs
#endif
constexpr int QCAP = PT_QCAP;                        // LDS queue entries of MODE 1, behind the record buffer, + its two counters
constexpr int QUEUE_WORDS = QCAP + 4;

// k_mesh (pt_kernels.hip)
#ifndef PT_MESHQ_CHUNK      // (not PT_MESH_CHUNK: that is pt_device.h's faces-per-lane of the small meshes -- the first build of this kernel
                           // took ITS value, 4, for the chunk: one global atomic per four rays, 8x slower, results right)
#define PT_MESHQ_CHUNK 128    // queue entries a wave reserves per global atomic (64: +1 %, 32: +30 % -- the cursor is one address per segment)
#endif
#ifndef PT_MESH_REFILL
#define PT_MESH_REFILL 16     // lanes without a walk that trigger a turnover
#endif
#ifndef PT_MESH_NMIN
#define PT_MESH_NMIN 32       // lanes holding an inner node that make the next round a node round
#endif
#ifndef PT_MESH_WG_PER_CU
#define PT_MESH_WG_PER_CU 3    // workgroups per CU of k_mesh's grid (see enqueue_batch)
#endif
constexpr int MESH_GEOM_WORDS = 20;      // per geom in k_mesh's LDS: inverseTransform rows 0-2 (12), root box lo / hi (6), wide root (-1: not searched here), pad

// SoA stream.  "stream" buffers hold paths waiting to be shaded (sorted); "stage" buffers hold the output of
// k_bounce in tile order; the sort exists only as the chunk-local index in their lsrc / lidx arrays plus the run tables.
struct PathSoA {
    // A stored path lies in up to FOUR arrays of 16-byte quads per slot: A = (shading point xyz, pixel slot) and B = (throughput colour rgb,
    // materialId | geomId << 16), which every record has; C = (normal xyz, texcoord u) unless the record's bin is in ntab_bins; D = (incoming
    // direction xyz, texcoord v) if its bin is in dir_bins.  One 16-byte load or store per part, and a run of a tile's records of one bin
    // is 16 B per record and array, not 4: the run's first and last cache lines, which the neighbouring bins' readers fetch as well, are
    // a fifth of what it reads instead of half (round 4: the wall time follows the HBM bytes).  The ints lie at i + k * stride (stride =
    // segments x capacity; a segment's part of an array starts seg * capacity slots further).  Kept as bases + stride rather than a pointer
    // per field: a kernel that holds two of these in scalar registers for its whole tile loop has none left for anything else.
    float *q;          // [4][stride] quads
    int32_t *i;        // [3][stride]: idx, lsrc, lidx -- or, where the local index is bin-major (BounceParams::loop_idx), that index and nothing else
    uint32_t stride;
    struct F4 { float *b; __host__ __device__ float &operator[](size_t s) const { return b[s * 4]; } };      // one component of a quad array
    struct I4 { int32_t *b; __host__ __device__ int32_t &operator[](size_t s) const { return b[s * 4]; } };
    __host__ __device__ float *quadA() const { return q; }                              // px py pz pix
    __host__ __device__ float *quadB() const { return q + 4 * (size_t)stride; }         // cr cg cb mg
    __host__ __device__ float *quadC() const { return q + 8 * (size_t)stride; }         // nx ny nz u
    __host__ __device__ float *quadD() const { return q + 12 * (size_t)stride; }        // dx dy dz v
    __host__ __device__ F4 px() const { return {q}; }              // shading point = origin + t * direction (src/pathtrace.cu:392)
    __host__ __device__ F4 py() const { return {q + 1}; }
    __host__ __device__ F4 pz() const { return {q + 2}; }
    __host__ __device__ I4 pix() const { return {reinterpret_cast<int32_t *>(q) + 3}; }                          // slot among the owned pixels
    __host__ __device__ F4 cr() const { return {quadB()}; }        // throughput colour
    __host__ __device__ F4 cg() const { return {quadB() + 1}; }
    __host__ __device__ F4 cb() const { return {quadB() + 2}; }
    __host__ __device__ I4 mg() const { return {reinterpret_cast<int32_t *>(quadB()) + 3}; }                     // materialId | geomId << 16
    __host__ __device__ F4 nx() const { return {quadC()}; }        // pending intersection: normal, texcoords (u, v only if textured)
    __host__ __device__ F4 ny() const { return {quadC() + 1}; }
    __host__ __device__ F4 nz() const { return {quadC() + 2}; }
    __host__ __device__ F4 u() const { return {quadC() + 3}; }
    __host__ __device__ F4 dx() const { return {quadD()}; }        // incoming direction
    __host__ __device__ F4 dy() const { return {quadD() + 1}; }
    __host__ __device__ F4 dz() const { return {quadD() + 2}; }
    __host__ __device__ F4 v() const { return {quadD() + 3}; }
    // logical field k of slot j, in the order the debug capture hands them out: point, direction, colour, normal, u, v
    __host__ __device__ float fieldAt(int k, size_t j) const {
        if (k < 3) return q[j * 4 + k];
        if (k < 6) return quadD()[j * 4 + (k - 3)];
        if (k < 9) return quadB()[j * 4 + (k - 6)];
        if (k < 12) return quadC()[j * 4 + (k - 9)];
        return k == 12 ? quadC()[j * 4 + 3] : quadD()[j * 4 + 3];
    }
    __host__ __device__ int32_t *idx() const { return i; }     // stage key (see stage_key) or -1
    // the chunk-local sorted index a workgroup leaves in its tail (see "local move" in k_bounce): entry e of the chunk's region is
    // the stage slot of the path that comes e-th in (bin, tile, rank) order inside the chunk, and its rank among ALL survivors of
    // its bin inside the chunk (the part of the RNG stream index the workgroup can know by itself)
    __host__ __device__ int32_t *lsrc() const { return i + (size_t)stride; }
    __host__ __device__ int32_t *lidx() const { return i + 2 * (size_t)stride; }
};
constexpr int SOA_FLOATS = 16, SOA_INTS = 3, SOA_LOGICAL_FLOATS = 14;      // words per slot in the float / int buffers; fields the capture hands out


__device__ __forceinline__ PathSoA soa_offset(PathSoA s, size_t off) {
    s.q += 4 * off; s.i += off;
    return s;
}
// The same stream, but with a stride the optimiser cannot see through: field addresses derived from the result are
// computed where they are used (a few scalar adds per tile) instead of being hoisted out of the tile loop and kept --
// 34 scalar registers per stream -- for its whole length.
// Uniform base + per-lane 32-bit byte offset: the form the hardware addresses by itself (global_load_dword v, voffset,
// s[base:base+1]).  Written as base[index] the compiler forms a 64-bit address per access in vector registers (one
// v_lshl_add_u64 and a register pair each); this way a record's 15 fields share one offset register and the per-field
// bases are scalar adds.  The base must be wave-uniform and the offset below 4 GiB (a segment's field is capacity x 4 B).
#ifndef PT_SCALAR_BASE
#define PT_SCALAR_BASE 1
#endif
template <class T> using gptr = T __attribute__((address_space(1))) *;
template <class T> __device__ __forceinline__ T ld_u(const T *base, uint32_t byteoff) {
#if PT_SCALAR_BASE
    gptr<const T> b = (gptr<const T>)base;
    asm volatile("" : "+s"(b));
    return *reinterpret_cast<gptr<const T>>(reinterpret_cast<gptr<const char>>(b) + byteoff);
#else
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byteoff);
#endif
}
template <class T> __device__ __forceinline__ void st_u(T *base, uint32_t byteoff, T v) {
#if PT_SCALAR_BASE
    gptr<T> b = (gptr<T>)base;
    asm volatile("" : "+s"(b));
    *reinterpret_cast<gptr<T>>(reinterpret_cast<gptr<char>>(b) + byteoff) = v;
#else
    *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byteoff) = v;
#endif
}

__device__ __forceinline__ PathSoA soa_fresh(PathSoA s) {
    asm volatile("" : "+s"(s.stride));
    return s;
}

struct TileMap {           // which pixels this device owns (row blocks round-robin over tile_world)
    int32_t W, H, tile_rows, tile_rank, tile_world, owned;
    uint32_t w_mul, w_sh, rows_mul, rows_sh;     // n / W and n / tile_rows as multiply-high + shift (fastdiv), set by the host
};

// n / d for 0 <= n < 2^31 and a divisor fixed at create: q = (n * mul) >> (32 + sh) with mul = floor(2^(32+sh) / d) + 1,
// sh = ceil(log2 d) - 1 (exact for that range: the classic invariant-divisor multiply); sh = 255 marks d == 1.
// Keeps the compiler's generic division -- a dozen instructions and a loop-invariant reciprocal that it spills -- out of
// the tile loop.
__device__ __forceinline__ int fastdiv(int n, uint32_t mul, uint32_t sh) {
    return sh == 255u ? n : (int)(__umulhi((uint32_t)n, mul) >> sh);
}

__device__ __forceinline__ void owned_pixel(const TileMap &tm, int i, int &x, int &y) {
    int r = fastdiv(i, tm.w_mul, tm.w_sh);
    x = i - r * tm.W;
    if (tm.tile_world <= 1) { y = r; return; }
    int k = fastdiv(r, tm.rows_mul, tm.rows_sh);
    y = (k * tm.tile_world + tm.tile_rank) * tm.tile_rows + (r - k * tm.tile_rows);
}

// global pixel index (x + y*W) of the `slot`-th pixel this device owns.  Paths carry the SLOT, not the pixel: with a
// row-tile split the per-iteration radiance buffers, like the streams, are then sized and indexed by what the device
// owns (1/8 of the frame on one of eight ranks), and with one device slot == pixel.
__device__ __forceinline__ int slot_to_pixel(const TileMap &tm, int slot) {
    if (tm.tile_world <= 1) return slot;
    int x, y;
    owned_pixel(tm, slot, x, y);
    return x + y * tm.W;
}

struct BounceParams {
    DScene sc;
    DCamera cam;
    TileMap tm;
    PathSoA in, stage;                     // in = the stage the previous bounce wrote (tile order) with its chunk-local sorted index
    // the run tables of the launch that wrote `in` (its grid had in_gx workgroups per segment; run r = bin * in_gx + workgroup):
    const int32_t *in_totals;              // [2][nbins]: survivors / stored paths per bin (n_in = sum of the stored ones)
    const int32_t *in_super;               // [2][nbins][nsuper]: the same per 64 consecutive workgroups
    const int32_t *in_chunk;               // [3][chunk_cap]: per run -- survivors, stored paths, start of the run in the local index
    int32_t in_gx;
    int32_t last_inplace;                  // the light-only last bounce tests each tile's rays where they are, no pool over tiles (in the
                                           // padding behind in_gx: no other member moves; PTX_DEBUG_LAST_INPLACE: A/B, tests of both)
    size_t seg_in_totals, seg_in_chunk;    // per-segment strides of those (0: the cached bounce 0, shared by all segments)
    float *image;
    int32_t iter, traceDepth, bounce;      // bounce = index b of the intersect stage done by this launch
    int32_t iter_stride;                   // iteration of segment s = iter + s * iter_stride (1; world size when ranks take turns)
    // split mesh search (MODE 1 / 2 of k_bounce, k_mesh in between): per-ray keys, the queue of parked rays (their stage slots)
    unsigned long long *keys; uint32_t *items; int32_t *item_count;
    int32_t *item_cursor;                  // one int per segment, after the counts: where k_mesh's waves draw their next chunk of the queue
    size_t seg_keys, seg_items;            // per-segment strides of keys / items; item_count has one int per segment
    const uint32_t *tile_geoms;            // first bounce: [tile] bit g = some pixel of the tile may see geom g (NULL: no information)
    int32_t *tile_done;                    // split first bounce: [segment][tile] 1 = pass 1 finished the tile (no ray of it reaches a mesh's box)
    int32_t aa, dof, sort;
    int32_t uses_uv;                       // some OBJ geom has a texture: texcoords are carried, otherwise not
    unsigned long long dir_bins;           // bit b: the records of material bin b carry the incoming direction (reflective, refractive, or a
                                           // material of an OBJ geom: what scatterRay reads it for); the other bins' records do not
    unsigned long long in_dir_bins, in_ntab_bins;      // dir_bins / ntab_bins of the launch that wrote `in` (the same, unless `in` is the cached camera bounce)
    // The local index as ONE word per stored path (round 5), where a workgroup's chunk of the writing launch is at most 128 tiles (32 768
    // slots; the host knows the bound: ceil(maxTiles / workgroups)): entry e = (slot - e) as 16 signed bits | the path's rank in its run
    // << 16 -- slot and entry lie in the same chunk's region, so their distance fits, and so does a rank below the chunk's slots.  Half
    // the index bytes: 4 B less read per ray, 4 B less written per stored path.  Larger chunks (8K frames with few iterations per set)
    // keep the two words, lsrc and lidx.  idx16: what THIS launch's tail writes; in_idx16: what the launch that wrote `in` did.
    int32_t idx16, in_idx16;
    unsigned long long ntab_bins;          // bit b: every hit of material bin b is a cube hit (no sphere or OBJ geom has the material): its records
                                           // carry the 3-bit code of the cube's tabulated normal in pix's bits 28-30 instead of the normal
    int32_t apps;                          // apps/src variant: radiance * PI at gather, albedo AOV on iteration 1
    // The local index written INSIDE the tile loop (pt_plan.h, IndexPlan; in the padding behind apps: no other member moves).  Bin-major:
    // a segment's index is [nbins][N2] entries, N2 = the stage's slots rounded up to a power of two, and the entry of a stored path is
    // bin * N2 + S + q -- S the first slot of the writing workgroup's chunk, q the bin's stored paths in the chunk's earlier tiles + the
    // path's rank among the tile's -- all of which a lane of the direct epilogue holds.  The word(s) are today's: (slot - (S + q)) as 16
    // signed bits | rank << 16, or slot and rank in two words (the second [nbins][N2] behind the first).  A run starts at bin * N2 + S,
    // known at kernel start; the reader's position inside the chunk is (entry & (N2 - 1)).  In this form stage.i / in.i point at the
    // index of the launch's first segment (segments nbins * N2 * words apart), and the stage key, the per-tile prefix tables and the
    // tail's pass over the keys do not exist.  Bit 0: THIS launch writes the form; bit 1: the launch that wrote `in` did; bit 2: two
    // words per entry are allocated (some launch set of the tracer keeps the two-word form); bits 8-15: log2 N2.
    int32_t loop_idx;
    float *albedo;
    int32_t nbins, maxTiles;
    int32_t *counts_all, *counts_scat;     // [nbins][maxTiles]: prefix of the tile inside its workgroup's chunk
    int32_t *chunk;                        // out, [3][chunk_cap], run r = bin * gridDim.x + workgroup: survivors and stored paths of
                                           // that workgroup's chunk of tiles in that bin, and where the run starts in the local index
    int32_t chunk_cap;                     // nbins x (workgroups per segment at most)
    int32_t *super_all, *super_scat;       // [nbins][nsuper]:   totals per 64 consecutive workgroups (atomics)
    int32_t *totals_all, *totals_scat;     // [nbins] of this bounce (atomics)
    int32_t nsuper;
    // batching: blockIdx.y = segment = one iteration of the batch (iteration p.iter + segment), each an independent
    // stream with its own buffers at these strides (in elements)
    size_t seg_in, seg_stage, seg_counts, seg_chunk, seg_totals, seg_part;
    unsigned long long *stamps;            // diagnostic build (-DPT_STAMPS) only: cycles per phase, summed over waves
    float *part;                           // != NULL: every ending path STORES its radiance to part[segment][pix]
                                           // (k_gather adds the segments to the image in iteration order)
    // first-bounce cache fill (iter 1, AA and DoF off): bounce-0 light hits are replayed on later iterations
    int32_t *emit_count; int32_t *emit_pix; float *emit_rgb;
    // Fences that report.  Every index the kernels take from a table another launch wrote -- a queue entry of the split mesh search,
    // a parked ray's owner, an entry of the local index, a sorted position's place in it -- is checked against `fence_slots` (the
    // stage's capacity, maxTiles x TILE) before it becomes an address: a bad one is skipped or clamped, so it costs a wrong pixel and
    // not a fault, and is COUNTED here (ptx_stats.fenced, 0 in every test): a wrong pixel is never the only symptom.
    unsigned long long *fenced;
    uint32_t fence_slots;
    uint32_t fence_slots_cap;              // maxTiles x TILE itself (fence_slots is that too, unless a test lowered it): where a segment's lit flags start
};

// A path that ends adds its radiance to its pixel (finalGather, src/pathtrace.cu:407-416).  Each pixel ends exactly
// once per iteration, so this is a plain read-modify-write, or -- when several iterations are in flight as
// segments of one launch -- a plain store into that iteration's buffer.
// three floats stored by one instruction (global_store_dwordx3 with a scalar base); the address is only 4-byte aligned
typedef float Rgb __attribute__((ext_vector_type(3)));
typedef Rgb RgbUnaligned __attribute__((aligned(4)));
__device__ __forceinline__ void st_rgb(float *base, uint32_t byteoff, float r, float g, float b) {
    const Rgb v = {r, g, b};
#if PT_SCALAR_BASE
    gptr<float> sb = (gptr<float>)base;
    asm volatile("" : "+s"(sb));
    *reinterpret_cast<RgbUnaligned __attribute__((address_space(1))) *>(reinterpret_cast<gptr<char>>(sb) + byteoff) = v;
#else
    *reinterpret_cast<RgbUnaligned *>(reinterpret_cast<char *>(base) + byteoff) = v;
#endif
}
// Batched mode, round 5: only paths that end WITH radiance (a light hit, an emissive texel) write their 12 bytes, and set the slot's bit
// in the segment's "lit" plane, which lies behind the segment's radiance ([cap] floats x 3, then [cap / 32] words, bit s & 31 of word s / 32
// for slot s).  The many that end black -- misses, the last bounce: most path ends of a Cornell frame -- write nothing, and k_gather adds only
// flagged slots: adding the +0 they used to store changes no sum (the image holds no -0: it starts at +0 and only grows), so the frames
// are the same bits.  C4 moved 12 B per path end and 12 B per pixel and iteration in k_gather for those zeros: 11 % of its HBM bytes.
// The planes are zero whenever no launch set is in flight: k_gather clears the words it reads (a full clear before a lane's next set
// where that does not hold: ptx_tracer::aux_dirty).  32 slots share a word, so a bit is set with an atomic.
__device__ __forceinline__ uint32_t *lit_flags(float *part, uint32_t cap) { return reinterpret_cast<uint32_t *>(part + 3 * (size_t)cap); }
__device__ __forceinline__ void set_lit(float *part, uint32_t cap, uint32_t slot) { atomicOr(lit_flags(part, cap) + (slot >> 5), 1u << (slot & 31u)); }
__device__ __forceinline__ void deposit(const TileMap &tm, float *image, float *part, bool batched, int pix, vec3 c, int apps, uint32_t cap) {
    if (apps) c = scale(c, 3.14159265358f);            // apps/src/pathtrace.cu:44,508: image += color * PI
    if (batched) {
        st_rgb(part, (uint32_t)pix * 12u, c.x, c.y, c.z);
        set_lit(part, cap, (uint32_t)pix);
    } else {
        float *px = image + (size_t)slot_to_pixel(tm, pix) * 3;
        px[0] += c.x; px[1] += c.y; px[2] += c.z;
    }
}

// Albedo AOV of the apps/src copy (apps/src/pathtrace.cu:412-462): what the first hit of iteration 1 looks like.
__device__ __forceinline__ void write_albedo(const DScene &sc, const Hit &hit, float *dst) {
    vec3 a = V3(0.f, 0.f, 0.f);
    if (hit.t > 0.0f) {
        const DMaterial m = getMaterial(sc, hit.mat);
        const DGeom &geom = sc.geoms[hit.geom];
        a = V3(m.color[0], m.color[1], m.color[2]);
        if (geom.type == G_OBJ) {
            const DTex &kd = geom.tex[0], &ke = geom.tex[2];
            vec3 emission = V3(0.f, 0.f, 0.f);
            if (ke.ch) {
                int pixelID = (int)(hit.v * ke.h) * ke.w + (int)(hit.u * ke.w);
                emission = V3(texel(sc, ke, pixelID, 0) / 255.f, texel(sc, ke, pixelID, 1) / 255.f, texel(sc, ke, pixelID, 2) / 255.f);
            }
            const float eps = 1.1920928955078125e-07f;
            if (emission.x > eps || emission.y > eps || emission.z > eps) a = scale(emission, 5.0f);
            else if (kd.ch) {
                int pixelID = (int)(hit.v * kd.h) * kd.w + (int)(hit.u * kd.w);
                a = V3(texel(sc, kd, pixelID, 0) / 255.f, texel(sc, kd, pixelID, 1) / 255.f, texel(sc, kd, pixelID, 2) / 255.f);
            }
        } else if (m.emittance > 0.0f) a = scale(a, m.emittance);
        else if (m.hasRefractive > 0.0f) a = V3(m.speccolor[0], m.speccolor[1], m.speccolor[2]);
    }
    dst[0] = a.x; dst[1] = a.y; dst[2] = a.z;
}

// number of set bits of a wave ballot below this lane
__device__ __forceinline__ int wavePrefix(unsigned long long b, int lane) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// the per-stage test kernels' records (k_kat_*, pt_kernels.hip): the reference's AoS PathSegment / ShadeableIntersection
struct HostPath { float o[3], d[3], c[3]; int32_t pixelIndex, remainingBounces; };       // 44 B
struct HostIsect { float t, n[3]; int32_t materialId; float uv[2]; int32_t geomId; };    // 32 B

// ---- the arithmetic-bearing kernels of one pt_kernels.hip code object as a table of launchers -------------------------------------
// pt_kernels.hip is compiled once per arithmetic level (pt_device.h: PT_ARITH), each a code object of its own that exports its table
// as ptx_arith_kernels_<level>().  Only pt_engine.hip holds the host side; it launches through the table of the level the tracer was
// created with (ptx_options.arith).  Plain types in the signatures (the parameter blocks travel as const void *): the structs are
// the same source in every translation unit but, formally, types of different anonymous namespaces.
struct KernelSet {
    int arith;
    void (*bounce)(int first, int mode, int fast, dim3 grid, size_t lds, hipStream_t st, const void *bounce_params);
    void (*mesh)(int first, dim3 grid, size_t lds, hipStream_t st, const void *bounce_params, int bvh_stack);
    void (*finish)(int first, dim3 grid, hipStream_t st, const void *bounce_params);
    void (*kat_geom)(dim3 grid, hipStream_t st, const void *scene, int gi, int n, const float *rays, float *out);
    void (*kat_intersect)(dim3 grid, hipStream_t st, const void *scene, int n, const void *paths, void *out);
    void (*kat_obj_tri)(dim3 grid, hipStream_t st, const void *scene, int gi, int n, const float *rays, float *out);
    void (*kat_jittered)(dim3 grid, hipStream_t st, int n, const float *normals, const int32_t *seeds, int max_iter, float *out);
    void (*kat_tile)(int split, dim3 grid, size_t lds, hipStream_t st, const void *sc, const void *scg, int n, const void *paths, void *out, int uses_uv);
    void (*kat_shade)(dim3 grid, hipStream_t st, const void *scene, int iter, int n, const int32_t *idx, const void *isects, void *paths);
    void (*kat_generate)(dim3 grid, hipStream_t st, const void *cam, int iter, int traceDepth, int aa, int dof, void *paths);
    void (*kat_libm)(dim3 grid, hipStream_t st, int n, const float *x, float *s, float *c, const double *pw, double *p5, const float *pxy, float *pout);
    int (*bounce_occupancy)(size_t lds);      // ptx_debug_bounce_occupancy: workgroups of the specialised later-bounce kernel per CU (< 0: error)
};
// The light-only last bounce, k_bounce<false, 3, .> -- the unsplit later bounce of a path's LAST intersection (bounce traceDepth - 1) -- is a
// code object of its own per level (pt_kernels_last.hip), exported as ptx_arith_last_<level>(); lds = what `bounce` is given for the same
// launch (last_violation, pt_engine.hip, says when it may be taken).
struct LastKernelSet {
    int arith;
    void (*bounce_last)(int fast, dim3 grid, size_t lds, hipStream_t st, const void *bounce_params);
};

}  // namespace
