// pt_compaction.hip -- scan / stream compaction on int arrays behind include/mi355x_stream_compaction.h.
//
// Replaces the reference's stream_compaction/{cpu,naive,efficient,thrust,common}.cu.  The reference's GPU scans
// issue one launch per tree level (2*log2(n)+1 launches for the Blelloch version, efficient.cu:46-61) and its
// compaction is map + scan + scatter over three int arrays (efficient.cu:79-136).  Here either is ONE pass over the
// data -- a chained scan with decoupled look-back, written for 64-wide wavefronts:
//   * a workgroup (512 threads for the scan, 1024 for compaction) takes the next 16384-element tile (ticket from an
//     atomic counter, so a tile's predecessors are always resident or done), loaded as coalesced non-temporal
//     16-byte loads, 8 or 4 per lane;
//   * scan inside the tile: 4 per lane per load in registers, wave scan in DPP (round 5; __shfl_up before), the 64 (load, wave) totals
//     scanned by wave 0 through LDS;
//   * the tile publishes {flag, total} as one 8-byte word (relaxed agent-scope store: one granule, no fence needed,
//     visible across the XCDs' L2s) and its wave 0 looks back over its predecessors' words, 64 per step, adding
//     tile totals until it meets one that already knows its inclusive prefix, then publishes its own;
//   * scan: the prefixes are stored; compaction (kernMapToBoolean fused, common.cu:25-34): the survivors of the
//     tile are packed in LDS and stored as one contiguous run (kernScatter, common.cu:40-49, without the index array).
// HBM traffic is the algorithmic minimum: scan 4 B read + 4 B written per element, compaction 4 B read + 4 B per
// survivor, plus 8 B per tile of status words (zeroed by a memset node in front of the kernel).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <string>
#include <string.h>

#include "../../include/mi355x_pathtracer.h"
#include "../../include/mi355x_stream_compaction.h"
#include "pt_handle.h"

namespace {

constexpr int SC_TILE = 16384;                                 // elements (64 KB) per workgroup: one ticket each, and one
                                                               // address takes only ~80 M atomics/s across the XCDs
// 64 (round, wave) totals per tile either way (one lane each in the second-level scan); measured on 2^28 ints:
// scan 1024 x 4: 4.39 TB/s, 512 x 8: 4.57 TB/s; compaction 1024 x 4: 3.75 TB/s, 512 x 8: 3.60 TB/s (copy: 4.9-5.0);
// at least 4 waves per SIMD (<= 128 registers): asking for 8 spills and is 5 % slower
constexpr int SC_SCAN_THREADS = 512, SC_COMPACT_THREADS = 1024;
constexpr int SC_HEAD = 64;                                    // workspace: [ticket, padding to 64 B][status word per tile]

typedef unsigned long long u64;
typedef int v4i __attribute__((ext_vector_type(4)));
constexpr u64 ST_AGGREGATE = 1ull << 32;                       // low word = this tile's total
constexpr u64 ST_INCLUSIVE = 2ull << 32;                       // low word = total of this tile and everything before it

thread_local float g_gpu_ms = 0.f, g_cpu_ms = 0.f;

// inclusive prefix sum over the lanes of a wave in the vector ALU's own lane network (DPP), as pt_kernels.hip's waveInclusiveScan: four
// shifted adds inside the rows of 16 lanes, lane 15 of a row broadcast into the next row (rows 1 and 3), lane 31 into the upper half.
// Six dependent vector instructions where __shfl_up made six ds_bpermute round trips through the LDS crossbar (rounds 1-4) -- at frame
// sizes (2 M elements) the kernel is a chain of such latencies, not a stream.
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
    (void)lane;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);      // row_shr:1 (lanes without a source add 0)
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);      // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);      // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);      // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
    return v;
}

// sum over the wave, in every lane: the scan's last lane through the scalar path (v_readlane), no LDS round trip
__device__ __forceinline__ int wave_sum(int v) { return __builtin_amdgcn_readlane(wave_inclusive_scan(v, 0), 63); }

// kernMapToBoolean (common.cu:25-34): bools[i] = idata[i] != 0.  The first n4 quads go as 16-byte accesses (both arrays 16-byte
// aligned), the rest one by one; HBM-bound, 8 B per element.
__global__ __launch_bounds__(256) void k_map_to_boolean(int n, int n4, int *__restrict__ bools, const int *__restrict__ idata) {
    const int stride = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
    for (int q = t0; q < n4; q += stride) {
        const v4i a = reinterpret_cast<const v4i *>(idata)[q];
        v4i b;
        b.x = a.x != 0; b.y = a.y != 0; b.z = a.z != 0; b.w = a.w != 0;
        reinterpret_cast<v4i *>(bools)[q] = b;
    }
    for (int i = 4 * n4 + t0; i < n; i += stride) bools[i] = idata[i] != 0 ? 1 : 0;
}
// kernScatter (common.cu:40-49): bools[i] == 1 => odata[indices[i]] = idata[i]
__global__ __launch_bounds__(256) void k_scatter(int n, int *__restrict__ odata, const int *__restrict__ idata, const int *__restrict__ bools,
                                                  const int *__restrict__ indices) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (bools[i] == 1) odata[indices[i]] = idata[i];
}

// COMPACT = false: out[i] = in[0] + .. + in[i-1].  COMPACT = true: out = the non-zero elements of in, in order;
// *count = how many.  A tile waits only for tiles with lower tickets, which are resident or done and post their totals
// before they wait for anything themselves: every wait ends.
template <bool COMPACT, int SC_THREADS>
__global__ __launch_bounds__(SC_THREADS, 4) void k_onepass(int n, const int *__restrict__ in, int *__restrict__ out,
                                                            unsigned *__restrict__ ticket, u64 *__restrict__ status,
                                                            int *__restrict__ count) {
    constexpr int SC_WAVES = SC_THREADS / 64, SC_ROUNDS = SC_TILE / (SC_THREADS * 4);       // 16-byte loads per lane
    __shared__ int s_tile, s_excl, s_total;
    __shared__ int s_wtot[SC_ROUNDS * SC_WAVES];              // (round, wave) totals, then their exclusive prefixes
    __shared__ int s_stage[COMPACT ? SC_TILE : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_tile = (int)atomicAdd(ticket, 1u);
    __syncthreads();
    const int tile = s_tile;
    const long long tbase = (long long)tile * SC_TILE;
    const bool whole = tbase + SC_TILE <= n;

    int x[SC_ROUNDS][4];
    if (whole && (((uintptr_t)in) & 15) == 0) {
#pragma unroll
        for (int r = 0; r < SC_ROUNDS; r++) {
            // streamed once: non-temporal loads and stores (+5 % on 1 GiB)
            const v4i a = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(in + tbase + (r * SC_THREADS + tid) * 4));
            x[r][0] = a.x; x[r][1] = a.y; x[r][2] = a.z; x[r][3] = a.w;
        }
    } else {
#pragma unroll
        for (int r = 0; r < SC_ROUNDS; r++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const long long i = tbase + (r * SC_THREADS + tid) * 4 + k;
                x[r][k] = i < n ? in[i] : 0;
            }
    }
    // what is summed: the value, or 1 per survivor
    int sum[SC_ROUNDS], incl[SC_ROUNDS];
#pragma unroll
    for (int r = 0; r < SC_ROUNDS; r++) {
        sum[r] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) sum[r] += COMPACT ? (x[r][k] != 0 ? 1 : 0) : x[r][k];
        incl[r] = wave_inclusive_scan(sum[r], lane);
        if (lane == 63) s_wtot[r * SC_WAVES + wave] = incl[r];
    }
    __syncthreads();

    if (wave == 0) {
        // the 64 (round, wave) totals are one wave's worth: scan them, then look back for what precedes the tile
        static_assert(SC_ROUNDS * SC_WAVES == 64, "one lane per (round, wave) total");
        const int t = s_wtot[lane];
        const int ti = wave_inclusive_scan(t, lane);
        s_wtot[lane] = ti - t;
        const int total = __builtin_amdgcn_readlane(ti, 63);
        int excl = 0;
        if (tile == 0) {
            if (lane == 0) __hip_atomic_store(&status[0], ST_INCLUSIVE | (unsigned)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0) __hip_atomic_store(&status[tile], ST_AGGREGATE | (unsigned)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // lane l looks at tile j - l; every predecessor holds a ticket, so its word is only a matter of time
            for (int j = tile - 1;; j -= 64) {
                const int idx = j - lane;
                int first, part;
                for (;;) {
                    const u64 st = idx >= 0 ? __hip_atomic_load(&status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ST_INCLUSIVE;
                    const u64 inclusive = __ballot((st >> 32) == 2);
                    const u64 pending = __ballot((st >> 32) == 0);
                    first = inclusive ? __builtin_ctzll(inclusive) : 64;
                    const u64 needed = first >= 63 ? ~0ull : ((2ull << first) - 1);       // lanes 0 .. first
                    if ((pending & needed) == 0) { part = lane <= first ? (int)(unsigned)st : 0; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                excl += wave_sum(part);
                if (first < 64) break;
            }
            if (lane == 0) __hip_atomic_store(&status[tile], ST_INCLUSIVE | (unsigned)(excl + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) { s_excl = excl; s_total = total; }
    }
    __syncthreads();
    const int excl = s_excl;
    int off[SC_ROUNDS];
#pragma unroll
    for (int r = 0; r < SC_ROUNDS; r++) off[r] = s_wtot[r * SC_WAVES + wave] + incl[r] - sum[r];

    if (!COMPACT) {
        if (whole && (((uintptr_t)out) & 15) == 0) {
#pragma unroll
            for (int r = 0; r < SC_ROUNDS; r++) {
                int4 o;
                o.x = excl + off[r]; o.y = o.x + x[r][0]; o.z = o.y + x[r][1]; o.w = o.z + x[r][2];
                __builtin_nontemporal_store(v4i{o.x, o.y, o.z, o.w}, reinterpret_cast<v4i *>(out + tbase + (r * SC_THREADS + tid) * 4));
            }
        } else {
#pragma unroll
            for (int r = 0; r < SC_ROUNDS; r++) {
                int run = excl + off[r];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const long long i = tbase + (r * SC_THREADS + tid) * 4 + k;
                    if (i < n) out[i] = run;
                    run += x[r][k];
                }
            }
        }
    } else {
        const int total = s_total;
#pragma unroll
        for (int r = 0; r < SC_ROUNDS; r++) {
            int rank = off[r];
#pragma unroll
            for (int k = 0; k < 4; k++) if (x[r][k] != 0) s_stage[rank++] = x[r][k];
        }
        __syncthreads();
        for (int i = tid; i < total; i += SC_THREADS) __builtin_nontemporal_store(s_stage[i], out + (long long)excl + i);
        if (tid == 0 && tbase + SC_TILE >= n) *count = excl + total;
    }
}

inline int sc_tiles(int n) { return (int)(((long long)n + SC_TILE - 1) / SC_TILE); }

int onepass_device(int n, int *d_out, const int *d_in, int *d_count, void *d_ws, hipStream_t st, bool compact) {
    const int ntiles = sc_tiles(n);
    unsigned *ticket = (unsigned *)d_ws;
    u64 *status = (u64 *)((char *)d_ws + SC_HEAD);
    PT_HC(hipMemsetAsync(d_ws, 0, SC_HEAD + sizeof(u64) * (size_t)ntiles, st));
    if (compact) hipLaunchKernelGGL((k_onepass<true, SC_COMPACT_THREADS>), dim3(ntiles), dim3(SC_COMPACT_THREADS), 0, st, n, d_in, d_out, ticket, status, d_count);
    else hipLaunchKernelGGL((k_onepass<false, SC_SCAN_THREADS>), dim3(ntiles), dim3(SC_SCAN_THREADS), 0, st, n, d_in, d_out, ticket, status, d_count);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

// what the host-pointer entry points time: `run` on the null stream between the two events of a timed region, the milliseconds in g_gpu_ms
template <class Run> int timed_on_null_stream(Run run) {
    TimedRegion timed;
    PT_HC(timed.begin(0));
    const int rc = run();
    PT_HC(timed.end(&g_gpu_ms));
    return rc;
}

// host-pointer scan shared by the three reference entry points (naive.cu:32, efficient.cu:35, thrust.cu:20)
int host_scan(int n, int *odata, const int *idata) {
    if (n <= 0) return PTX_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        ptx_internal_set_error("no HIP device available; the GPU scan has no CPU path (use sc_cpu_scan)");
        return PTX_ERR_NODEVICE;
    }
    DevBuf<int> d_in, d_out;
    DevBuf<char> d_ws;
    PT_HC(d_in.upload(idata, (size_t)n));
    PT_HC(d_out.alloc((size_t)n));
    PT_HC(d_ws.alloc(sc_scan_workspace_bytes(n)));
    const int rc = timed_on_null_stream([&] { return onepass_device(n, d_out, d_in, nullptr, d_ws, 0, false); });
    if (rc == PTX_OK) PT_HC(d_out.download(odata));
    return rc;
}

// host-pointer compaction (efficient.cu:79-136): *count survivors in odata
int compact_host(int n, int *odata, const int *idata, int *count) {
    DevBuf<int> d_in, d_out, d_count;
    DevBuf<char> d_ws;
    PT_HC(d_in.upload(idata, (size_t)n));
    PT_HC(d_out.alloc((size_t)n));
    PT_HC(d_count.alloc(1));
    PT_HC(d_ws.alloc(sc_scan_workspace_bytes(n)));
    if (const int rc = timed_on_null_stream([&] { return sc_compact_device(n, d_out, d_in, d_count, d_ws, nullptr); })) return rc;
    PT_HC(d_count.download(count));
    if (*count > 0) PT_HC(hipMemcpy(odata, d_out, sizeof(int) * (size_t)*count, hipMemcpyDeviceToHost));
    return PTX_OK;
}

struct CpuTimer {
    std::chrono::high_resolution_clock::time_point t0 = std::chrono::high_resolution_clock::now();
    ~CpuTimer() { g_cpu_ms = std::chrono::duration<float, std::milli>(std::chrono::high_resolution_clock::now() - t0).count(); }
};


// ---- records: a stable counting sort by a small integer key (sc_sort_records_by_key_device, sc_partition_records_device,
// sc_compact_records_device) ------------------------------------------------------------------------------------------------------
// What the reference's loop asks of thrust per bounce (src/pathtrace.cu:418-428, 518, 541): sort_by_key of 32-byte intersections by
// materialId with the 44-byte path segments as values, then stable_partition of the segments by remainingBounces.  Both are ONE
// mechanism here -- partition is the two-key case (kept = key 0), compaction is partition that never writes key 1 -- in three
// kernels ordered by the stream:
//   count: a workgroup takes the tile of SR_TILE consecutive elements, reads every key straight out of the caller's array (an int at
//          keys + i * stride, so a field of a record serves) and leaves the tile's count per key in table[key][tile];
//   scan : ONE exclusive scan over the key-major table (the library's own k_onepass, in place) makes table[key][tile] the global start
//          of the tile's run of that key: everything of smaller keys, then the same key in earlier tiles;
//   move : the same tile again.  An element's rank among the tile's elements of its key = ballot of the key over the wave + popcount
//          below the lane (one trip per distinct key in the wave, as k_bounce ranks its bins), plus the counts of the earlier
//          (round, wave) groups, scanned per key through LDS.  The tile is then ordered by (key, rank) INSIDE LDS -- source slot and
//          global destination per sorted position -- and the records are copied in that order, a record's dwords (or quads) on
//          consecutive lanes: every key's run of the tile is one contiguous store stream, the loads gather inside the tile.
// No workgroup waits for another (the scan's look-back is the only one) and the only atomics add up the count kernel's LDS histogram:
// a destination is a function of the keys alone, so the result is stable and the same on every run.  A key outside [0, nkeys) is clamped in both phases alike.
constexpr int SR_THREADS = 256, SR_WAVES = SR_THREADS / 64, SR_ROUNDS = 8;
constexpr int SR_TILE = SR_THREADS * SR_ROUNDS;                // 2048 elements: a 3840x2160 frame is 4050 tiles, its 7-key table 28350 ints
constexpr int SR_RW = SR_ROUNDS * SR_WAVES;                    // (round, wave) groups of 64 consecutive elements
constexpr int SR_MAXKEYS = 256, SR_MAXBYTES = 256;

struct SrKeys {
    const char *keys;
    int stride, nkeys, flags, descending;                      // flags: key = value != 0 ? 0 : 1 (kept first)
};
struct SrArray {
    void *out;
    const void *in;
    int units;                                                 // 16-byte or 4-byte units per record
    unsigned magic;                                            // floor(2^32 / units) + 1: idx / units = umulhi(idx, magic) for idx < 2^17, units in 2..64
    int vec16;
};

__device__ __forceinline__ int sr_key(const SrKeys &K, long long i) {
    const int v = *reinterpret_cast<const int *>(K.keys + i * K.stride);
    if (K.flags) return v != 0 ? 0 : 1;
    const int c = min(max(v, 0), K.nkeys - 1);
    return K.descending ? K.nkeys - 1 - c : c;
}

__global__ __launch_bounds__(SR_THREADS) void k_records_count(int n, int tiles, SrKeys K, int *__restrict__ table) {
    __shared__ int s_hist[SR_WAVES][SR_MAXKEYS];               // a row per wave: its atomics only count, and only against its own later rounds
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
    const long long tbase = (long long)tile * SR_TILE;
    for (int k = lane; k < K.nkeys; k += 64) s_hist[wave][k] = 0;
    int kk[SR_ROUNDS];
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; r++) {
        const long long i = tbase + r * SR_THREADS + tid;
        kk[r] = i < n ? sr_key(K, i) : -1;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; r++) {
        unsigned long long remaining = __builtin_amdgcn_uicmp((uint32_t)kk[r], 0xffffffffu, 33);      // lanes with an element
        while (remaining) {
            const int leader = __ffsll((long long)remaining) - 1;
            const int b = __builtin_amdgcn_readlane(kk[r], leader);
            const unsigned long long m = __builtin_amdgcn_uicmp((uint32_t)kk[r], (uint32_t)b, 32);
            if (lane == leader) atomicAdd(&s_hist[wave][b], (int)__popcll(m));
            remaining &= ~m;
        }
    }
    __syncthreads();
    for (int k = tid; k < K.nkeys; k += SR_THREADS) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < SR_WAVES; w++) c += s_hist[w][k];
        table[(size_t)k * tiles + tile] = c;
    }
}

template <typename V>
__device__ __forceinline__ void sr_copy(const SrArray &A, long long tbase, int placed, const uint16_t *s_src, const int *s_dst, int tid) {
    const V *__restrict__ src = reinterpret_cast<const V *>(A.in) + tbase * A.units;
    V *__restrict__ dst = reinterpret_cast<V *>(A.out);
    const unsigned units = (unsigned)A.units, total = (unsigned)placed * units;
#pragma unroll 4
    for (unsigned idx = tid; idx < total; idx += SR_THREADS) {
        const unsigned p = units == 1 ? idx : __umulhi(idx, A.magic), w = idx - p * units;
        dst[(long long)s_dst[p] * units + w] = src[(unsigned)s_src[p] * units + w];
    }
}

__global__ __launch_bounds__(SR_THREADS) void k_records_move(int n, int tiles, SrKeys K, const int *__restrict__ table, SrArray A, SrArray B,
                                                            int *__restrict__ perm, int *__restrict__ totals, int ntotals, int compact) {
    __shared__ uint16_t s_cnt[SR_RW * SR_MAXKEYS];             // [group][key] counts (<= 64), then per key their exclusive prefixes (< 2048)
    __shared__ int s_kstart[SR_MAXKEYS], s_gbase[SR_MAXKEYS];  // where a key's run starts: in the tile's sorted order, and in the output
    __shared__ uint16_t s_src[SR_TILE];                        // per sorted position of the tile: the element's slot in the tile
    __shared__ int s_dst[SR_TILE];                             //                                  and its place in the output
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, nkeys = K.nkeys;
    const long long tbase = (long long)tile * SR_TILE;
    const int cnt = (int)min((long long)SR_TILE, n - tbase);

    for (int q = tid; q < SR_RW * nkeys / 2; q += SR_THREADS) reinterpret_cast<uint32_t *>(s_cnt)[q] = 0u;      // (SR_RW is even)
    int kk[SR_ROUNDS], rk[SR_ROUNDS];
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; r++) {
        const long long i = tbase + r * SR_THREADS + tid;
        kk[r] = i < n ? sr_key(K, i) : -1;
    }
    for (int k = tid; k < nkeys; k += SR_THREADS) s_gbase[k] = table[(size_t)k * tiles + tile];
    if (tile == 0 && totals)                                   // elements per key = the distance between the keys' first starts
        for (int k = tid; k < ntotals; k += SR_THREADS) totals[k] = (k + 1 < nkeys ? table[(size_t)(k + 1) * tiles] : n) - table[(size_t)k * tiles];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; r++) {
        rk[r] = 0;
        unsigned long long remaining = __builtin_amdgcn_uicmp((uint32_t)kk[r], 0xffffffffu, 33);
        while (remaining) {
            const int leader = __ffsll((long long)remaining) - 1;
            const int b = __builtin_amdgcn_readlane(kk[r], leader);
            const unsigned long long m = __builtin_amdgcn_uicmp((uint32_t)kk[r], (uint32_t)b, 32);
            const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (kk[r] == b) rk[r] = below;
            if (lane == leader) s_cnt[(r * SR_WAVES + wave) * nkeys + b] = (uint16_t)__popcll(m);
            remaining &= ~m;
        }
    }
    __syncthreads();
    for (int k = tid; k < nkeys; k += SR_THREADS) {            // per key: exclusive prefix over the groups, in tile order
        int run = 0;
        for (int g = 0; g < SR_RW; g++) {
            const int c = s_cnt[g * nkeys + k];
            s_cnt[g * nkeys + k] = (uint16_t)run;
            run += c;
        }
        s_kstart[k] = run;
    }
    __syncthreads();
    if (wave == 0) {                                           // exclusive prefix over the keys' totals, four keys per lane
        int t[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) { t[j] = 4 * lane + j < nkeys ? s_kstart[4 * lane + j] : 0; sum += t[j]; }
        int run = wave_inclusive_scan(sum, lane) - sum;
#pragma unroll
        for (int j = 0; j < 4; j++) { if (4 * lane + j < nkeys) s_kstart[4 * lane + j] = run; run += t[j]; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; r++)
        if (kk[r] >= 0) {
            const int off = s_cnt[(r * SR_WAVES + wave) * nkeys + kk[r]] + rk[r], p = s_kstart[kk[r]] + off;
            s_src[p] = (uint16_t)(r * SR_THREADS + tid);
            s_dst[p] = s_gbase[kk[r]] + off;
        }
    __syncthreads();
    const int placed = compact ? s_kstart[1] : cnt;            // compaction: the kept ones (key 0) and nothing else
    if (A.vec16) sr_copy<v4i>(A, tbase, placed, s_src, s_dst, tid); else sr_copy<int>(A, tbase, placed, s_src, s_dst, tid);
    if (B.in) { if (B.vec16) sr_copy<v4i>(B, tbase, placed, s_src, s_dst, tid); else sr_copy<int>(B, tbase, placed, s_src, s_dst, tid); }
    if (perm)
        for (int p = tid; p < placed; p += SR_THREADS) perm[s_dst[p]] = (int)(tbase + s_src[p]);
}

inline int sr_tiles(int n) { return n > 0 ? (int)(((long long)n + SR_TILE - 1) / SR_TILE) : 1; }

int sr_invalid(const char *what, const char *name, long long value, const char *rule) {
    ptx_internal_set_error((std::string(what) + ": " + name + " = " + std::to_string(value) + " " + rule).c_str());
    return PTX_ERR_INVALID;
}

// the limits that need no pointer and no device
int sr_check_sizes(const char *what, int n, int nkeys, int stride, int bytes_a, int bytes_b, bool has_b) {
    if (n < 0) return sr_invalid(what, "n", n, "is negative");
    if (nkeys < 1 || nkeys > SR_MAXKEYS) return sr_invalid(what, "nkeys", nkeys, "is outside 1..256");
    if (stride < 4 || stride % 4) return sr_invalid(what, "key_stride_bytes", stride, "must be a multiple of 4, at least 4");
    if (bytes_a < 4 || bytes_a > SR_MAXBYTES || bytes_a % 4) return sr_invalid(what, "record_bytes", bytes_a, "must be a multiple of 4 in 4..256");
    if (has_b && (bytes_b < 4 || bytes_b > SR_MAXBYTES || bytes_b % 4)) return sr_invalid(what, "record_bytes_b", bytes_b, "must be a multiple of 4 in 4..256");
    if ((long long)nkeys * sr_tiles(n) > 0x7fffffffLL) return sr_invalid(what, "nkeys * tiles", (long long)nkeys * sr_tiles(n), "does not fit the scan's int");
    return PTX_OK;
}

int sr_no_device(const char *what) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) return PTX_OK;
    ptx_internal_set_error((std::string(what) + ": no HIP device available; the record sort has no CPU path").c_str());
    return PTX_ERR_NODEVICE;
}

SrArray sr_array(void *out, const void *in, int bytes) {
    SrArray a;
    a.out = out; a.in = in;
    a.vec16 = in && bytes % 16 == 0 && (((uintptr_t)out | (uintptr_t)in) & 15) == 0;
    a.units = bytes / (a.vec16 ? 16 : 4);
    a.magic = a.units > 1 ? (unsigned)(0x100000000ULL / (unsigned)a.units) + 1u : 0u;
    return a;
}

// one entry path: flags = partition / compaction (two keys, kept first), totals: ntotals ints (nkeys for the sort, the count otherwise)
int records_device(const char *what, int n, int nkeys, int descending, bool flags, bool compact, const void *d_keys, int stride,
                   void *d_out_a, const void *d_in_a, int bytes_a, void *d_out_b, const void *d_in_b, int bytes_b,
                   int *d_perm, int *d_totals, int ntotals, void *d_ws, hipStream_t st) {
    const bool has_b = d_out_b || d_in_b || bytes_b;
    if (int rc = sr_check_sizes(what, n, nkeys, stride, bytes_a, bytes_b, has_b)) return rc;
    if (n > 0) {
        if (!d_keys || !d_out_a || !d_in_a || !d_ws || (has_b && (!d_out_b || !d_in_b))) return sr_invalid(what, "a device pointer", 0, "is null");
        if (((uintptr_t)d_ws) & 7) return sr_invalid(what, "d_workspace", (long long)(uintptr_t)d_ws, "must be 8-byte aligned");
        if ((((uintptr_t)d_keys | (uintptr_t)d_out_a | (uintptr_t)d_in_a | (uintptr_t)d_out_b | (uintptr_t)d_in_b | (uintptr_t)d_perm) & 3))
            return sr_invalid(what, "a device pointer", 0, "is not 4-byte aligned");
        if (d_out_a == d_in_a || (has_b && (d_out_b == d_in_b || d_out_b == d_in_a || d_out_a == d_in_b || d_out_a == d_out_b)))
            return sr_invalid(what, "d_out", (long long)(uintptr_t)d_out_a, "is an input or the other output: there is no in-place form");
    }
    if (int rc = sr_no_device(what)) return rc;
    if (n == 0) {
        if (d_totals) PT_HC(hipMemsetAsync(d_totals, 0, sizeof(int) * (size_t)ntotals, st));
        return PTX_OK;
    }
    const int tiles = sr_tiles(n), m = nkeys * tiles;
    int *table = (int *)((char *)d_ws + sc_scan_workspace_bytes(m));
    SrKeys K;
    K.keys = (const char *)d_keys; K.stride = stride; K.nkeys = nkeys; K.flags = flags; K.descending = descending != 0;
    hipLaunchKernelGGL(k_records_count, dim3(tiles), dim3(SR_THREADS), 0, st, n, tiles, K, table);
    PT_HC(hipGetLastError());
    if (int rc = onepass_device(m, table, table, nullptr, d_ws, st, false)) return rc;
    hipLaunchKernelGGL(k_records_move, dim3(tiles), dim3(SR_THREADS), 0, st, n, tiles, K, (const int *)table, sr_array(d_out_a, d_in_a, bytes_a),
                       sr_array(has_b ? d_out_b : nullptr, has_b ? d_in_b : nullptr, has_b ? bytes_b : 4), d_perm, d_totals, ntotals, compact ? 1 : 0);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

// host-pointer forms: allocate, copy in, run on the null stream, copy out -- as sc_efficient_compact does for ints
int records_host(const char *what, int n, int nkeys, int descending, bool flags, bool compact, const int *keys,
                 void *out_a, const void *in_a, int bytes_a, void *out_b, const void *in_b, int bytes_b, int *perm, int *totals, int ntotals) {
    const bool has_b = out_b || in_b || bytes_b;
    if (int rc = sr_check_sizes(what, n, nkeys, 4, bytes_a, bytes_b, has_b)) return rc;
    if (n > 0 && (!keys || !out_a || !in_a || (has_b && (!out_b || !in_b)))) return sr_invalid(what, "a host pointer", 0, "is null");
    if (int rc = sr_no_device(what)) return rc;
    if (n == 0) { for (int k = 0; totals && k < ntotals; k++) totals[k] = 0; return PTX_OK; }
    DevBuf<int> d_keys, d_perm, d_tot;                         // (d_in_b, d_out_b and d_perm stay NULL where the caller has none)
    DevBuf<char> d_in_a, d_out_a, d_in_b, d_out_b, d_ws;
    const size_t na = (size_t)n * bytes_a, nb = has_b ? (size_t)n * bytes_b : 0;
    PT_HC(d_keys.upload(keys, (size_t)n));
    PT_HC(d_in_a.upload(in_a, na)); PT_HC(d_out_a.alloc(na));
    if (has_b) { PT_HC(d_in_b.upload(in_b, nb)); PT_HC(d_out_b.alloc(nb)); }
    if (perm) PT_HC(d_perm.alloc((size_t)n));
    PT_HC(d_tot.alloc((size_t)ntotals));
    PT_HC(d_ws.alloc(sc_records_workspace_bytes(n, nkeys)));
    if (const int rc = timed_on_null_stream([&] { return records_device(what, n, nkeys, descending, flags, compact, d_keys, 4, d_out_a, d_in_a, bytes_a,
                                                                        d_out_b, d_in_b, bytes_b, d_perm, d_tot, ntotals, d_ws, 0); })) return rc;
    int first = 0;                                             // partition / compaction: the count; what compaction wrote ends there
    PT_HC(hipMemcpy(&first, d_tot, sizeof(int), hipMemcpyDeviceToHost));
    if (totals) PT_HC(d_tot.download(totals));
    const size_t written = compact ? (size_t)first : (size_t)n;
    if (written) PT_HC(hipMemcpy(out_a, d_out_a, written * bytes_a, hipMemcpyDeviceToHost));
    if (has_b && written) PT_HC(hipMemcpy(out_b, d_out_b, written * bytes_b, hipMemcpyDeviceToHost));
    if (perm && written) PT_HC(hipMemcpy(perm, d_perm, sizeof(int) * written, hipMemcpyDeviceToHost));
    return PTX_OK;
}


// ---- records by full 32-bit keys: an LSD radix sort on top of the counting pass (sc_radix_sort_records_device) ------------------------
// thrust::sort_by_key sorts by any int; the counting sort above takes 256 distinct keys.  This is the general case: the caller's 32 key
// bits are mapped to an unsigned u whose order is the key type's (rx_map), and the field (u >> begin_bit) & (2^(end_bit - begin_bit) - 1)
// is sorted 8 bits at a time, least significant digit first, every pass stable.  What the passes move is (u, source index) pairs, held
// structure-of-arrays in the workspace; the wide records move ONCE, in a gather behind the last pass.
//   pass  : count -> scan -> move over the same SR_TILE tiles and the same key-major table[digit][tile] as the counting sort, the scan
//           being the library's own k_onepass.  The first pass reads the caller's strided keys and maps them (the source index is the
//           position); later passes read one pair buffer and write the other.  The last pass writes the indices alone.
//   rank  : inside a wave, by a constant eight ballots -- one per digit bit, ANDed (or AND-NOTed) into the lane's peer mask -- and
//           mbcnt below the lane, where k_records_move takes one trip per distinct key (up to 64 with random digits).  Groups and digits
//           are then combined through the same [32 groups][256] uint16 LDS counts.
//   move  : every pair is put at its sorted position of the tile in LDS and the tile is stored in that order: a digit's run of a tile is
//           one contiguous store stream.  The destination of position p is recomputed from its digit (table start + p - the digit's
//           start in the tile), so no destination array is kept.
//   gather: out[p] = in[index[p]] for one or two arrays, a record's dwords (or quads) on consecutive lanes as sr_copy has them; the
//           same kernel writes d_perm and d_keys_out (the caller's original bits, fetched through the index).
// As above no atomic decides a rank (they add up the count kernel's LDS histogram and nothing else), so a destination is a function of
// the keys alone.  Whatever comes out of the workspace and becomes an address -- a table entry, a source index -- is clamped below n
// first: a workspace that something else scribbled on between the kernels gives a wrong order, never an address outside the arrays.
constexpr int RX_BITS = 8, RX_DIGITS = 1 << RX_BITS;
static_assert(RX_DIGITS == SR_MAXKEYS, "the radix passes share the counting sort's table and LDS count layout");

__host__ __device__ inline unsigned rx_map(int key_type, int descending, unsigned bits) {
    unsigned u = bits;
    if (key_type == SC_KEY_INT32) u = bits ^ 0x80000000u;
    else if (key_type == SC_KEY_FLOAT32) u = (bits >> 31) ? ~bits : bits | 0x80000000u;
    return descending ? ~u : u;
}

struct RxKeys {
    const char *keys;                                          // the caller's: first pass and gather
    int stride, key_type, descending;
    const unsigned *u_in, *i_in;                               // later passes: the pair buffer to read (u_in == nullptr: first pass)
    int shift, bits;                                           // this pass's digit = (u >> shift) & ((1 << bits) - 1)
};

__device__ __forceinline__ unsigned rx_u(const RxKeys &K, long long i) {
    if (K.u_in) return K.u_in[i];
    return rx_map(K.key_type, K.descending, *reinterpret_cast<const unsigned *>(K.keys + i * K.stride));
}
__device__ __forceinline__ int rx_digit(const RxKeys &K, unsigned u) { return (int)((u >> K.shift) & ((1u << K.bits) - 1u)); }

__global__ __launch_bounds__(SR_THREADS) void k_radix_count(int n, int tiles, RxKeys K, int *__restrict__ table) {
    __shared__ int s_hist[SR_WAVES][RX_DIGITS];                // a row per wave; the atomics only count
    const int tid = threadIdx.x, wave = tid >> 6, tile = blockIdx.x, nd = 1 << K.bits;
    const long long tbase = (long long)tile * SR_TILE;
    for (int k = tid; k < SR_WAVES * RX_DIGITS; k += SR_THREADS) (&s_hist[0][0])[k] = 0;
    unsigned u[SR_ROUNDS];
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; r++) {
        const long long i = tbase + r * SR_THREADS + tid;
        u[r] = i < n ? rx_u(K, i) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; r++)
        if (tbase + r * SR_THREADS + tid < n) atomicAdd(&s_hist[wave][rx_digit(K, u[r])], 1);
    __syncthreads();
    for (int k = tid; k < nd; k += SR_THREADS) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < SR_WAVES; w++) c += s_hist[w][k];
        table[(size_t)k * tiles + tile] = c;
    }
}

__global__ __launch_bounds__(SR_THREADS) void k_radix_move(int n, int tiles, RxKeys K, const int *__restrict__ table,
                                                          unsigned *__restrict__ u_out, unsigned *__restrict__ i_out) {
    __shared__ alignas(8) uint16_t s_cnt[SR_RW * RX_DIGITS];   // [group][digit] counts (<= 64), then per digit their exclusive prefixes (< 2048)
    __shared__ int s_kstart[RX_DIGITS], s_gbase[RX_DIGITS];    // where a digit's run starts: in the tile's sorted order, and in the output
    __shared__ unsigned s_u[SR_TILE], s_i[SR_TILE];            // the tile's pairs in sorted order
    static_assert(sizeof(s_cnt) % 8 == 0 && __alignof__(s_cnt) >= 8, "s_cnt is zeroed in words: aligned and a whole number of them");
    const int tid = threadIdx.x, wave = tid >> 6, tile = blockIdx.x, nd = 1 << K.bits;
    const long long tbase = (long long)tile * SR_TILE;
    const int cnt = (int)min((long long)SR_TILE, n - tbase);

    for (int q = tid; q < SR_RW * nd / 2; q += SR_THREADS) reinterpret_cast<uint32_t *>(s_cnt)[q] = 0u;      // (SR_RW is even)
    unsigned u[SR_ROUNDS], src[SR_ROUNDS];
    int rk[SR_ROUNDS];
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; r++) {
        const int slot = r * SR_THREADS + tid;
        u[r] = slot < cnt ? rx_u(K, tbase + slot) : 0u;
        src[r] = slot < cnt ? (K.i_in ? K.i_in[tbase + slot] : (unsigned)(tbase + slot)) : 0u;
    }
    // (fence: a table entry becomes the base of store addresses)
    for (int k = tid; k < nd; k += SR_THREADS) s_gbase[k] = (int)min((unsigned)table[(size_t)k * tiles + tile], (unsigned)n);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; r++) {
        const bool valid = r * SR_THREADS + tid < cnt;
        const int d = rx_digit(K, u[r]);
        unsigned long long peers = __ballot(valid);            // the lanes with this lane's digit: one ballot per digit bit
#pragma unroll
        for (int b = 0; b < RX_BITS; b++) {
            const bool bit = (d >> b) & 1;
            const unsigned long long set = __ballot(valid && bit);
            peers &= bit ? set : ~set;
        }
        rk[r] = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
        if (valid && rk[r] == 0) s_cnt[(r * SR_WAVES + wave) * nd + d] = (uint16_t)__popcll(peers);
    }
    __syncthreads();
    for (int k = tid; k < nd; k += SR_THREADS) {               // per digit: exclusive prefix over the groups, in tile order
        int run = 0;
        for (int g = 0; g < SR_RW; g++) {
            const int c = s_cnt[g * nd + k];
            s_cnt[g * nd + k] = (uint16_t)run;
            run += c;
        }
        s_kstart[k] = run;
    }
    __syncthreads();
    if (wave == 0) {                                           // exclusive prefix over the digits' totals, four digits per lane
        const int lane = tid;
        int t[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) { t[j] = 4 * lane + j < nd ? s_kstart[4 * lane + j] : 0; sum += t[j]; }
        int run = wave_inclusive_scan(sum, lane) - sum;
#pragma unroll
        for (int j = 0; j < 4; j++) { if (4 * lane + j < nd) s_kstart[4 * lane + j] = run; run += t[j]; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; r++)
        if (r * SR_THREADS + tid < cnt) {
            const int d = rx_digit(K, u[r]);
            const int p = s_kstart[d] + s_cnt[(r * SR_WAVES + wave) * nd + d] + rk[r];
            s_u[p] = u[r];
            s_i[p] = src[r];
        }
    __syncthreads();
    for (int p = tid; p < cnt; p += SR_THREADS) {
        const unsigned v = s_u[p];
        const int d = rx_digit(K, v);
        // (fence: table start + place in the run, below n whatever the table held)
        const unsigned dst = min((unsigned)s_gbase[d] + (unsigned)(p - s_kstart[d]), (unsigned)(n - 1));
        if (u_out) u_out[dst] = v;
        i_out[dst] = s_i[p];
    }
}

template <typename V>
__device__ __forceinline__ void rx_gather_copy(const SrArray &A, long long tbase, int cnt, const int *s_idx, int tid) {
    const V *__restrict__ src = reinterpret_cast<const V *>(A.in);
    V *__restrict__ dst = reinterpret_cast<V *>(A.out) + tbase * A.units;
    const unsigned units = (unsigned)A.units, total = (unsigned)cnt * units;
#pragma unroll 4
    for (unsigned idx = tid; idx < total; idx += SR_THREADS) {
        const unsigned p = units == 1 ? idx : __umulhi(idx, A.magic), w = idx - p * units;
        dst[idx] = src[(long long)s_idx[p] * units + w];
    }
}

// out[p] = in[index[p]] (index == nullptr: the identity, a copy); d_perm[p] = index[p]; d_keys_out[p] = the caller's key bits of that row
__global__ __launch_bounds__(SR_THREADS) void k_radix_gather(int n, RxKeys K, const unsigned *__restrict__ index, SrArray A, SrArray B,
                                                            int *__restrict__ perm, unsigned *__restrict__ keys_out) {
    __shared__ int s_idx[SR_TILE];
    const int tid = threadIdx.x;
    const long long tbase = (long long)blockIdx.x * SR_TILE;
    const int cnt = (int)min((long long)SR_TILE, n - tbase);
    for (int p = tid; p < cnt; p += SR_THREADS) {
        // (fence: a source index becomes a load address)
        const int s = index ? (int)min(index[tbase + p], (unsigned)(n - 1)) : (int)(tbase + p);
        s_idx[p] = s;
        if (perm) perm[tbase + p] = s;
        if (keys_out) keys_out[tbase + p] = *reinterpret_cast<const unsigned *>(K.keys + (long long)s * K.stride);
    }
    __syncthreads();
    if (A.vec16) rx_gather_copy<v4i>(A, tbase, cnt, s_idx, tid); else rx_gather_copy<int>(A, tbase, cnt, s_idx, tid);
    if (B.in) { if (B.vec16) rx_gather_copy<v4i>(B, tbase, cnt, s_idx, tid); else rx_gather_copy<int>(B, tbase, cnt, s_idx, tid); }
}

// workspace: [the scan's own, for 256 * tiles ints][the table, 256 * tiles ints][u0][i0][u1][i1], n words each, every part 8-byte aligned
struct RxLayout { unsigned long long table, pair[4], total; };
RxLayout rx_layout(int n) {
    RxLayout L;
    const unsigned long long m = (unsigned long long)RX_DIGITS * sr_tiles(n), words = ((unsigned long long)n * 4 + 7) & ~7ull;
    L.table = (sc_scan_workspace_bytes((int)m) + 7) & ~7ull;
    L.pair[0] = L.table + ((m * 4 + 7) & ~7ull);
    for (int k = 1; k < 4; k++) L.pair[k] = L.pair[k - 1] + words;
    L.total = L.pair[3] + words;
    return L;
}

int rx_check(const char *what, int n, int key_type, int begin_bit, int end_bit, int stride, int bytes_a, int bytes_b, bool has_b) {
    if (key_type != SC_KEY_INT32 && key_type != SC_KEY_UINT32 && key_type != SC_KEY_FLOAT32) return sr_invalid(what, "key_type", key_type, "is none of SC_KEY_INT32, SC_KEY_UINT32, SC_KEY_FLOAT32");
    if (begin_bit < 0 || begin_bit > 32) return sr_invalid(what, "begin_bit", begin_bit, "is outside 0..32");
    if (end_bit < 0 || end_bit > 32) return sr_invalid(what, "end_bit", end_bit, "is outside 0..32");
    if (begin_bit > end_bit) return sr_invalid(what, "begin_bit", begin_bit, "is above end_bit");
    return sr_check_sizes(what, n, RX_DIGITS, stride, bytes_a, bytes_b, has_b);
}

int radix_device(const char *what, int n, int key_type, int descending, int begin_bit, int end_bit, const void *d_keys, int stride,
                 void *d_out_a, const void *d_in_a, int bytes_a, void *d_out_b, const void *d_in_b, int bytes_b,
                 int *d_perm, void *d_keys_out, void *d_ws, hipStream_t st) {
    const bool has_b = d_out_b || d_in_b || bytes_b;
    if (int rc = rx_check(what, n, key_type, begin_bit, end_bit, stride, bytes_a, bytes_b, has_b)) return rc;
    if (n > 0) {
        if (!d_keys || !d_out_a || !d_in_a || !d_ws || (has_b && (!d_out_b || !d_in_b))) return sr_invalid(what, "a device pointer", 0, "is null");
        if (((uintptr_t)d_ws) & 7) return sr_invalid(what, "d_workspace", (long long)(uintptr_t)d_ws, "must be 8-byte aligned");
        if ((((uintptr_t)d_keys | (uintptr_t)d_out_a | (uintptr_t)d_in_a | (uintptr_t)d_out_b | (uintptr_t)d_in_b | (uintptr_t)d_perm | (uintptr_t)d_keys_out) & 3))
            return sr_invalid(what, "a device pointer", 0, "is not 4-byte aligned");
        if (d_out_a == d_in_a || d_out_a == d_keys || (has_b && (d_out_b == d_in_b || d_out_b == d_in_a || d_out_a == d_in_b || d_out_a == d_out_b || d_out_b == d_keys)))
            return sr_invalid(what, "d_out", (long long)(uintptr_t)d_out_a, "is an input or the other output: there is no in-place form");
        if (d_keys_out && (d_keys_out == d_keys || d_keys_out == d_in_a || d_keys_out == d_in_b || d_keys_out == d_out_a || d_keys_out == d_out_b || d_keys_out == (void *)d_perm))
            return sr_invalid(what, "d_keys_out", (long long)(uintptr_t)d_keys_out, "is an input or another output: there is no in-place form");
        if (d_perm && ((void *)d_perm == d_keys || (void *)d_perm == d_in_a || (void *)d_perm == d_in_b || (void *)d_perm == d_out_a || (void *)d_perm == d_out_b))
            return sr_invalid(what, "d_perm", (long long)(uintptr_t)d_perm, "is an input or another output");
    }
    if (int rc = sr_no_device(what)) return rc;
    if (n == 0) return PTX_OK;
    const int tiles = sr_tiles(n);
    const RxLayout L = rx_layout(n);
    int *table = (int *)((char *)d_ws + L.table);
    unsigned *buf[4];
    for (int k = 0; k < 4; k++) buf[k] = (unsigned *)((char *)d_ws + L.pair[k]);
    RxKeys K;
    K.keys = (const char *)d_keys; K.stride = stride; K.key_type = key_type; K.descending = descending != 0;
    K.u_in = nullptr; K.i_in = nullptr; K.shift = 0; K.bits = 0;
    const int passes = (end_bit - begin_bit + RX_BITS - 1) / RX_BITS;
    for (int p = 0; p < passes; p++) {
        K.shift = begin_bit + RX_BITS * p;
        K.bits = std::min(RX_BITS, end_bit - K.shift);
        const bool last = p + 1 == passes;
        unsigned *u_out = last ? nullptr : buf[2 * (p & 1)], *i_out = buf[2 * (p & 1) + 1];
        hipLaunchKernelGGL(k_radix_count, dim3(tiles), dim3(SR_THREADS), 0, st, n, tiles, K, table);
        PT_HC(hipGetLastError());
        if (int rc = onepass_device((1 << K.bits) * tiles, table, table, nullptr, d_ws, st, false)) return rc;
        hipLaunchKernelGGL(k_radix_move, dim3(tiles), dim3(SR_THREADS), 0, st, n, tiles, K, (const int *)table, u_out, i_out);
        PT_HC(hipGetLastError());
        K.u_in = u_out; K.i_in = i_out;
    }
    hipLaunchKernelGGL(k_radix_gather, dim3(tiles), dim3(SR_THREADS), 0, st, n, K, (const unsigned *)K.i_in, sr_array(d_out_a, d_in_a, bytes_a),
                       sr_array(has_b ? d_out_b : nullptr, has_b ? d_in_b : nullptr, has_b ? bytes_b : 4), d_perm, (unsigned *)d_keys_out);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

int radix_host(const char *what, int n, int key_type, int descending, int begin_bit, int end_bit, const void *keys,
               void *out_a, const void *in_a, int bytes_a, void *out_b, const void *in_b, int bytes_b, int *perm, void *keys_out) {
    const bool has_b = out_b || in_b || bytes_b;
    if (int rc = rx_check(what, n, key_type, begin_bit, end_bit, 4, bytes_a, bytes_b, has_b)) return rc;
    if (n > 0 && (!keys || !out_a || !in_a || (has_b && (!out_b || !in_b)))) return sr_invalid(what, "a host pointer", 0, "is null");
    if (int rc = sr_no_device(what)) return rc;
    if (n == 0) return PTX_OK;
    DevBuf<int> d_keys, d_perm, d_kout;                        // (d_in_b, d_out_b, d_perm and d_kout stay NULL where the caller has none)
    DevBuf<char> d_in_a, d_out_a, d_in_b, d_out_b, d_ws;
    const size_t na = (size_t)n * bytes_a, nb = has_b ? (size_t)n * bytes_b : 0;
    PT_HC(d_keys.upload(keys, (size_t)n));
    PT_HC(d_in_a.upload(in_a, na)); PT_HC(d_out_a.alloc(na));
    if (has_b) { PT_HC(d_in_b.upload(in_b, nb)); PT_HC(d_out_b.alloc(nb)); }
    if (perm) PT_HC(d_perm.alloc((size_t)n));
    if (keys_out) PT_HC(d_kout.alloc((size_t)n));
    PT_HC(d_ws.alloc(sc_radix_workspace_bytes(n)));
    if (const int rc = timed_on_null_stream([&] { return radix_device(what, n, key_type, descending, begin_bit, end_bit, d_keys, 4, d_out_a, d_in_a, bytes_a,
                                                                      d_out_b, d_in_b, bytes_b, d_perm, d_kout, d_ws, 0); })) return rc;
    PT_HC(d_out_a.download(out_a));
    if (has_b) PT_HC(d_out_b.download(out_b));
    if (perm) PT_HC(d_perm.download(perm));
    if (keys_out) PT_HC(d_kout.download(keys_out));
    return PTX_OK;
}

}  // namespace

extern "C" {

// ---- StreamCompaction::CPU (host code by definition: these are the reference's CPU entry points) ---------------
// cpu.cu:20-32
void sc_cpu_scan(int n, int *odata, const int *idata) {
    CpuTimer tm;
    if (n <= 0) return;
    odata[0] = idata[0];
    for (int i = 1; i < n; i++) odata[i] = odata[i - 1] + idata[i];
    for (int i = 0; i < n; i++) odata[i] -= idata[i];
}

// cpu.cu:39-51
int sc_cpu_compact_without_scan(int n, int *odata, const int *idata) {
    CpuTimer tm;
    int num = 0;
    for (int i = 0; i < n; i++) if (idata[i] != 0) odata[num++] = idata[i];
    return num;
}

// cpu.cu:58-95: map, scan, scatter
int sc_cpu_compact_with_scan(int n, int *odata, const int *idata) {
    if (n <= 0) return 0;
    int *flags = new int[n];
    int *pos = new int[n];
    int num = 0;
    {
        CpuTimer tm;
        for (int i = 0; i < n; i++) flags[i] = idata[i] == 0 ? 0 : 1;
        pos[0] = flags[0];
        for (int i = 1; i < n; i++) pos[i] = pos[i - 1] + flags[i];
        for (int i = 0; i < n; i++) pos[i] -= flags[i];
        for (int i = 0; i < n; i++) if (flags[i] == 1) { odata[pos[i]] = idata[i]; num++; }
    }
    delete[] flags;
    delete[] pos;
    return num;
}

int sc_naive_scan(int n, int *odata, const int *idata) { return host_scan(n, odata, idata); }
int sc_efficient_scan(int n, int *odata, const int *idata) { return host_scan(n, odata, idata); }
int sc_thrust_scan(int n, int *odata, const int *idata) { return host_scan(n, odata, idata); }

// efficient.cu:79-136
int sc_efficient_compact(int n, int *odata, const int *idata) {
    if (n <= 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        ptx_internal_set_error("no HIP device available; the GPU compaction has no CPU path (use sc_cpu_compact_*)");
        return -1;
    }
    int count = -1;
    return compact_host(n, odata, idata, &count) == PTX_OK ? count : -1;      // (the reference's int: -1 for every failure)
}

unsigned long long sc_scan_workspace_bytes(int n) {
    // the ticket counter and one status word per tile; the workspace must be 8-byte aligned (any hipMalloc is)
    return SC_HEAD + sizeof(u64) * (unsigned long long)(n > 0 ? sc_tiles(n) : 1);
}

int sc_scan_device(int n, int *d_odata, const int *d_idata, void *d_workspace, void *stream) {
    if (n <= 0) return PTX_OK;
    if (!d_odata || !d_idata || !d_workspace) { ptx_internal_set_error("null device pointer"); return PTX_ERR_INVALID; }
    if (((uintptr_t)d_workspace) & 7) { ptx_internal_set_error("workspace must be 8-byte aligned"); return PTX_ERR_INVALID; }
    return onepass_device(n, d_odata, d_idata, nullptr, d_workspace, (hipStream_t)stream, false);
}

// d_odata must not alias d_idata: a tile's survivors land where an earlier position's tile may still be reading
int sc_compact_device(int n, int *d_odata, const int *d_idata, int *d_count, void *d_workspace, void *stream) {
    if (!d_count) { ptx_internal_set_error("null device pointer"); return PTX_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    if (n <= 0) { PT_HC(hipMemsetAsync(d_count, 0, sizeof(int), st)); return PTX_OK; }
    if (!d_odata || !d_idata || !d_workspace) { ptx_internal_set_error("null device pointer"); return PTX_ERR_INVALID; }
    if (((uintptr_t)d_workspace) & 7) { ptx_internal_set_error("workspace must be 8-byte aligned"); return PTX_ERR_INVALID; }
    return onepass_device(n, d_odata, d_idata, d_count, d_workspace, st, true);
}

// StreamCompaction::Common::kernMapToBoolean / kernScatter (stream_compaction/common.cu:25-49) on device arrays.  The library's own
// compaction fuses both into k_onepass and never materialises bools[] or indices[]; these exist for callers that built their own
// pipeline on the reference's two kernels (map -> their scan -> scatter).
int sc_map_to_boolean_device(int n, int *d_bools, const int *d_idata, void *stream) {
    if (n <= 0) return PTX_OK;
    if (!d_bools || !d_idata) { ptx_internal_set_error("null device pointer"); return PTX_ERR_INVALID; }
    const int n4 = (((uintptr_t)d_bools | (uintptr_t)d_idata) & 15) == 0 ? n / 4 : 0;
    const int work = n4 + (n - 4 * n4);
    hipLaunchKernelGGL(k_map_to_boolean, dim3((unsigned)std::min(8192, (work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, n4, d_bools, d_idata);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

int sc_scatter_device(int n, int *d_odata, const int *d_idata, const int *d_bools, const int *d_indices, void *stream) {
    if (n <= 0) return PTX_OK;
    if (!d_odata || !d_idata || !d_bools || !d_indices) { ptx_internal_set_error("null device pointer"); return PTX_ERR_INVALID; }
    hipLaunchKernelGGL(k_scatter, dim3((unsigned)std::min(8192, (n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, d_odata, d_idata, d_bools, d_indices);
    PT_HC(hipGetLastError());
    return PTX_OK;
}

// ---- records (kernels and limits: k_records_count / k_records_move above) -----------------------------------------------------
int sc_records_tile_elements(void) { return SR_TILE; }

// [the scan's own workspace for nkeys * tiles ints][the table, nkeys * tiles ints, scanned in place]; 0 for arguments the calls refuse
unsigned long long sc_records_workspace_bytes(int n, int nkeys) {
    if (n < 0 || nkeys < 1 || nkeys > SR_MAXKEYS || (long long)nkeys * sr_tiles(n) > 0x7fffffffLL) return 0;
    const int m = nkeys * sr_tiles(n);
    return sc_scan_workspace_bytes(m) + ((sizeof(int) * (unsigned long long)m + 7) & ~7ull);
}

// thrust::sort_by_key(dev_intersections, ..., dev_paths, sortByMaterial())  src/pathtrace.cu:418-422,518
int sc_sort_records_by_key_device(int n, int nkeys, int descending, const void *d_keys, int key_stride_bytes,
                                  void *d_out_a, const void *d_in_a, int record_bytes_a, void *d_out_b, const void *d_in_b, int record_bytes_b,
                                  int *d_perm, int *d_key_totals, void *d_workspace, void *stream) {
    return records_device("sc_sort_records_by_key_device", n, nkeys, descending, false, false, d_keys, key_stride_bytes, d_out_a, d_in_a, record_bytes_a,
                          d_out_b, d_in_b, record_bytes_b, d_perm, d_key_totals, nkeys, d_workspace, (hipStream_t)stream);
}

// thrust::stable_partition(dev_paths, ..., isTerminate())  src/pathtrace.cu:424-428,541
int sc_partition_records_device(int n, int record_bytes, void *d_out, const void *d_in, const void *d_flags, int flag_stride_bytes, int *d_count,
                                void *d_workspace, void *stream) {
    if (!d_count) { ptx_internal_set_error("sc_partition_records_device: d_count is null"); return PTX_ERR_INVALID; }
    return records_device("sc_partition_records_device", n, 2, 0, true, false, d_flags, flag_stride_bytes, d_out, d_in, record_bytes, nullptr, nullptr, 0,
                          nullptr, d_count, 1, d_workspace, (hipStream_t)stream);
}

int sc_compact_records_device(int n, int record_bytes, void *d_out, const void *d_in, const void *d_flags, int flag_stride_bytes, int *d_count,
                              void *d_workspace, void *stream) {
    if (!d_count) { ptx_internal_set_error("sc_compact_records_device: d_count is null"); return PTX_ERR_INVALID; }
    return records_device("sc_compact_records_device", n, 2, 0, true, true, d_flags, flag_stride_bytes, d_out, d_in, record_bytes, nullptr, nullptr, 0,
                          nullptr, d_count, 1, d_workspace, (hipStream_t)stream);
}

int sc_sort_records_by_key(int n, int nkeys, int descending, const int *keys, void *out_a, const void *in_a, int record_bytes_a,
                           void *out_b, const void *in_b, int record_bytes_b, int *perm, int *key_totals) {
    return records_host("sc_sort_records_by_key", n, nkeys, descending, false, false, keys, out_a, in_a, record_bytes_a, out_b, in_b, record_bytes_b,
                        perm, key_totals, nkeys);
}

int sc_partition_records(int n, int record_bytes, void *out, const void *in, const int *flags, int *count) {
    if (!count) { ptx_internal_set_error("sc_partition_records: count is null"); return PTX_ERR_INVALID; }
    return records_host("sc_partition_records", n, 2, 0, true, false, flags, out, in, record_bytes, nullptr, nullptr, 0, nullptr, count, 1);
}

int sc_compact_records(int n, int record_bytes, void *out, const void *in, const int *flags, int *count) {
    if (!count) { ptx_internal_set_error("sc_compact_records: count is null"); return PTX_ERR_INVALID; }
    return records_host("sc_compact_records", n, 2, 0, true, true, flags, out, in, record_bytes, nullptr, nullptr, 0, nullptr, count, 1);
}

// ---- records by full 32-bit keys (kernels and limits: k_radix_count / k_radix_move / k_radix_gather above) -------------------------
unsigned long long sc_radix_workspace_bytes(int n) { return n < 0 ? 0 : rx_layout(n).total; }

unsigned int sc_radix_map_key(int key_type, int descending, unsigned int bits) { return rx_map(key_type, descending != 0, bits); }

// thrust::sort_by_key with keys of any value: int, unsigned or float, a bit range of them, ascending or descending
int sc_radix_sort_records_device(int n, int key_type, int descending, int begin_bit, int end_bit, const void *d_keys, int key_stride_bytes,
                                 void *d_out_a, const void *d_in_a, int record_bytes_a, void *d_out_b, const void *d_in_b, int record_bytes_b,
                                 int *d_perm, void *d_keys_out, void *d_workspace, void *stream) {
    return radix_device("sc_radix_sort_records_device", n, key_type, descending, begin_bit, end_bit, d_keys, key_stride_bytes, d_out_a, d_in_a, record_bytes_a,
                        d_out_b, d_in_b, record_bytes_b, d_perm, d_keys_out, d_workspace, (hipStream_t)stream);
}

int sc_radix_sort_records(int n, int key_type, int descending, int begin_bit, int end_bit, const void *keys, void *out_a, const void *in_a, int record_bytes_a,
                          void *out_b, const void *in_b, int record_bytes_b, int *perm, void *keys_out) {
    return radix_host("sc_radix_sort_records", n, key_type, descending, begin_bit, end_bit, keys, out_a, in_a, record_bytes_a, out_b, in_b, record_bytes_b,
                      perm, keys_out);
}

float sc_last_gpu_ms(void) { return g_gpu_ms; }
float sc_last_cpu_ms(void) { return g_cpu_ms; }

// common.h:21-31
int sc_ilog2(int x) { int lg = 0; while (x >>= 1) ++lg; return lg; }
int sc_ilog2ceil(int x) { return x == 1 ? 0 : sc_ilog2(x - 1) + 1; }

}  // extern "C"
