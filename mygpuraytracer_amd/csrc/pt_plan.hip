// pt_plan.hip -- launch planning as host-only code (pt_plan.h): the debug switches and the integer arithmetic that turns a tracer's sizes
// into launch sets, grids and LDS bytes.  No __global__ function and no hip* runtime call, so a CPU program links this object without a
// GPU; compiled as HIP with pt_engine.hip's flags because the LDS sizes are pt_kernels.h's own constexpr functions.  Frames are
// bit-identical whatever the grid: a slip here costs only speed, so tests/launch_plan_check.cpp pins the numbers.
#include <stdlib.h>
#include <string.h>
#include <algorithm>

#include "pt_plan.h"
#include "pt_kernels.h"

namespace ptd {

DebugSwitches read_debug_switches() {
    DebugSwitches d;
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    auto num = [](const char *name, long long lo, long long unset) { const char *e = getenv(name); return e ? std::max(lo, atoll(e)) : unset; };
    auto count = [](const char *name, int lo) { const char *e = getenv(name); return e ? std::max(lo, atoi(e)) : 0; };
    d.scene.no_wide_bvh = on("PTX_DEBUG_NO_WIDE_BVH"); d.scene.no_chunks = on("PTX_DEBUG_NO_CHUNKS");
    d.scene.no_dir_skip = on("PTX_DEBUG_NO_DIR_SKIP"); d.scene.no_normal_codes = on("PTX_DEBUG_NO_NORMAL_CODES");
    d.scene.force_split = on("PTX_DEBUG_FORCE_SPLIT"); d.scene.no_objcull = on("PTX_DEBUG_NO_OBJCULL");
    d.no_tile_geoms = on("PTX_DEBUG_NO_TILE_GEOMS"); d.no_tile_geoms_dof = on("PTX_DEBUG_NO_TILE_GEOMS_DOF");
    d.no_fast = on("PTX_DEBUG_NO_FAST"); d.no_last = on("PTX_DEBUG_NO_LAST"); d.last_inplace = on("PTX_DEBUG_LAST_INPLACE");
    d.force_fast = on("PTX_DEBUG_FORCE_FAST"); d.no_tangents = on("PTX_DEBUG_NO_TANGENTS"); d.keep_dir_skip = on("PTX_DEBUG_KEEP_DIR_SKIP");
    d.no_unit_rsqrt = on("PTX_DEBUG_NO_UNIT_RSQRT");
    d.tail_index = on("PTX_DEBUG_TAIL_INDEX");
    d.no_idx16 = on("PTX_DEBUG_NO_IDX16"); d.no_priority = on("PTX_DEBUG_NO_PRIORITY"); d.no_first_fusion = on("PTX_DEBUG_NO_FIRST_FUSION");
    d.wg_per_cu = count("PTX_DEBUG_WG_PER_CU", 1);
    d.total_wg_per_cu = count("PTX_DEBUG_TOTAL_WG_PER_CU", 0);
    d.wg_first = count("PTX_DEBUG_WG_FIRST", 1); d.wg_later = count("PTX_DEBUG_WG_LATER", 1); d.wg_last = count("PTX_DEBUG_WG_LAST", 1);
    d.gx_last = count("PTX_DEBUG_GX_LAST", 1);
    d.mesh_wg_per_cu = count("PTX_DEBUG_MESH_WG_PER_CU", 0);
    d.extra_lds = std::min(count("PTX_DEBUG_EXTRA_LDS", 0), 32768) & ~15;
    d.nsets = count("PTX_DEBUG_NSETS", 0);
    if (const char *e = getenv("PTX_DEBUG_FIRST_SET")) d.first_set = atoi(e);
    d.split_min_paths = num("PTX_DEBUG_SPLIT_MIN", 1, d.split_min_paths);
    d.mem_budget_mb = num("PTX_DEBUG_MEM_BUDGET_MB", 1, 0);
    d.fence_slots = num("PTX_DEBUG_FENCE_SLOTS", 1, 0);
    if (const char *e = getenv("PTX_DEBUG_LANE_PRIO")) {
        d.has_lane_prio = true;
        for (int l = 1; l < MAX_LANES; l++) {
            const char *q = e;
            for (int k = 1; k <= l && q; k++) { d.lane_prio[l] = atoi(q); q = strchr(q, ','); if (q) q++; }
        }
    }
    return d;
}

long long launch_budget_bytes(size_t mem_free, size_t mem_total, long long budget_mb) {
    long long budget = 64LL << 30;
    if (mem_total > 0) budget = std::min<long long>(budget, (long long)(std::min(mem_free, mem_total) / 4));
    if (budget_mb > 0) budget = budget_mb << 20;
    return budget;
}

LaunchPlan plan_launch_sets(int owned_pixels, int nbins, int maxTiles, const ptx_options &opt, int kmax_cap, size_t mem_free, size_t mem_total,
                            long long budget_mb) {
    LaunchPlan p;
    // three launch sets in flight (one per stream) unless told otherwise: kernels of different sets overlap and
    // kernel tails are filled (C4, iterations per set x sets: 8 x 1 0.41, 8 x 2 0.30, 12 x 3 0.276, 12 x 4 0.31 ms per
    // iteration); also with one iteration per launch set, i.e. frames so large that only one fits the memory rule below
    // (7680 x 4320: 6.2 -> 4.75 ms per iteration); needs the per-iteration radiance buffers
    p.lanes = opt.lanes >= 1 ? std::min(opt.lanes, MAX_LANES) : 3;
    // With the first-bounce cache the iterations of a batch all start from the one cached bounce-0 stream
    int kmax = opt.batch;
    if (kmax <= 0) {
        // about 24 M paths per launch set, at least 12 iterations: 12 of a 1080p frame, up to 32 of a small frame or of one rank's tile
        // (1/8 of 1080p: 0.058 -> 0.048 ms per iteration with 32 instead of 8), fewer only where the streams of all launch sets in
        // flight (two stages of 19 words + radiance + the split search's keys and queue = 176 B per path and iteration) would pass
        // 64 GB of the 288.  Round 4: 12 instead of 5 at 3840x2160 (the rule was 16 GB with a guessed 400 B per path): every kernel of the
        // split bounce gets 2.4x the work per launch -- C5 1.23 -> 1.17 ms per iteration with round 3's kernels, and what the refilling
        // k_mesh needs: 1.4 M parked rays per launch instead of 0.6 M for the chip's 330 k lanes.
        // Round 5: the 64 GB are a ceiling, not a constant -- a quarter of what the device (a CPX / NPS partition, a GPU shared by
        // several ranks) has free or in total, whichever is less; and an allocation that still fails is retried with half the
        // iterations per set (ptx_create) before the caller is told.
        const long long owned = std::max(owned_pixels, 1);
        long long want = ((24LL << 20) + owned / 2) / owned;
        want = std::min<long long>(32, std::max<long long>(12, want));
        // (176 B is the chunk-compact index's figure; where the bin-major index is wider, plan_local_index takes that form only if the
        // kmax chosen here still fits with ITS bytes per path, so the plans below do not move)
        const long long budget = launch_budget_bytes(mem_free, mem_total, budget_mb);
        kmax = (int)std::min<long long>(want, std::max<long long>(1, budget / (176LL * p.lanes * owned)));
    }
    if (kmax_cap > 0 && kmax > kmax_cap) kmax = kmax_cap;      // (the retry after an allocation failed)
    if (kmax > 64) kmax = 64;
    // the per-tile prefix tables grow with bins x tiles x iterations in flight: keep them under 4 GiB by putting fewer
    // iterations into a launch set, then fewer launch sets in flight
    auto counts_bytes = [&](int k, int l) { return sizeof(int32_t) * (2 * (size_t)nbins + 1) * maxTiles * (size_t)k * l; };
    while (counts_bytes(kmax, p.lanes) > (4ULL << 30) && kmax > 1) kmax /= 2;
    if (counts_bytes(kmax, p.lanes) > (4ULL << 30)) p.lanes = 1;
    if (counts_bytes(kmax, 1) > (4ULL << 30))
        p.refusal = "material sort over " + std::to_string(nbins) + " materials on " + std::to_string(maxTiles) +
                    " tiles needs more than 4 GiB of prefix tables: render with sort_by_material = 0";
    p.kmax = kmax;
    return p;
}

void plan_grids(PlanFacts &f) {
    // 16 per CU: an upper bound (sizes the per-workgroup tables); plan_batch picks 6, 8, 20 or 32 per CU
    // (also for K segments in one launch: a 1/8 tile's ten iterations as 10 x 101 workgroups of 10 tiles run 6 % FASTER than as
    // 10 x 128 of 8 -- a grid that does not quite fill the chip leaves room for the other launch set's kernel to start)
    f.grid = std::max(1, std::min(f.maxTiles, f.cus * (f.grid_forced() ? f.dbg.wg_per_cu : 16)));
    f.grid_seg = std::max(1, std::min(f.grid, f.maxTiles));      // what one segment (iteration) can use: sizes its tables
}

BatchPlan plan_batch(const PlanFacts &f, int K, bool defer, bool needs_albedo) {
    const DebugSwitches &dbg = f.dbg;
    BatchPlan p;
    const bool batched = K > 1 || f.lanes > 1;      // ending paths store into per-iteration buffers, k_gather sums them
    // Only the grid sizes depend on this estimate; what is launched is decided per launch by fast_violation (pt_engine.hip).  Of that
    // predicate's terms it omits: more than 64 bins, depth of field on the camera bounce, a far camera (cull == 2 by the camera's
    // position), the cache-filling pass.  There the general kernel runs on the specialised one's grid; aligning the two would move grids.
    // (the apps variant's x PI at the deposit stays a run-time value in every kernel; its albedo AOV is written by iteration 1 alone,
    // so only a launch set that contains iteration 1 needs the general kernel for it)
    p.fast_unsplit = !f.split_mesh && !dbg.no_fast && batched && !f.uses_uv && f.sort_by_material &&
                     !needs_albedo && f.cull == 1 && f.tri_lds && f.bump_bits == 0 && f.ntri_lds == f.ntri &&
                     !f.has_bvh;
    // Workgroups per CU of a whole launch.
    // The specialised unsplit kernel runs 8 workgroups per CU at a time (PT_FAST_WAVES): the later bounces are ONE round of that occupancy
    // and the camera bounce 20 -- end of round 4, after the records' diet (32 B instead of 56 for a wall hit, 16-byte quads) and with eight
    // workgroups' LDS per CU: C4's 20-step run 0.147 -> 0.1425 ms per step, its long run 0.1415 -> 0.138 (three runs each of six plans on
    // one box; 28 / 14 was the choice while the kernels moved 40 % more bytes and a chunk's tail of index traffic was worth spreading).
    // Why more than one round on the camera bounce: a workgroup owns a contiguous chunk of tiles, and chunks are unequal -- the camera-ray
    // bounce's tiles cost anything from nothing (a tile that sees no geom) to a full tile, the later bounces' tiles differ by material mix --
    // so with one chunk per resident workgroup a kernel ends when its heaviest chunk does; and the other launch sets' short kernels
    // (k_finish, the ranking pass) get a slot only when a workgroup of the long one retires.  Round 4, with the heavier records, on one box
    // each: C4 camera bounce alone 0.0365 (7 per CU) / 0.0338 (14) / 0.0320 (21) / 0.0300 ms (28), later bounces 0.163 / 0.161 / 0.160 /
    // 0.160 / 0.173 (42), wall of the 20-step run 0.176 / 0.172 / 0.173 / 0.173 / 0.179.
    // Traced ahead of per-call requests (defer): two of the eight slots per CU stay free, so that the caller's own short kernels -- gather,
    // preview -- start at once instead of waiting for one of these long-running workgroups to end: 0.53 -> 0.50 ms per call.
    // The split bounce's kernels are many short ones: 32 per CU (C5 16 per CU 1.06-1.10, 32 1.03-1.07, 48 1.04-1.07 ms per iteration);
    // everything else 8.  (Earlier, while the specialised unsplit kernel ran 5 workgroups per CU at a time, a grid of 8 per CU was 1.6 rounds
    // of them: C4 -1.3 %.)
    auto per_cu = [&](bool first_bounce, bool last_bounce = false) {
        if (p.fast_unsplit && !defer && last_bounce && dbg.wg_last > 0) return dbg.wg_last;
        if (p.fast_unsplit && !defer && (first_bounce ? dbg.wg_first : dbg.wg_later) > 0) return first_bounce ? dbg.wg_first : dbg.wg_later;
        if (p.fast_unsplit) return defer ? PT_FAST_WAVES - 2 : first_bounce ? 20 : PT_FAST_WAVES;
        return f.split_mesh ? 32 : 8;
    };
    // Workgroups per segment: the launch's workgroups are sized for the whole chip, WHATEVER one segment holds (round 3: until then the
    // total was capped by one segment's tile count, so the K = 10 segments of a 1/8 tile ran as 1010 workgroups of ten tiles -- 4 per CU --
    // instead of 1790 of six: 20 steps of such a tile 0.636 -> 0.585 ms, tools/gpu_tile_grid_sweep.py)
    auto gx_of = [&](bool first_bounce, bool last_bounce = false) {
        int grid = f.grid_forced() ? f.grid : f.cus * per_cu(first_bounce, last_bounce);
        if (dbg.total_wg_per_cu > 0) grid = f.cus * dbg.total_wg_per_cu;
        int g = grid / K;
        if (!f.grid_forced() && dbg.total_wg_per_cu <= 0) {
            // ... but more than one round of the occupancy only where a workgroup keeps at least ~8 tiles of the camera bounce: a rank's 1/8
            // tile is a chain of dependent round trips per workgroup life, and more workgroups are more prologues there -- 20
            // steps of such a tile 0.54 -> 0.60 ms with the larger grids.  Below that the grid is one round of the occupancy, as before.
            const int base = f.cus * (p.fast_unsplit ? (defer ? PT_FAST_WAVES - 2 : PT_FAST_WAVES) : f.split_mesh ? 16 : 8) / K;
            g = std::min(g, std::max(base, f.maxTiles / 8));
        }
        if (g < 64 && dbg.total_wg_per_cu <= 0) g = 64;
        if (g > f.maxTiles) g = f.maxTiles;
        if (g > f.grid_seg) g = f.grid_seg;
        if (g > grid) g = grid;
        return g < 1 ? 1 : g;
    };
    p.gx_first = gx_of(true); p.gx_later = gx_of(false);
    // the light-only last bounce: the later bounces' grid -- 4 / 8 / 16 workgroups per CU measured alike, profiles/last_bounce_ab.txt
    p.gx_last = gx_of(false, true);
    if (dbg.gx_last > 0) p.gx_last = std::min(dbg.gx_last, p.gx_last);
    p.finish_grid = f.cus * (dbg.total_wg_per_cu > 0 ? dbg.total_wg_per_cu : per_cu(false));
    p.finish_gx = std::max(1, p.finish_grid / K);
    // k_mesh's waves draw from the segment's queue until it is empty: one round of the kernel's occupancy is all the grid needs.
    // Three workgroups per CU (PT_MESH_WG_PER_CU), not the five its LDS would admit: a workgroup holds 31 KB (the walks' stacks), five of
    // them nearly all of a CU's 160 KB -- while k_mesh runs, the OTHER launch sets' kernels then find no LDS to start in and the overlap of
    // the three sets stops.  With three, k_mesh alone is 4 % slower and C5's wall time 2 % shorter (1.066 -> 1.045 ms per iteration; 4:
    // 1.054, 2: 1.059; nine runs each on one box); a wave also draws from 460 rays instead of 270.
    p.mesh_gx = std::max(1, f.cus * (dbg.mesh_wg_per_cu > 0 ? dbg.mesh_wg_per_cu : PT_MESH_WG_PER_CU) / K);
    // (split: the mesh search runs in k_mesh from global memory, so the triangle tables need no LDS)
    const int triWords = f.tri_lds ? sceneTableWords(f.split_mesh ? 0 : f.ntri_lds, f.nmats, f.ngeoms) : 0;
    p.lds_bounce = sizeof(int32_t) * (bounceLdsWords(triWords, f.nbins) + (f.split_mesh ? QUEUE_WORDS : 0)) + (size_t)dbg.extra_lds;
    p.lds_pass2 = sizeof(int32_t) * ((size_t)ldsHeadWords(f.nbins) + TILE);      // (ranking head + one key per slot)
    // the per-lane traversal stack lives in LDS and is what limits k_mesh's occupancy: as many entries as the longest walk needs
    p.lds_mesh = sizeof(int32_t) * ((size_t)f.bvh_stack * 256 + 32 * MESH_GEOM_WORDS);
    // (one-word local index where no workgroup's chunk can pass 128 tiles)
    auto idx16_of = [&](int gxw) { return (!dbg.no_idx16 && (f.maxTiles + gxw - 1) / std::max(gxw, 1) <= 128) ? 1 : 0; };
    p.idx16_first = idx16_of(p.gx_first); p.idx16_later = idx16_of(p.gx_later);
    p.chunk_cap = (size_t)f.nbins * f.grid_seg;
    p.seg_counts = (2 * (size_t)f.nbins + 1) * f.maxTiles; p.seg_chunk = 2 * 3 * p.chunk_cap;
    return p;
}

IndexPlan plan_local_index(const PlanFacts &f, int slots, int owned_pixels, int kmax, long long budget_bytes) {
    IndexPlan x;
    slots = std::max(slots, 1);
    while (((size_t)1 << x.n2_log2) < (size_t)slots) x.n2_log2++;
    const size_t n2 = (size_t)1 << x.n2_log2;
    x.entries = (size_t)std::max(f.nbins, 1) * n2;
    for (int K = 1; K <= std::max(kmax, 1) && x.words == 1; K++)
        for (int v = 0; v < 4 && x.words == 1; v++) {
            const BatchPlan p = plan_batch(f, K, (v & 1) != 0, (v & 2) != 0);
            if (!p.idx16_first || !p.idx16_later) x.words = 2;
        }
    x.seg_words = x.entries * x.words;
    const long long wide = 176 - 24 + (long long)((2 * sizeof(int32_t) * x.seg_words + slots - 1) / slots);
    const long long lanes = std::max(f.lanes, 1), owned = std::max(owned_pixels, 1);
    auto no = [&](int code, const char *why) { x.why_code = code; x.why = why; };
    if (f.dbg.tail_index) no(1, "PTX_DEBUG_TAIL_INDEX");
    else if (f.split_mesh) no(2, "split bounce");
    else if (f.nbins > 64) no(3, "more than 64 bins");
    else if (!PT_DIRECT_STORE) no(4, "no direct epilogue");
    else if (x.entries > ((size_t)1 << 30)) no(5, "index offsets pass 32 bits");
    else if (wide * lanes * owned * std::max(kmax, 1) > budget_bytes) no(6, "memory rule");
    else { x.loop = true; x.bytes_per_path = wide; }
    if (!x.loop) { x.words = 1; x.entries = x.seg_words = 0; }
    return x;
}

int sets_per_call(int count, int kmax, int lanes, int owned_pixels, long long split_min_paths, int dbg_nsets) {
    // A run shorter than lanes x kmax iterations is cut into equal launch sets, one per lane, as long as each keeps at
    // least split_min_paths primary rays (below that the launches no longer fill the chip and overlap buys nothing).
    if (lanes <= 1 || count >= lanes * kmax) return kmax;
    const long long owned = std::max(owned_pixels, 1);
    const int kmin = (int)std::min<long long>(kmax, (split_min_paths + owned - 1) / owned);
    // ... and into TWO sets rather than three while two can hold the call: a one-shot of three sets starts its third
    // late (the host issues the sets one after the other) and makes all of them smaller -- 20 iterations as 10 + 10
    // instead of 7 + 7 + 6: full frame equal, 1/2 tile -2 %, 1/4 and 1/8 tile -7 % (round 3's sweep; tools/gpu_tile_grid_sweep.py is its successor)
    int nsets = count <= 2 * kmax ? std::min(2, lanes) : lanes;
    if (dbg_nsets > 0) nsets = std::min(dbg_nsets, lanes);
    return std::min(kmax, std::max(kmin, (count + nsets - 1) / nsets));
}

}  // namespace ptd
