// pt_plan.h -- launch planning (pt_plan.hip): the PTX_DEBUG_* switches, read once, and everything the engine decides from sizes alone --
// iterations per launch set, the grids, LDS sizes and table strides of a launch set, the cut of a short run.  The unit holds no kernel and
// calls no hip* runtime function, so a CPU program links it without a GPU (tests/launch_plan_check.cpp does, under the sanitizers).
#pragma once
#include <string>

#include "pt_scene.h"

namespace ptd {

constexpr int MAX_LANES = 8;     // launch sets in flight at most (ptx_options.lanes)

// Every PTX_DEBUG_* variable the engine reads, as read_debug_switches found it when the tracer was created (a variable changed later
// changes nothing: the cached camera bounce keeps state that depends on them).  0 / false = not set.  The table is in DESIGN.md 5.
struct DebugSwitches {
    SceneSwitches scene;               // ... those of scene preparation (pt_scene.h)
    bool no_tile_geoms = false;        // PTX_DEBUG_NO_TILE_GEOMS: no per-tile geom masks on the camera bounce (tests of both)
    bool no_tile_geoms_dof = false;    // PTX_DEBUG_NO_TILE_GEOMS_DOF: none with depth of field only
    bool no_fast = false;              // PTX_DEBUG_NO_FAST: always the general k_bounce (A/B timing, tests of both variants)
    bool no_last = false;              // PTX_DEBUG_NO_LAST: the last bounce runs the full k_bounce like every other (A/B timing, tests of both)
    bool last_inplace = false;         // PTX_DEBUG_LAST_INPLACE: the light-only last bounce without the pool of survivors over tiles (A/B timing, tests of both)
    bool force_fast = false;           // PTX_DEBUG_FORCE_FAST: ask for the specialised variant at every launch (refused with PTX_ERR_INVALID
                                       // where its preconditions do not hold; tests only)
    bool no_tangents = false;          // PTX_DEBUG_NO_TANGENTS: DScene::ctan is NULL, every lane computes its frame (A/B timing, tests of both)
    bool no_unit_rsqrt = false;        // PTX_DEBUG_NO_UNIT_RSQRT: levels 0 and 1 from the code objects built without pt_rsqrt_unit and the shared reciprocal
                                       // of the slab test (pt_device.h; A/B timing, tests of both)
    bool keep_dir_skip = false;        // PTX_DEBUG_KEEP_DIR_SKIP: a debug capture leaves the record masks on (tests only)
    bool no_idx16 = false;             // PTX_DEBUG_NO_IDX16: the two-word local index everywhere (tests of both forms)
    bool tail_index = false;           // PTX_DEBUG_TAIL_INDEX: the chunk-compact local index written by k_bounce's tail everywhere (A/B timing, tests of both)
    bool no_priority = false;          // PTX_DEBUG_NO_PRIORITY: every stream at the default priority (tuning experiments)
    bool no_first_fusion = false;      // PTX_DEBUG_NO_FIRST_FUSION: the split camera bounce without BounceParams::tile_done (tuning experiments)
    int wg_per_cu = 0;                 // PTX_DEBUG_WG_PER_CU (>= 1): the grid is what it says for every kernel (tuning experiments only)
    int total_wg_per_cu = 0;           // PTX_DEBUG_TOTAL_WG_PER_CU: grid of a whole launch (tuning experiments)
    int wg_first = 0, wg_later = 0, wg_last = 0;      // PTX_DEBUG_WG_FIRST / _LATER / _LAST (>= 1): workgroups per CU of the specialised unsplit bounces (tuning experiments)
    int gx_last = 0;                   // PTX_DEBUG_GX_LAST (>= 1), tests only: at most that many workgroups per segment on the light-only last bounce, so that a
                                       // small frame gives a workgroup many tiles -- its pool of light-box survivors fills and drains as it does at 1080p
    int mesh_wg_per_cu = 0;            // PTX_DEBUG_MESH_WG_PER_CU: workgroups per CU of k_mesh's grid (tuning experiments)
    int extra_lds = 0;                 // PTX_DEBUG_EXTRA_LDS: bytes added to k_bounce's LDS, a multiple of 16 up to 32768 (occupancy experiments)
    int nsets = 0;                     // PTX_DEBUG_NSETS: sets of a short run (tuning experiments)
    int first_set = 0;                 // PTX_DEBUG_FIRST_SET: iterations of a two-set run's first set (tuning experiments only)
    long long split_min_paths = 1LL << 20;      // PTX_DEBUG_SPLIT_MIN (>= 1): smallest launch set a short run is cut into (tuning experiments only)
    long long mem_budget_mb = 0;       // PTX_DEBUG_MEM_BUDGET_MB (>= 1): plan_launch_sets' budget (tests only)
    long long fence_slots = 0;         // PTX_DEBUG_FENCE_SLOTS (>= 1; the tracer clamps it to its slots): entries beyond it are fenced (test of the counter)
    bool has_lane_prio = false;        // PTX_DEBUG_LANE_PRIO = p1,p2,... (HIP priority values; tuning experiments only): lane_prio[l] is lane l's,
    int lane_prio[MAX_LANES] = {};     // the list's last where it is shorter
};
// the one getenv of the engine (but PTX_DEBUG_PREQUEUE_US, see ptx_render_strided); ptx_create calls it once
DebugSwitches read_debug_switches();

// Iterations per launch set and launch sets in flight, from sizes alone: the explicit option, or the rule in pt_plan.hip (about 24 M paths
// per set, within a quarter of the device's memory: mem_free / mem_total, 0 = unknown; budget_mb > 0 = PTX_DEBUG_MEM_BUDGET_MB, tests only),
// then the cap of the out-of-memory retry (kmax_cap > 0), 64, and the 4 GiB of the prefix tables.  refusal: non-empty = nothing fits.
struct LaunchPlan { int kmax = 1, lanes = 1; std::string refusal; };
LaunchPlan plan_launch_sets(int owned_pixels, int nbins, int maxTiles, const ptx_options &opt, int kmax_cap, size_t mem_free, size_t mem_total,
                            long long budget_mb);

// plan_launch_sets' ceiling on what the streams of all launch sets in flight may take, in bytes
long long launch_budget_bytes(size_t mem_free, size_t mem_total, long long budget_mb);

// The plain numbers a launch set's plan depends on, all fixed at create: the tracer (ptx_tracer) is one of these.
struct PlanFacts : SceneFacts {      // (+ what the scene decides about how it is traced, pt_scene.h: ntri, cull, tri_lds, split_mesh, the masks ...)
    int nbins = 1, nmats = 0, ngeoms = 0, maxTiles = 0, cus = 0;
    int grid = 0, grid_seg = 0;        // plan_grids: upper bound of a launch's workgroups / of one segment's (sizes the per-workgroup tables)
    int lanes = 1;                     // launch sets in flight at once
    bool sort_by_material = false;     // ptx_options.sort_by_material
    bool has_bvh = false;              // some mesh has a tree (DScene::bvh_root != NULL)
    DebugSwitches dbg;
    bool grid_forced() const { return dbg.wg_per_cu > 0; }
};
void plan_grids(PlanFacts &f);       // grid, grid_seg from cus, maxTiles and the switches

// What enqueue_batch launches a set of K iterations with (K segments of every launch: blockIdx.y)
struct BatchPlan {
    bool fast_unsplit = false;                   // the grids are those of the specialised unsplit kernel (an estimate, see plan_batch)
    int gx_first = 1, gx_later = 1, gx_last = 1; // workgroups per segment: camera bounce, later bounces, the light-only last bounce
    int finish_grid = 1, finish_gx = 1;          // k_finish's grid-stride launch: in all, per segment
    int mesh_gx = 1;                             // k_mesh's workgroups per segment
    size_t lds_bounce = 0, lds_pass2 = 0, lds_mesh = 0;      // bytes: k_bounce (unsplit, and pass 1 of the split bounce), its ranking pass, k_mesh
    int idx16_first = 0, idx16_later = 0;        // BounceParams::idx16 of a launch of gx_first / gx_later workgroups per segment
    size_t chunk_cap = 0;                        // runs per table at most
    size_t seg_counts = 0, seg_chunk = 0;        // words per segment of d_counts (two prefix tables + stored paths per tile) / d_chunk
};
// defer: traced ahead of per-call requests; needs_albedo: the set contains iteration 1 of the apps variant
BatchPlan plan_batch(const PlanFacts &f, int K, bool defer, bool needs_albedo);

// The form of the local index (BounceParams::loop_idx), fixed at create for all of a tracer's launches.  loop: bin-major, written in
// k_bounce's tile loop -- only where ALL of these hold: the switch PTX_DEBUG_TAIL_INDEX is not set; the bounce is unsplit (MODE 0: no
// k_mesh / k_finish, whose ranking pass writes keys for the tail); at most 64 bins; the direct epilogue is compiled in; an entry's byte
// offset fits 32 bits (nbins * N2 <= 2^30); and the streams with the nbins-fold index still fit the memory rule at the kmax chosen:
// bytes_per_path x lanes x owned x kmax <= the budget, where bytes_per_path = plan_launch_sets' 176 - the three int words of two stages
// (24) + the index of two stages, 2 x 4 x words x nbins x N2 / slots rounded up.  Otherwise today's tail and layout, and `why` says which
// term failed.  words: 1 where every launch set the tracer can plan (K = 1 .. kmax, traced ahead or not, with or without the albedo
// AOV) has the one-word form, else 2.
struct IndexPlan {
    bool loop = false;
    int n2_log2 = 0;                   // N2 = 1 << n2_log2: the smallest power of two >= slots
    int words = 1;                     // words allocated per entry
    size_t entries = 0;                // nbins * N2: the bound an entry is checked against, and the words of one table
    size_t seg_words = 0;              // entries * words: what one segment's index takes (the allocation is that per segment)
    long long bytes_per_path = 176;    // per path and iteration of a launch set, all streams
    const char *why = "";              // loop == false: the term that failed ...
    int why_code = 0;                  // ... as a number, in the order of the list above (1 = the switch ... 6 = the memory rule)
};
IndexPlan plan_local_index(const PlanFacts &f, int slots, int owned_pixels, int kmax, long long budget_bytes);

// Iterations per launch set of a ptx_render call of `count` iterations: kmax, or the equal cut of a short run over the lanes
int sets_per_call(int count, int kmax, int lanes, int owned_pixels, long long split_min_paths, int dbg_nsets);

}  // namespace ptd
