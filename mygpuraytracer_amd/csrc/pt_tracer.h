// pt_tracer.h -- the tracer itself, for the host units that work on one: struct ptx_tracer with the owned device array its buffers
// are (DevBuf, pt_handle.h), and the few functions of pt_engine.hip that pt_post.hip calls.  pt_engine.hip creates, renders and frees a tracer;
// pt_post.hip hands its buffers to the post-processing units (pt_denoise.hip, pt_temporal.hip, pt_moments.hip, pt_adaptive.hip,
// pt_display.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/mi355x_pathtracer.h"
#include "pt_handle.h"
#include "pt_kernels.h"
#include "pt_scene.h"
#include "pt_plan.h"
#include "pt_denoise.h"

// The kernel unit's tables, one per arithmetic level (pt_kernels.hip).  Levels 1 and 2 are weak: a library linked without their
// objects still loads, and refuses arith != 0.
extern "C" const void *ptx_arith_kernels_0(void);
extern "C" const void *ptx_arith_kernels_1(void) __attribute__((weak));
extern "C" const void *ptx_arith_kernels_2(void) __attribute__((weak));
extern "C" const void *ptx_arith_last_0(void);      // (pt_kernels_last.hip: the light-only last bounce of each level)
extern "C" const void *ptx_arith_last_1(void) __attribute__((weak));
extern "C" const void *ptx_arith_last_2(void) __attribute__((weak));
// the exact and the contracted level once more, compiled with -DPT_UNIT_RSQRT=0 -DPT_SHARED_RCP=0 (pt_device.h): the plain second normalize
// and six divisions per cube pair, for PTX_DEBUG_NO_UNIT_RSQRT -- a switch inside the kernels would cost them a scalar register
extern "C" const void *ptx_arith_kernels_0p(void) __attribute__((weak));
extern "C" const void *ptx_arith_kernels_1p(void) __attribute__((weak));
extern "C" const void *ptx_arith_last_0p(void) __attribute__((weak));
extern "C" const void *ptx_arith_last_1p(void) __attribute__((weak));

// ---------------------------------------------------------------------------------------------------------------
struct ptx_tracer : PlanFacts {       // (+ the sizes its launch plans depend on and the debug switches `dbg`, pt_plan.h; what the scene decides, pt_scene.h)
    int device = 0;
    // Every stream and event, declared in front of the buffers and in this order.  Members go in the reverse of their declaration: a tracer
    // that is deleted frees its buffers first, then destroys its events (kev first, ev_start last), then the lane streams, the main stream
    // last.  free_tracer has synchronised every stream by then -- nothing is enqueued, no wait is pending, no buffer is in use -- so any
    // order would be safe; this one lets go of what was recorded before what it was recorded on.
    OwnedStream stream;                           // the caller's (borrowed: never destroyed) or the tracer's own
    OwnedStream lane_stream[MAX_LANES];           // (lanes, below) [0] = `stream` and stays empty, the others are the tracer's own
    OwnedEvent ev_start, ev_stop, ev_fork, ev_join[MAX_LANES], ev_chain[MAX_LANES];
    OwnedEvent ev_ahead0[MAX_LANES], ev_ahead1[MAX_LANES];      // (render-ahead, below)
    std::vector<OwnedEvent> kev;                  // per-kernel timing, below: pairs (start, stop)
    bool timing_valid = false;
    ptx_options opt{};
    DCamera cam{};
    int traceDepth = 0;
    TileMap tm{};
    int cap = 0;                               // slots of one segment: maxTiles x TILE
    // device memory
    DevBuf<DGeom> d_geoms; DevBuf<DMaterial> d_mats; DevBuf<float> d_faces; DevBuf<uint8_t> d_texels;
    float *d_image = nullptr; DevBuf<float> d_image_own; // d_image: the caller's buffer, or d_image_own
    DevBuf<float> d_fbuf[3];                             // stream, stage, cache
    DevBuf<int32_t> d_ibuf[3];
    PathSoA soa[3];                                      // 0, 1 = the two stages (bounce b writes soa[1 - (b & 1)], b + 1 reads it), 2 = first-bounce cache
    DevBuf<int32_t> d_counts;                            // per segment: [2][nbins][maxTiles] prefix tables + [maxTiles] stored paths per tile
    DevBuf<int32_t> d_chunk;                             // [segments][2 (bounce parity)][3][nbins x grid_seg]: the run tables (BounceParams::chunk)
    DevBuf<int32_t> d_cache_chunk;                       // [3][nbins x grid_seg]: the cached bounce 0's
    DevBuf<int32_t> d_cache_super;                       // [2][nbins][nsuper]: the cached bounce 0's
    int cache_gx = 0;                                    // workgroups per segment of the launch that filled the cache (its run tables' width)
    DevBuf<int32_t> d_totals;                            // [maxBounces][2][nbins] then [maxBounces][2][nbins][nsuper]
    int32_t *d_super = nullptr;                          // (points into d_totals' allocation)
    DevBuf<float> d_tri9, d_gtab, d_aabb, d_objcull;
    std::vector<float> h_aabb;                           // host copy of the world boxes (update_tile_geoms)
    std::vector<int32_t> h_geom_type, h_roots, h_depths, h_wroots, h_wneeds;      // host copies of the per-geom tree tables (ptx_debug_mesh_plan)
    DevBuf<uint32_t> d_tile_geoms; bool tile_geoms_valid = false;      // BounceParams::tile_geoms of the current camera
    // the active-tile mask (ptx_set_active_tiles), both allocated when the first mask is set: the flags, one byte per tile, and the table
    // the camera bounce reads instead of d_tile_geoms while mask_set (written by k_tile_mask alone)
    DevBuf<uint8_t> d_tile_active; DevBuf<uint32_t> d_tile_eff; bool mask_set = false;
    DevBuf<BvhQuad> d_bvh_nodes; DevBuf<float> d_bvh_tris; DevBuf<int32_t> d_bvh_root, d_bvh_depth;                          // pt_bvh.h (NULL: no mesh has one)
    DevBuf<BvhWide4> d_bvh_wide; DevBuf<int32_t> d_bvh_wroot, d_bvh_wneed;                                                   // four-wide nodes of the same trees (k_mesh)
    DevBuf<float> d_fnorm, d_cnorm;                      // precomputed normals (DScene::fnorm / cnorm)
    DevBuf<float> d_ctan;                                // tangent frames of the cubes' tabulated normals (DScene::ctan)
    DevBuf<float> d_ldsblob;                             // DScene::ldsblob for the ntri_lds k_bounce is launched with
    DevBuf<unsigned long long> d_keys; DevBuf<uint32_t> d_items; DevBuf<int32_t> d_item_count;
    DevBuf<int32_t> d_tile_done;                         // split first bounce: [segments][maxTiles], see BounceParams::tile_done
    size_t seg_items = 0;
    int nsuper = 1;
    size_t totals_bytes = 0, seg_totals = 0, field_stride = 0, seg_part = 0;
    int kmax = 1;                                        // iterations per launch set (segments)
    // (lanes, pt_plan.h: each launch set in flight runs on a stream of its own -- lane_stream, with ev_fork / ev_join / ev_chain -- and
    // with its own kmax segments of every per-iteration buffer)
    // Render-ahead for the one-iteration-per-call shape (ptx_iterate = the reference's pathtrace(iter)): lanes 1 and 2 take
    // turns tracing the NEXT kmax iterations into their per-iteration radiance buffers while the caller works the current
    // batch off, one k_gather (+ k_stats) per call on the main stream.  What a call returns is unchanged: the image holds
    // exactly the iterations asked for so far, summed in the same order.
    struct Ahead { int first = 0, count = 0, next = 0, unfolded = 0; bool use_cache = false, valid = false, timed = false;
                   unsigned long long dir_bins = ~0ull, ntab_bins = 0ull; };      // (the record masks the batch was written with: k_stats)
    Ahead ahead[MAX_LANES];
    int ahead_cur = -1, ahead_nxt = -1;                  // lane whose batch is being consumed / lane holding the batch after it
    bool render_ahead = false;
    int last_ahead_lane = -1;                            // != -1: the previous operation was a call served from that lane's batch
    // The lit planes and totals of a lane's segments are zero between its launch sets: the set's k_gather and k_stats clear what they
    // read.  Where that may not hold -- nothing has run yet, a traced-ahead batch was dropped unfinished, a set ended early on an error,
    // the image was reset -- the lane's next set starts with a full clear of both (enqueue_batch).
    bool aux_dirty[MAX_LANES] = {};
    unsigned long long cache_dir_bins = ~0ull, cache_ntab_bins = 0ull;      // ... as the cached camera bounce was written
    int cache_idx16 = 0;                                                    // ... and its local index (BounceParams::idx16)
    bool cache_loop = false;                                                // ... and that index's layout (bit 0 of BounceParams::loop_idx)
    IndexPlan ix;                                                           // the local index's layout, for every launch of this tracer
    DevBuf<uchar4> d_pbo;                                // ptx_write_pbo's device staging (allocated on first use)
    DevBuf<float> d_denoised;                            // ptx_write_denoised_pbo_device's copy of the host frame (first use)
    DevBuf<float> d_albedo;                              // apps variant only: W*H*3
    // denoiser (ptx_denoise), all allocated on its first call: G-buffer [nh | xt | alb] x W*H float4 then W*H int2 ids (pt_denoise.h),
    // the filter's two float4 colour buffers, its W*H*3 result
    DevBuf<float4> d_gbuf, d_dn_tmp;
    DevBuf<float> d_dn_out;
    bool gbuf_valid = false, dn_done = false;            // G-buffer of the current camera / d_dn_out holds a result
    uint64_t gbuf_serial = 0;                            // of the G-buffer's last computation, from a process-wide counter (0: none yet): what a prefilter's cached guides are of
    int guide_first = 1, guide_count = 0;                // ptx_set_guide_samples: count 0 = k_gbuffer's pixel-centre guides, else k_guides over these iterations
    int guide_bounces = 0;                               // ptx_set_guide_bounces: > 0 = k_guides_follow in either mode, the guide rays continued through mirrors and glass
    std::vector<uint8_t> h_spec;                         // per material: reflective or refractive (ptx_denoise_temporal's rule)
    DevBuf<uint8_t> d_spec;                              // its device copy, on the first ptx_denoise_temporal
    DevBuf<float> d_var;                                 // [2][W*H]: v0 and the last pass's v of the last ptx_denoise_variance (first use)
    bool var_done = false;
    DevBuf<unsigned long long> d_stamps;                 // diagnostic build only
    DevBuf<float> d_part;                                // [kmax][W*H*3] per-iteration radiance (batched mode)
    DevBuf<int32_t> d_cache_totals;                      // [2][nbins] of bounce 0 (cache)
    DevBuf<int32_t> d_emit_count, d_emit_pix; DevBuf<float> d_emit_rgb;
    DevBuf<int64_t> d_stats;                             // [64] last iteration, [64] = running total, [65] = fenced indices (BounceParams::fenced), [66..68] = stored paths: all, with direction, with normal code
    int maxBounces = 0;
    bool cache_valid = false;
    int64_t iterations = 0;
    double loop_ms_total = 0.0;
    // optional per-kernel timing (bench.py's roofline leg): events around every launch of an iteration (kev)
    bool ktiming = false;
    std::vector<int> kev_kind;                           // per pair of kev: 0 k_bounce<first>, 1 k_bounce, 2 k_mesh + k_finish, 3 pass 2 of the split bounce (the ranking pass)
    size_t kev_used = 0;
    // debug capture
    int capture_bounce = -1;
    DevBuf<int32_t> d_cap;                               // pix, idx, mg [cap each] + totals
    DevBuf<float> d_cap_f;                               // the 15 float fields [cap each]
    bool cap_filled = false;
    DScene scene() const {
        DScene s; s.geoms = d_geoms; s.mats = d_mats; s.faces = d_faces; s.tri9 = d_tri9; s.texels = d_texels; s.ngeoms = ngeoms; s.nmats = nmats;
        s.gtab = d_gtab; s.aabb = d_aabb; s.cull = 0; s.cube_bits = cube_bits; s.sphere_bits = sphere_bits; s.mesh_bits = mesh_bits; s.light_bits = light_bits;
        s.objcull = d_objcull; s.objcull_bits = objcull_bits;
        s.bvh_nodes = d_bvh_nodes; s.bvh_tris = d_bvh_tris; s.bvh_root = d_bvh_root; s.bvh_depth = d_bvh_depth; s.bvh_wide = d_bvh_wide; s.bvh_wroot = d_bvh_wroot; s.bvh_wneed = d_bvh_wneed; s.bvh_stack = 0; s.ntri_lds = 0; s.mesh_chunks = mesh_chunks;
        s.fnorm = d_fnorm; s.cnorm = d_cnorm; s.bump_bits = bump_bits;
        s.ctan = dbg.no_tangents ? nullptr : d_ctan.p;
        s.tri_lds = 0; s.ntri = ntri;      // tri_lds is switched on only by launches that stage the table (k_bounce)
        s.ldsblob = nullptr;               // (set by enqueue_batch together with tri_lds / ntri_lds: the blob is laid out for those)
        return s;
    }
    bool cache_active() const { return opt.cache_first_bounce && !opt.antialiasing && !opt.depth_of_field; }
    const KernelSet *ks = nullptr;      // the code object the arithmetic-bearing kernels are launched from (ptx_options.arith)
    const LastKernelSet *ksl = nullptr;    // ... and the same level's light-only last bounce
};

// ---- pt_engine.hip's, for pt_post.hip ---------------------------------------------------------------------------
// The G-buffer of the current camera on the tracer's stream (k_gbuffer, or the sampled guides), buffers allocated on first use
int pt_ensure_gbuffer(ptx_tracer *t);
// why this tracer cannot take a mask of `ntiles` flags (the code through `code`), or NULL
const char *pt_active_tiles_problem(const ptx_tracer *t, int ntiles, int &code);
// The mask `d_flags` (one byte per tile on the device; NULL: the tracer's own copy) made the tracer's, in the order of a camera change:
// what is on the tracer's stream ends, what was traced ahead is dropped, then the table is written by a launch of its own
int pt_set_tile_mask(ptx_tracer *t, const uint8_t *d_flags);

// What a call that needs the whole frame says to a tracer that renders a row tile (`fn`: the entry point's name), else PTX_OK
inline int pt_whole_frame_problem(const char *fn, const ptx_tracer *t) {
    if (t->tm.tile_world <= 1) return PTX_OK;
    return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": this tracer renders a row tile (tile_world > 1); its frame holds only its own rows");
}
