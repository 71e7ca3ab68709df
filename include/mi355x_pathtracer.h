/* mi355x_pathtracer.h -- C ABI of the MI355X-native path tracer (libmi355x_pathtracer.so).
 *
 * Drop-in boundary for the reference's path-tracing module (nkkk98/MyGPURaytracer, all file:line citations are
 * relative to the reference root):
 *
 *   reference interface                                  this ABI
 *   ---------------------------------------------------  --------------------------------------------------
 *   Scene::Scene(filename)            src/scene.cpp:10    ptx_scene_load / ptx_scene_get_* / ptx_scene_free
 *   runCuda() camera recompute        src/main.cpp:105    ptx_scene_apply_runcuda_camera
 *   pathtraceInit(Scene*)             src/pathtrace.h:7   ptx_create        (scene flattened to POD, options =
 *                                     src/pathtrace.cu:101                   the #defines of pathtrace.cu:36-40)
 *   pathtrace(uchar4* pbo, frame, it) src/pathtrace.h:9   ptx_iterate (+ ptx_write_pbo, ptx_read_image)
 *                                     src/pathtrace.cu:433
 *   pathtraceFree()                   src/pathtrace.h:8   ptx_destroy
 *   timer()                           src/pathtrace.h:6   ptx_last_loop_ms
 *   checkCUDAError -> exit()          src/pathtrace.cu:42 return codes + ptx_last_error()
 *
 * Plain C types only: no C++ classes, no torch types.  Every pointer marked "device" is a HIP device pointer on
 * the device the handle was created on; everything else is host memory.  The C++ veneer with the reference's
 * own names (pathtraceInit / pathtrace / pathtraceFree, class Scene) lives in
 * mygpuraytracer_amd/csrc/pathtrace_api.h and is a few lines over this ABI.
 */
#ifndef MI355X_PATHTRACER_H
#define MI355X_PATHTRACER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision of this header: bumped whenever a struct a caller allocates (ptx_options, ptx_stats, ptx_camera ...) grows or an entry
 * point changes meaning.  A caller compiled against one revision and loaded against a library of another must not hand it those
 * structs: check ptx_abi_version() == PTX_ABI_VERSION after loading (mygpuraytracer_amd/api.py does, and refuses), or use the sized
 * entry points (ptx_get_stats_sized), which never write more than the caller says it has.
 * 5 = round 5: ptx_options.arith; ptx_stats as of round 4 (fenced, stored_*).  Libraries before 5 do not export ptx_abi_version. */
#define PTX_ABI_VERSION 5
int ptx_abi_version(void);
size_t ptx_sizeof_options(void);           /* sizeof(ptx_options) / sizeof(ptx_stats) as the LIBRARY was compiled */
size_t ptx_sizeof_stats(void);

#define PTX_OK 0
#define PTX_ERR_INVALID 1      /* bad argument / malformed scene                      */
#define PTX_ERR_IO 2           /* file could not be read                              */
#define PTX_ERR_HIP 3          /* a HIP runtime call failed (message in ptx_last_error) */
#define PTX_ERR_NODEVICE 4     /* no usable HIP device: there is no CPU fallback      */
#define PTX_ERR_UNSUPPORTED 5

/* enum GeomType, src/sceneStructs.h:10-15 */
enum { PTX_SPHERE = 0, PTX_CUBE = 1, PTX_TRIANGLE = 2, PTX_OBJ = 3 };

/* struct Material, src/sceneStructs.h:71-81 -- same 44-byte layout */
typedef struct ptx_material {
    float color[3];
    float specular_exponent;
    float specular_color[3];
    float hasReflective;
    float hasRefractive;
    float indexOfRefraction;
    float emittance;
} ptx_material;

/* struct Texture, src/sceneStructs.h:36-48 (host pixels; uploaded by ptx_create) */
typedef struct ptx_texture {
    int32_t width, height, channels;
    const uint8_t *image;          /* width*height*channels bytes, or NULL when channels == 0 */
} ptx_texture;

/* struct Geom, src/sceneStructs.h:50-69.  Matrices in glm memory order (column major, m[c*4+r]).
 * faces: faceSize x 15 floats = 3 vertices x (position xyz, texcoord uv) -- the only Face fields the path
 * tracer reads (src/intersections.h:216-262). */
typedef struct ptx_geom {
    int32_t type;
    int32_t materialid;
    float translation[3], rotation[3], scale[3];
    float transform[16], inverseTransform[16], invTranspose[16];
    int32_t faceSize;
    const float *faces;
    ptx_texture kd, ks, bump, ke;
} ptx_geom;

/* struct Camera, src/sceneStructs.h:83-92 */
typedef struct ptx_camera {
    int32_t resolution[2];
    float position[3], lookAt[3], view[3], up[3], right[3];
    float fov[2];
    float pixelLength[2];
} ptx_camera;

/* Runtime form of the compile-time switches of src/pathtrace.cu:36-40 (same defaults via ptx_default_options),
 * plus the multi-GPU row-tile split.  A device owns the row blocks b (of tile_rows rows each) with
 * b % tile_world == tile_rank; pixelIndex stays global (x + y*W). */
typedef struct ptx_options {
    int32_t depth_of_field;      /* DEPTH_OF_FIELD 0      */
    int32_t cache_first_bounce;  /* CACHE_FIRST_BOUNCE 1  */
    int32_t sort_by_material;    /* SORT_BY_MATERIAL 1    */
    int32_t antialiasing;        /* ANTIALIASING 1        */
    int32_t bounding_box;        /* BOUNDING_BOX 0 (accepted, must be 0) */
    int32_t tile_rows, tile_rank, tile_world;   /* 0,0,1 = whole frame */
    int32_t device;              /* HIP device ordinal, -1 = current device */
    int32_t batch;               /* iterations traced per launch set by ptx_render (independent streams, results
                                    identical to one at a time); 0 = choose from the tile size */
    int32_t no_lds_triangles;    /* 1 = read the triangle table from global memory even when it would fit in LDS */
    int32_t apps_variant;        /* 1 = behave like the apps/src copy of the reference (the one its CMake builds):
                                    finalGather adds color * PI (apps/src/pathtrace.cu:508) and iteration 1 fills an
                                    albedo AOV (apps/src/pathtrace.cu:412-462, ptx_read_albedo) */
    int32_t no_cull;             /* 1 = every ray tests every geom (the reference's loop) instead of per-lane candidate
                                    lists from conservative world boxes; results are identical either way */
    int32_t no_bvh;              /* 1 = every mesh is searched by the reference's loop over all its faces; 0 = meshes of
                                    24+ faces get a bounding-volume hierarchy (same nearest face, see csrc/pt_bvh.h)      */
    int32_t lanes;               /* launch sets in flight, each on a stream of its own: 0 = default (3), 1 .. 8 explicit  */
    int32_t no_mesh_split;       /* 1 = meshes are searched inside the bounce kernel even when they have a BVH; 0 = scenes
                                    with BVH meshes run the mesh search as a kernel of its own between two halves of it   */
    int32_t arith;               /* 0 = EXACT (default, and what every headline number is measured with): fp32 without contraction,
                                    IEEE division and square root, own correctly rounded sin/cos -- bit-identical to the CPU
                                    oracle.  1 = CONTRACTED: the same kernels compiled as a second code object with fused
                                    multiply-adds wherever the expression tree allows (what nvcc's default --fmad=true does to
                                    the reference's kernels); division and square root stay IEEE, sine and cosine are an fp32
                                    routine of about one ulp.  2 = FAST: level 1 as a third code object with the hardware's
                                    approximate reciprocal / square root / reciprocal square root (one ulp each, a quotient
                                    a * rcp(b) about 2.5 ulp) and its sine / cosine / exp2 / log2 instructions.  Levels 1 and 2
                                    agree with EXACT within the statistical fp32 tolerance of DESIGN.md section 3
                                    (tests/test_fp_tolerance.py) and, stage by stage, stay within 2 x / 8 x EXACT's own distance
                                    from a float64 reference (tests/test_gpu_arith_f64.py) -- never bit for bit.  ptx_create
                                    returns PTX_ERR_UNSUPPORTED for a level whose code object the library was built without
                                    (it never falls back to another level) and PTX_ERR_INVALID for a value outside 0 .. 2.  */
} ptx_options;
#define PTX_ARITH_EXACT 0
#define PTX_ARITH_CONTRACTED 1
#define PTX_ARITH_FAST 2

typedef struct ptx_stats {
    int32_t bounces;                 /* bounce-loop passes of the last iteration                       */
    int64_t rays_per_bounce[64];     /* paths entering the intersect stage, per bounce (last iteration) */
    int64_t rays_total;              /* sum over all iterations since create/reset                      */
    double loop_ms_total;            /* device time of the bounce loops since create/reset              */
    int64_t iterations;
    int64_t fenced;                  /* indices from internal tables (mesh-search queue, sort index) that the kernels found out of
                                        range and skipped or clamped instead of faulting, since create/reset.  Always 0: anything else
                                        means corrupted internal state (and a wrong pixel somewhere) -- report it                      */
    int64_t stored_paths;            /* paths stored for a next bounce since create/reset, and how many of their records carry ...        */
    int64_t stored_with_direction;   /* ... the incoming direction (reflective / refractive materials, materials of OBJ geoms: 16 B more) */
    int64_t stored_with_normal_code; /* ... a 3-bit code instead of the normal (materials only cubes have: 16 B less)                      */
} ptx_stats;

typedef struct ptx_tracer ptx_tracer;     /* opaque: one scene on one device */
typedef struct ptx_scene ptx_scene;       /* opaque: a loaded scenes/<x>.txt  */

const char *ptx_last_error(void);
int ptx_device_count(void);               /* HIP devices visible; 0 means nothing here can run */
void ptx_default_options(ptx_options *o);

/* ---- scene loader (src/scene.cpp, src/utilities.cpp) ------------------------------------------------------ */
/* Paths inside the scene file ("../models/x.obj", mtl search path "../models/materials") resolve relative to
 * base_dir, which plays the role of the reference's process CWD; NULL = directory of scene_path. */
int ptx_scene_load(const char *scene_path, const char *base_dir, ptx_scene **out);
void ptx_scene_free(ptx_scene *s);
int ptx_scene_num_geoms(const ptx_scene *s);
int ptx_scene_num_materials(const ptx_scene *s);
const ptx_geom *ptx_scene_geoms(const ptx_scene *s);
const ptx_material *ptx_scene_materials(const ptx_scene *s);
ptx_camera *ptx_scene_camera(ptx_scene *s);            /* mutable: RenderState.camera      */
int ptx_scene_iterations(const ptx_scene *s);          /* RenderState.iterations           */
int ptx_scene_trace_depth(const ptx_scene *s);         /* RenderState.traceDepth           */
void ptx_scene_set_trace_depth(ptx_scene *s, int depth);
void ptx_scene_set_resolution(ptx_scene *s, int w, int h);   /* re-derives fov/pixelLength as loadCamera does */
const char *ptx_scene_image_name(const ptx_scene *s);  /* RenderState.imageName            */
void ptx_scene_apply_runcuda_camera(ptx_scene *s);     /* src/main.cpp:56-70 + :105-123    */

/* The interactive camera of src/main.cpp without the window: the state its mouse handlers keep (main.cpp:18-20) and
 * one function per handler, so that a script of events moves the camera exactly as the same drags would.
 * After any of them call ptx_orbit_apply (runCuda's recompute) and hand the camera to the tracer with ptx_set_camera +
 * ptx_reset_image (runCuda restarts the accumulation: iteration = 0, :106). */
typedef struct ptx_orbit { float phi, theta, zoom; float og_look_at[3]; } ptx_orbit;
void ptx_orbit_init(const ptx_scene *s, ptx_orbit *o);                                  /* main.cpp:56-70   */
void ptx_orbit_left_drag(ptx_orbit *o, double dx, double dy, int width, int height);    /* main.cpp:184-189 */
void ptx_orbit_right_drag(ptx_orbit *o, double dy, int height);                         /* main.cpp:190-194 */
void ptx_orbit_middle_drag(ptx_scene *s, double dx, double dy);                         /* main.cpp:195-209 */
void ptx_orbit_recenter(ptx_scene *s, const ptx_orbit *o);                              /* SPACE, :166-171  */
void ptx_orbit_apply(ptx_scene *s, const ptx_orbit *o);                                 /* main.cpp:105-123 */

/* ---- tracer ------------------------------------------------------------------------------------------------ */
/* pathtraceInit.  external_image: optional device buffer of W*H*3 floats to accumulate into (caller keeps
 * ownership, e.g. a torch tensor that is later reduced over RCCL); NULL = the tracer allocates and zeroes one.
 * stream: optional hipStream_t to run on; NULL = the tracer creates its own (non-blocking) stream.
 * Ordering is the caller's: whatever initialised external_image (a fill, a checkpoint copy) must have COMPLETED, or have
 * been issued on `stream`, before the first render call -- the tracer's stream does not wait for other streams. */
int ptx_create(int ngeoms, const ptx_geom *geoms, int nmaterials, const ptx_material *materials,
               const ptx_camera *camera, int trace_depth, const ptx_options *options,
               float *external_image, void *stream, ptx_tracer **out);
int ptx_create_from_scene(const ptx_scene *s, const ptx_options *options, float *external_image, void *stream,
                          ptx_tracer **out);
void ptx_destroy(ptx_tracer *t);                        /* pathtraceFree; NULL is a no-op */

int ptx_set_camera(ptx_tracer *t, const ptx_camera *camera, int trace_depth);  /* camera edits without re-init */
int ptx_reset_image(ptx_tracer *t);

/* ---- active tiles: switch parts of the frame off ------------------------------------------------------------------
 * A tile is ptx_tile_pixels() consecutive owned pixels, tile = (y * W + x) / ptx_tile_pixels() -- one workgroup pass of the
 * camera bounce; a tracer has ptx_num_tiles(t) of them, the last one maybe partial.  While a mask is set, the camera bounce
 * of an inactive tile generates no rays, tests nothing and stores nothing: its paths end black and deposit nothing, so its
 * pixels of the accumulation buffer keep their bits, and no later bounce sees them.  The path kernels are the same: the mask
 * is ANDed into the per-tile table of visible geoms they read anyway (a tile that sees no geom takes the same way out).
 *   Iteration numbers go on counting for the whole frame (they seed the RNG).  The shading RNG is also seeded by a path's place
 *   in the material-sorted stream, which the missing paths shift: an active pixel receives another sample of the same
 *   distribution than it would without a mask, not the same bits (a mask that switches off only tiles that see no geom shifts
 *   nothing: the same bits).  ptx_stats.rays_per_bounce[0] still counts every owned pixel (a masked tile's paths are
 *   survivors in the miss bin of the camera bounce); ptx_write_pbo divides by the iteration it is given and ptx_read_image
 *   returns the raw sums, whatever the tiles received -- ptx_adaptive_resolve normalises tile by tile.
 *   Setting or clearing is ordered like a camera change: it waits for the tracer's stream and drops what was traced ahead
 *   (ptx_set_render_ahead), then writes the table with a launch on that stream.  A camera change (ptx_set_camera) keeps the mask.
 * host_active: ntiles bytes, != 0 = active.  Refused: PTX_ERR_INVALID for tile_world > 1 or ntiles != ptx_num_tiles(t);
 * PTX_ERR_UNSUPPORTED for a tracer without that table (no_cull, more than 32 geoms) or with the first-bounce cache in use
 * (cache_first_bounce without antialiasing and depth of field: it replays a camera bounce of the whole frame).  The tracer
 * stays usable, without a mask or with the one it had.  Without a mask every launch is what it is without these calls. */
int ptx_tile_pixels(void);
int ptx_num_tiles(const ptx_tracer *t);
int ptx_set_active_tiles(ptx_tracer *t, const uint8_t *host_active, int ntiles);
int ptx_clear_active_tiles(ptx_tracer *t);              /* no mask set: a no-op */

/* One iteration of pathtrace() (iter is 1-based and seeds the RNG).  Enqueues on the tracer's stream and
 * returns without waiting; any read entry point below synchronises. */
int ptx_iterate(ptx_tracer *t, int iter);
/* Render-ahead for callers that keep the reference's shape -- one pathtrace(iter) per call, iter counting up
 * (src/main.cpp:128-148).  on != 0: ptx_iterate traces the next batch of iterations in the background (other streams,
 * per-iteration radiance buffers) and each call adds exactly its own iteration to the image, so what every call returns
 * -- image, statistics, preview -- is unchanged bit for bit, at the cost per iteration of ptx_render.  A camera change,
 * a jump in iter or any other render call simply drops what was traced ahead.  Off by default in this ABI; the C++ veneer
 * (pathtrace_api.h) switches it on.  Needs the default launch-set layout (lanes >= 3, batch > 1); otherwise it is a no-op. */
int ptx_set_render_ahead(ptx_tracer *t, int on);
/* iterations iter_first .. iter_first+count-1 back to back, no host round trip in between */
int ptx_render(ptx_tracer *t, int iter_first, int count);
/* iterations iter_first, iter_first+stride, ... (count of them): N ranks that take turns over the iterations of one
 * full frame (rank r: iter_first = r+1, stride = N) and sum their buffers reproduce the single-GPU frame, which
 * pixel-row tiles cannot (the shading RNG is seeded by stream position) */
int ptx_render_strided(ptx_tracer *t, int iter_first, int count, int stride);
int ptx_synchronize(ptx_tracer *t);

int ptx_read_image(ptx_tracer *t, float *host_rgb);     /* W*H*3 floats = sum over iterations (state.image) */
int ptx_write_image(ptx_tracer *t, const float *host_rgb);  /* the reverse: resume from a saved accumulation buffer   */
int ptx_read_albedo(ptx_tracer *t, float *host_rgb);    /* RenderState.albedo of apps/src (apps_variant only)  */
/* sendToGPU, apps/src/pathtrace.h:10: a finished (e.g. denoised) host frame -> 8-bit preview, no division by iter */
int ptx_write_denoised_pbo(ptx_tracer *t, const float *host_rgb, uint8_t *host_rgba);
int ptx_write_denoised_pbo_device(ptx_tracer *t, const float *host_rgb, void *device_uchar4);   /* pbo in device memory, as the reference's */
float *ptx_device_image(ptx_tracer *t);                 /* device pointer of the accumulation buffer        */
int ptx_write_pbo(ptx_tracer *t, int iter, uint8_t *host_rgba);          /* sendImageToPBO, pathtrace.cu:69 */
int ptx_write_pbo_device(ptx_tracer *t, int iter, void *device_uchar4);
double ptx_last_loop_ms(ptx_tracer *t);                 /* timer(): bounce loop of the last iteration       */
int ptx_get_stats(ptx_tracer *t, ptx_stats *out);
/* the same, writing at most out_bytes of the struct (a caller compiled against an older, shorter ptx_stats passes ITS sizeof;
 * fields past the library's own struct are zeroed) */
int ptx_get_stats_sized(ptx_tracer *t, void *out, size_t out_bytes);
int ptx_owned_pixels(const ptx_tracer *t);              /* pixels this tracer generates (tile split)        */
void *ptx_stream(ptx_tracer *t);
/* ---- N GPUs of one node, one process (csrc/pt_multi.cpp) ---------------------------------------------------------
 * No reference counterpart: the reference drives device 0 only (src/preview.cpp:107).  A main.cpp-shaped caller
 * (src/main.cpp:128-148) uses these instead of ptx_create / ptx_iterate / ptx_read_image: device i of n traces the
 * interleaved row blocks (y / tile_rows) % n == i as a stream of its own; ptx_multi_assemble copies every device's row
 * blocks into device[0]'s frame (one strided peer copy per device over xGMI), ptx_multi_read_image = assemble + read.
 * `devices` may name one ordinal more than once (two tiles on one GPU: how the one-GPU tests exercise it).
 * tile_rows <= 0 = 8.  Each tile equals the reference's algorithm run on that tile. */
typedef struct ptx_multi ptx_multi;
int ptx_multi_create(const ptx_scene *s, const ptx_options *options, const int *devices, int ndevices, int tile_rows, ptx_multi **out);
void ptx_multi_destroy(ptx_multi *m);
int ptx_multi_device_count(const ptx_multi *m);
ptx_tracer *ptx_multi_tracer(ptx_multi *m, int i);            /* device i's tracer (statistics, kernel timing, ...) */
int ptx_multi_set_camera(ptx_multi *m, const ptx_camera *camera, int trace_depth);
int ptx_multi_reset_image(ptx_multi *m);
int ptx_multi_iterate(ptx_multi *m, int iter);                /* pathtrace(iter) on every device's tile; enqueues, returns */
int ptx_multi_set_render_ahead(ptx_multi *m, int on);
int ptx_multi_render(ptx_multi *m, int iter_first, int count);
int ptx_multi_synchronize(ptx_multi *m);
int ptx_multi_assemble(ptx_multi *m);                         /* owned row blocks -> device[0]'s frame; waits for them */
float *ptx_multi_device_image(ptx_multi *m);                  /* device[0]'s frame (complete after ptx_multi_assemble) */
int ptx_multi_read_image(ptx_multi *m, float *host_rgb);      /* assemble + W*H*3 floats to the host */
int ptx_multi_read_albedo(ptx_multi *m, float *host_rgb);     /* apps_variant: the devices' rows of the albedo AOV, merged */
int ptx_multi_get_stats(ptx_multi *m, ptx_stats *out);        /* rays summed over the devices */
/* Page-lock / release a caller-owned host buffer (the reference's scene->state.image: the destination of its per-iteration
 * read-back, src/pathtrace.cu:555-556), so that ptx_read_image / ptx_multi_read_image into it are direct DMA. */
int ptx_pin_host_buffer(void *p, size_t bytes);
int ptx_unpin_host_buffer(void *p);

/* Optional per-kernel device timing (hipEvents on the tracer's stream around every launch while on).
 * kinds: 0 = k_bounce<first> (ray generation + intersect), 1 = k_bounce (shade + intersect), 2 = k_mesh + k_finish (split mesh search only: the search of the parked rays' meshes and their
 * finishing, one bracket around both launches), 3 = pass 2 of the split bounce (the ranking pass after k_mesh, first and later bounces; 0 for scenes without the split: kinds 0 / 1 are then the whole bounce,
 * with the split they are its pass 1).
 * ptx_get_kernel_times returns the sums since it was last called and clears them. */
int ptx_set_kernel_timing(ptx_tracer *t, int on);
int ptx_get_kernel_times(ptx_tracer *t, double ms_by_kind[4], int64_t launches_by_kind[4]);

/* ---- denoiser: edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) on the device, csrc/pt_denoise.hip -------------
 * The GPU counterpart of the OIDN step of apps/src/main.cpp:167-219 (colour + albedo in, state.output out).  Guide images come from a
 * G-buffer pass through the same intersection as the path, giving per pixel hit flag, world position o + t*d, shading normal
 * (bump-mapped where the path's is), albedo (the apps-variant AOV's rule) and material / geom ids.  Two modes (ptx_set_guide_samples):
 *   pixel-centre guides (the default): one pixel-centre pinhole ray per pixel, no antialiasing jitter, no depth of field -- with DoF
 *   on, the guides are the sharp pinhole view while the colour is not;
 *   sampled guides (count = K >= 1): the average over the camera rays of iterations iter_first .. iter_first + K - 1 exactly as the
 *   path kernels generate them, jitter and lens included (a camera ray is a pure function of iteration, pixel and trace depth), so
 *   the guides are as soft as the colour they guide.  Of the H samples that hit: normal = sum n / H (NOT renormalised: a crease or a
 *   blurred silhouette gives a shorter normal), position = sum (o + t*d) / H, t = sum t / H, ids = the first hit sample's, hit = 1;
 *   albedo = sum albedo / K and coverage = H / K (coverage-weighted as the colour is: a miss deposits nothing).  H = 0: a miss, all
 *   zeros.  The sums begin with the first hit sample and add in iteration order, fp32, no contraction, IEEE division: with
 *   antialiasing = depth_of_field = 0 and K = 1 this is the pixel-centre record bit for bit.
 * Either is computed on the tracer's stream on the first ptx_denoise* / ptx_read_gbuffer after ptx_create, after a ptx_set_camera that
 * changed the camera or the trace depth (the rays' seed depends on it), or after a ptx_set_guide_samples that changed the mode, into
 * buffers allocated on that first use.
 *
 * The filter, exactly (tests/atrous_ref.py restates it):
 *   c = rgb / spp per channel (mean radiance); demodulate: c / max(albedo, 1e-3) per channel on hit pixels.
 *   pass i = 0 .. passes-1, step s = 2^i, for every hit pixel p:
 *     out_p = sum_q w_q c_q / sum_q w_q over the 5x5 taps q = clamp_to_frame(p + s*(dx, dy)), dx, dy in -2..2, miss taps excluded,
 *     w_q = b[dx] b[dy] exp(-|c_p - c_q|^2 / (phi_color * 2^-i)) exp(-(|n_p - n_q|^2 / s^2) / phi_normal) exp(-|x_p - x_q|^2 / phi_position),
 *     b = (1/16, 1/4, 3/8, 1/4, 1/16).  The centre tap weighs 9/64, so the sum is never 0.  Miss pixels keep c in every pass.
 *   result = the last pass, multiplied back by max(albedo, 1e-3) on hit pixels when demodulating: W*H*3 fp32 mean radiance (what
 *   RenderState.output holds in apps/src, so ptx_write_denoised_pbo* / sendToGPU take it without dividing by the iteration count).
 * ptx_multi_* has no denoiser; a tracer that renders a row tile (tile_world > 1) is refused: its frame holds only its own rows. */
typedef struct ptx_denoise_params {
    int32_t passes;          /* 1 .. 10; default 5 (steps 1, 2, 4, 8, 16: a 125-pixel footprint)                            */
    int32_t demodulate;      /* != 0: filter colour / albedo (texture detail survives); default 1                              */
    float phi_color;         /* > 0, squared mean-radiance units, halved every pass; see DESIGN.md 10 for the chosen defaults  */
    float phi_normal;        /* > 0, squared unit-normal difference per squared step                                          */
    float phi_position;      /* > 0, squared scene units (the Cornell scenes are about 10 units across)                       */
} ptx_denoise_params;
void ptx_default_denoise_params(ptx_denoise_params *p);
size_t ptx_sizeof_denoise_params(void);
/* Enqueues G-buffer (when stale) + filter of the accumulation buffer / spp on the tracer's stream and returns; p NULL = defaults.
 * The accumulation buffer, statistics and what later iterations compute are untouched. */
int ptx_denoise(ptx_tracer *t, const ptx_denoise_params *p, int spp);
int ptx_read_denoised(ptx_tracer *t, float *host_rgb);                  /* W*H*3 mean radiance of the last ptx_denoise (waits for it) */
float *ptx_device_denoised(ptx_tracer *t);                               /* device pointer of that frame; NULL before the first denoise */
int ptx_write_denoised_pbo_from_device(ptx_tracer *t, void *device_uchar4);   /* sendToGPU of that frame without a host round trip (enqueues) */
/* The G-buffer as the last ptx_denoise used it (computed now if stale): W*H*3 floats each of position, normal, albedo, W*H*2 int32
 * (material id, geom id), W*H floats of t and W*H bytes of hit flag; any pointer may be NULL.  Misses read as zeros. */
int ptx_read_gbuffer(ptx_tracer *t, float *pos3, float *nrm3, float *alb3, int32_t *ids2, float *t1, uint8_t *hit1);
/* count = 0 (the default): pixel-centre guides, today's behaviour exactly.  count >= 1: sampled guides over
 * iterations iter_first .. iter_first+count-1.  Marks the G-buffer stale; the next denoise / read recomputes it.
 * PTX_ERR_INVALID: iter_first < 1, count < 0, count > 4096 (the cap: the pass costs about count pixel-centre passes), a row-tile tracer
 * (tile_world > 1).  count may exceed the spp of the denoise call: the guides are an independent estimate of the same expectation.
 * While count > 0, ptx_denoise_temporal and ptx_denoise_variance / ptx_denoise_temporal_measured with a history handle return
 * PTX_ERR_UNSUPPORTED: reprojection and history matching need one surface per pixel.  ptx_denoise, ptx_denoise_variance without a
 * handle, ptx_denoise_measured and ptx_denoise_adaptive take the sampled guides as they take the others.  On an adaptive frame, whose
 * tiles hold different sample counts, the albedo's coverage equals the colour's only in expectation (on a uniform frame with
 * iter_first = 1 and count = spp they are the same rays). */
int ptx_set_guide_samples(ptx_tracer *t, int iter_first, int count);
int ptx_get_guide_samples(const ptx_tracer *t, int *iter_first, int *count);
int ptx_read_guide_coverage(ptx_tracer *t, float *coverage1);   /* W*H floats, H/K (pixel-centre guides: the hit flag); computed now if stale */
/* Guides through mirrors and glass.  bounces = 0 (the default): the guides describe the first surface a guide ray hits, today's
 * behaviour exactly.  bounces = B >= 1: every guide ray -- the pixel-centre ray, or each of the count rays of ptx_set_guide_samples --
 * is followed through perfectly specular surfaces, at most min(B, trace depth - 1) times, and the surface seen at the end of the
 * chain is recorded in place of the first hit (for a perfect mirror, what OIDN asks its callers for: albedo and normal of the first
 * non-specular hit).  A hit is followed when its geom is not an OBJ mesh, its material has emittance <= 0 and hasReflective > 0 or
 * else hasRefractive > 0; the ray is continued by the deterministic parts of the path's own scatterRay: the reflective branch whole,
 * the refractive branch with its random draw taken as "not reflected" (refract, unless the branch's total-internal-reflection test
 * reflects), fp32, no contraction.  The chain ends on a hit that is not followed, on the budget, or on a continued ray that misses;
 * the recorded surface is the last one hit (after such a miss: the specular surface the ray left).  Per ray: normal and ids of the
 * recorded surface, position = o + t*d of its own segment, t = the segments' t summed in order, albedo = T x albedo of the recorded
 * hit, T = the product of the colour factors of the surfaces the ray was followed through (1 when none).  The samples are averaged
 * as ptx_set_guide_samples states.  A pixel none of whose rays is followed gets the record of bounces = 0 bit for bit.
 * Changing the value marks the G-buffer stale (setting the same value does not).  PTX_ERR_INVALID: bounces < 0, bounces > 64, a
 * row-tile tracer.  While bounces > 0 the calls that take a temporal history return PTX_ERR_UNSUPPORTED, as with sampled guides:
 * reprojection needs the first surface.  The reflected branch of glass is not followed. */
int ptx_set_guide_bounces(ptx_tracer *t, int bounces);
int ptx_get_guide_bounces(const ptx_tracer *t, int *bounces);
/* The filter alone over caller-owned host buffers (W*H*3 floats; hit W*H bytes, != 0 = hit): rgb is mean radiance (spp = 1), out_rgb
 * receives the result.  alb3 may be NULL when p->demodulate is 0.  Runs on `device`, synchronously; PTX_ERR_NODEVICE without one. */
int ptx_denoise_buffers(int device, int w, int h, const float *rgb, const float *alb3, const float *nrm3, const float *pos3,
                        const uint8_t *hit, const ptx_denoise_params *p, float *out_rgb);

/* ---- temporal reuse in front of the denoiser (in the spirit of SVGF, Schied et al., HPG 2017), csrc/pt_temporal.hip -----------------
 * The previous view's result, reprojected through the G-buffer into the current view, blended with the current accumulation by sample
 * count, then the a-trous filter above.  The history lives in a handle of its own, so it outlives the tracer: the reference's loop
 * (apps/src/main.cpp:221-271) destroys and recreates the tracer on every camera change.  Definition (tests/temporal_ref.py
 * restates it):
 *   State: the camera (ptx_camera floats) and per pixel hit flag, world position, normal, geom id, material id (copied from the tracer's
 *   G-buffer), D = mix / max(albedo, 1e-3) per channel on hit pixels (mix on miss pixels) and a float sample count n.  The handle keeps
 *   `cur` (the state of its last call) and `hist` (the committed history).
 *   Segments: each ptx_denoise_temporal compares the tracer's camera bit for bit with cur's.  Different: cur becomes hist and a new cur
 *   starts.  Equal: the same segment -- cur is recomputed from the same hist and the tracer's current accumulation, so no sample is
 *   counted twice (ptx_reset_image with the same camera included).  The first call, and the first after ptx_temporal_reset, has no hist.
 *   Reprojection, every hit pixel p (position x_p, normal n_p, ids, albedo a_p), P = hist's camera: solve
 *     x_p - P.position = s * (view - right*pl.x*(u - W/2) - up*pl.y*(v - H/2))        (generateRay's pixel-centre ray, unnormalised)
 *   for (s, u, v) as a 3x3 linear system in (s, s*u, s*v) (right and up need not be orthonormal).  s <= 0: nothing.  Pixel centres are
 *   at integer (u, v); the bilinear taps (floor(u) + i, floor(v) + j), i, j in {0, 1}, of non-zero weight w_q are accepted when inside
 *   the frame, a hit in hist, of the same geom and material id, dot(n_p, n_q) >= normal_cos and |dot(n_p, x_q - x_p)| <=
 *   plane_tolerance * |x_p - P.position|.  With specular_history == 0 a pixel whose material has hasReflective > 0 or hasRefractive > 0
 *   accepts nothing.  Sum of accepted weights S > 0: n_h = min(sum w_q n_q / S, max_history), and when n_h > 0
 *   h = sum w_q D_q / S * max(a_p, 1e-3) per channel; otherwise n_h = 0 and h = 0.
 *   Mix: c = rgb / spp (the fp32 division of ptx_denoise).  Miss pixel or n_h == 0: mix = c exactly, n = spp.  Otherwise
 *   mix = (spp*c + n_h*h) / (spp + n_h), n = spp + n_h.
 *   Output: the a-trous filter of mix (spp = 1) with the tracer's G-buffer, into the tracer's denoised frame (ptx_read_denoised,
 *   ptx_device_denoised, ptx_write_denoised_pbo_from_device take it).  Without hist, or with max_history == 0, that is bit for bit
 *   ptx_denoise.
 * A handle serves one W x H on one device, across tracers and streams: each call makes the tracer's stream wait for the handle's
 * previous work and records an event after its own. */
typedef struct ptx_temporal ptx_temporal;          /* opaque: history of one W x H view sequence on one device */
typedef struct ptx_temporal_params {
    int32_t max_history;       /* samples a pixel may inherit; 0 = no reuse (== ptx_denoise); default 16 */
    int32_t specular_history;  /* 0 = reflective / refractive materials inherit nothing (default)        */
    float   normal_cos;        /* default 0.9                                                            */
    float   plane_tolerance;   /* relative to the distance from the previous camera; default 0.01        */
} ptx_temporal_params;
void   ptx_default_temporal_params(ptx_temporal_params *p);
size_t ptx_sizeof_temporal_params(void);
int  ptx_temporal_create(int device, int width, int height, ptx_temporal **out);   /* PTX_ERR_NODEVICE without a device */
void ptx_temporal_destroy(ptx_temporal *h);        /* NULL is a no-op; waits for its last use */
int  ptx_temporal_reset(ptx_temporal *h);          /* forget all history */
/* Enqueues G-buffer (when stale) + reprojection + mix + filter on the tracer's stream; dp / tp NULL = defaults.  The accumulation buffer,
 * statistics and what later iterations compute are untouched.  Refused: a handle of another device or size, tile_world > 1, spp < 1. */
int  ptx_denoise_temporal(ptx_tracer *t, ptx_temporal *h, const ptx_denoise_params *dp, const ptx_temporal_params *tp, int spp);
int  ptx_temporal_read(ptx_temporal *h, float *hist_rgb3, float *hist_count1, float *mix_rgb3);   /* last call's h, n_h, mix; NULLs allowed; waits */

/* ---- variance guidance of the a-trous filter (the middle of SVGF, Schied et al., HPG 2017), csrc/pt_denoise.hip ----------------------
 * A per-pixel estimate of the variance of the filter's input replaces the fixed phi_color: the colour weight becomes a luminance weight
 * normalised by the local standard deviation, and the variance is filtered along.  Definition (tests/variance_ref.py
 * restates it).  l(c) = 0.2126 r + 0.7152 g + 0.0722 b; every variance is one of the luminance of the filter's input in the filter's
 * colour space (demodulated by max(albedo, 1e-3) when demodulate != 0).
 *   Stored per pixel: V, an estimate of the PER-SAMPLE luminance variance (the variance of a mean of n samples is V / n), in the fourth
 *   float of the temporal state's D record; the handle remembers per state whether that float holds a V (ptx_denoise_temporal writes 0
 *   there and marks the state as carrying none).
 *   Spatial estimate var_s(p) of a hit pixel: over the (2r+1)^2 window (r = spatial_radius, taps clamped to the frame), weights
 *   w_q = exp(-|n_p - n_q|^2 / phi_normal) exp(-|x_p - x_q|^2 / phi_position) for hit taps of the same geom and material id, else 0:
 *   lbar = sum w l_q / sum w, var_s = sum w (l_q - lbar)^2 / sum w.  Miss pixels: 0.
 *   Without history (no handle, no hist, n_h == 0, or a hist without V): V = n * var_s(l(mix)), n the pixel's sample count.
 *   With history (taps, weights w, accepted sum S, n_h of ptx_denoise_temporal): V_h = sum w V_q / S, mu_h = l(sum w D_q / S),
 *   l_c = l(c / a): e = (l_c - mu_h)^2 * n_h * spp / (n_h + spp), V = (n_h * V_h + spp * e) / (n_h + spp).
 *   The filter's input variance is v0 = V / n.  Pass i, step s = 2^i, hit pixel p, colour c and variance v of the previous pass:
 *     g_p = 3x3 Gaussian (1/4, 1/2, 1/4 per axis, neighbours at distance 1, clamped to the frame) of v over hit taps, renormalised over
 *           the taps used (prefilter == 0: g_p = v_p),
 *     w_q = b[dx] b[dy] exp(-|l(c_p) - l(c_q)| / (phi_luminance * sqrt(g_p) + epsilon)) * (normal term) * (position term of ptx_denoise),
 *     c_out = sum w c_q / sum w, v_out = sum w^2 v_q / (sum w)^2.  Miss pixels keep c, with v = 0.  phi_color is not used.
 *   Result: as ptx_denoise, into the tracer's denoised frame. */
typedef struct ptx_variance_params {
    float   phi_luminance;     /* > 0, in standard deviations of the filtered luminance; default 4   */
    float   epsilon;           /* > 0, added to phi_luminance * sigma; default 1e-4                                  */
    int32_t spatial_radius;    /* 1 .. 3: the spatial estimate's window is (2r+1)^2; default 3                      */
    int32_t prefilter;         /* != 0: 3x3 Gaussian of the variance before it normalises the weight; default 1     */
} ptx_variance_params;
void   ptx_default_variance_params(ptx_variance_params *p);
size_t ptx_sizeof_variance_params(void);
/* ptx_denoise (h NULL) or ptx_denoise_temporal (h a handle) with the variance-guided filter; dp / tp / vp NULL = defaults.  Refused
 * like those, and with a handle when dp->demodulate == 0: the state's moments are in demodulated space.  A handle may be used by
 * ptx_denoise_temporal and ptx_denoise_variance in any order; after the former the next call here takes the spatial estimate. */
int  ptx_denoise_variance(ptx_tracer *t, ptx_temporal *h, const ptx_denoise_params *dp, const ptx_temporal_params *tp,
                          const ptx_variance_params *vp, int spp);
/* v0 and the last pass's v of the last ptx_denoise_variance, W*H floats each; NULLs allowed; waits */
int  ptx_read_variance(ptx_tracer *t, float *input_var1, float *output_var1);
/* The variance-guided filter alone over host buffers (as ptx_denoise_buffers): ids2 = W*H*2 int32 (material, geom), NULL = the spatial
 * estimate skips its id test; var1 = W*H floats of v0 (negative values read as 0), NULL = the spatial estimate with n = 1; out_var1
 * (W*H floats, may be NULL) receives the last pass's v. */
int  ptx_denoise_buffers_variance(int device, int w, int h, const float *rgb, const float *alb3, const float *nrm3, const float *pos3,
                                  const uint8_t *hit, const int32_t *ids2, const float *var1, const ptx_denoise_params *dp,
                                  const ptx_variance_params *vp, float *out_rgb, float *out_var1);

/* ---- sample moments by batch means: error estimate, stop rule, measured variance for the filter, csrc/pt_moments.hip ----------------
 * The per-sample covariance of every pixel's radiance, estimated from the accumulation buffer alone: no rendering kernel is involved.
 * Whenever the caller says "N samples are in the buffer now" (ptx_moments_add), the difference to the snapshot the handle kept is the
 * sum of one batch; the batch mean is folded into running moments and the snapshot is replaced.  Batches of iid samples give an
 * unbiased estimate of the per-sample covariance whatever their sizes.  Definition (tests/moments_ref.py restates it):
 *   State per pixel (56 B): snap = accumulation rgb at the last add and W, the samples it held; mean = the weighted mean rgb of the
 *   batch means and the batch count B; M = the upper triangle (rr, gg, bb, rg, rb, gb) of the weighted scatter matrix.  All zero after
 *   create and reset, so the first add takes everything in the buffer as one batch.
 *   Add with samples_total = N > W: k = N - W, x = (acc - snap) / k per channel, then West's weighted update
 *     W' = W + k, d = x - mean, mean' = mean + (k / W') d, M' = M + k d (x - mean')^T, B' = B + 1, snap' = (acc, N).
 *   (mean = snap / W and x - mean' = (W / W') d, so d = D / (k W) with D = W acc - W' snap and the scatter term is D D^T / (k W W'): the
 *   device evaluates it in that form, D from exact fp32 products, so that a batch mean close to the running mean costs no precision.)
 *   B >= 2: the per-sample covariance estimate is C = M / (B - 1), and the variance of the frame's mean of a linear functional g of
 *   the colour is g^T C g / W.  B < 2: no estimate (ptx_moments_read gives C = 0).
 *   Summary (ptx_moments_summarize), over the pixels with B >= 2, g = Rec. 709 (l above): q = max(g^T C g, 0), se = sqrt(q / W),
 *   rel = se / max(l(mean), floor).  Reduced on the device in two stages of fixed order without float atomics: the same bits on
 *   every run.
 *   Measured variance for the filter (ptx_denoise_measured): ptx_denoise_variance without a handle, whose v0 on a hit pixel with
 *   B >= min_batches is max(g^T C g, 0) / W, g_k = l_k / max(albedo_k, 1e-3) when demodulating, else g_k = l_k (l_k the Rec. 709
 *   weights): the exact variance of the demodulated luminance, which is why the state is a covariance and not a scalar.  Hit pixels
 *   with B < min_batches take the spatial estimate of ptx_denoise_variance; miss pixels 0.  The colour is rgb / spp as in ptx_denoise;
 *   W is the handle's, so samples rendered after the last add make v0 conservative, never too small.
 * Precision: everything is fp32.  acc - snap is exact or correctly rounded, but acc itself carries ulp(acc) / 2 per gather, so a batch
 * mean carries about ulp(acc) / k = 2^-23 N / k of the pixel's mean in rounding noise, against a sampling noise of sigma / sqrt(k):
 * negligible (below 1 % of the batch's standard deviation for sigma >= the mean / 10) below about 10^5 samples per pixel with batches
 * of at least 8.  W, k and B are held as floats, exact to 2^24: an add whose samples_total exceeds 2^24 is refused on every path
 * (above it W' rounds, and an error of 1 in W' shifts D = W acc - W' snap by acc, as much as D itself once sigma / mean nears
 * sqrt(k / W)).  Up to there the state stays within (B + 8) 2^-23 sqrt(C_ii C_jj) per covariance entry and (B + 2) 2^-23 |mean| per
 * channel of the float64 definition fed the same buffers, however small the noise (tests/test_gpu_moments_grid.py).
 * The handle never looks at what the buffer holds: after ptx_reset_image (or ptx_write_image, or a camera change that restarts the
 * accumulation) the caller MUST call ptx_moments_reset before the next add, or that add's batch is the difference of two unrelated
 * frames.  A handle serves one W x H on one device, across tracers and streams, like ptx_temporal: each enqueueing call makes the
 * tracer's stream wait for the handle's previous work and records an event after its own. */
typedef struct ptx_moments ptx_moments;            /* opaque */
typedef struct ptx_moments_params {
    float floor;               /* > 0: rel = se / max(l(mean), floor); default 0.05 (stated, not tuned) */
    float threshold;           /* >= 0: pixels with rel > threshold are counted; default 0.05 (stated, not tuned) */
} ptx_moments_params;
typedef struct ptx_moments_summary {
    int64_t pixels;            /* pixels with B >= 2 (0: every other field but samples and batches is 0) */
    int64_t pixels_over;       /* of those, rel > threshold */
    int64_t samples;           /* W: samples_total of the last add */
    double  mean_rel_se;       /* mean, root mean square and maximum of rel */
    double  rms_rel_se;
    double  max_rel_se;
    double  mean_variance;     /* mean of q = g^T C g, the per-sample luminance variance */
    int32_t batches;           /* B: adds since create / reset */
    int32_t reserved;
} ptx_moments_summary;
void   ptx_default_moments_params(ptx_moments_params *p);
size_t ptx_sizeof_moments_params(void);
size_t ptx_sizeof_moments_summary(void);
int  ptx_moments_create(int device, int width, int height, ptx_moments **out);     /* PTX_ERR_NODEVICE without a device */
void ptx_moments_destroy(ptx_moments *m);          /* NULL is a no-op; waits for its last use */
int  ptx_moments_reset(ptx_moments *m);            /* forget everything: required after ptx_reset_image (see above) */
/* Enqueues one add on t's stream, ordered after every iteration rendered so far (render-ahead included: an iteration is in the buffer
 * once its ptx_iterate / ptx_render returned, exactly what ptx_denoise reads).  The accumulation buffer, statistics and what later
 * iterations compute are untouched.  Refused (PTX_ERR_INVALID, nothing enqueued): samples_total <= the last add's, samples_total >
 * 2^24 (before any device call; the message names the value), a handle of another device or size, tile_world > 1. */
int  ptx_moments_add(ptx_moments *m, ptx_tracer *t, int64_t samples_total);
/* The same from a host frame (W*H*3 floats, a sum of samples_total samples, e.g. after ptx_multi_read_image), through a staging buffer
 * the handle owns; synchronous.  samples_total > 2^24 is refused in the same way. */
int  ptx_moments_add_host(ptx_moments *m, const float *host_rgb_sum, int64_t samples_total);
/* The add in which tiles advance by different amounts (adaptive sampling below; multi-device callers): tile_samples_total[tile] = the
 * samples tile's pixels hold now, tile = (y * W + x) / ptx_tile_pixels(), ntiles = ceil(W * H / ptx_tile_pixels()).  The same update
 * per pixel with its tile's k and W'.  A tile whose total equals its last one is idle: its pixels keep their state bit for bit (zeros
 * on a fresh handle), W and B included, so ptx_moments_read and ptx_moments_summarize, which use the per-pixel W and B, need nothing
 * new.  Refused (PTX_ERR_INVALID): a total below the tile's last one, a wrong ntiles.  From its first tiled add until ptx_moments_reset
 * the handle's `samples` and `batches` are the maxima over the tiles, ptx_moments_add and ptx_moments_add_host are refused, and so are
 * ptx_denoise_measured and ptx_denoise_temporal_measured, which assume one spp and one B for the frame: the filter on an adaptive
 * frame is ptx_denoise_adaptive below, which takes both per tile.  Synchronous. */
int  ptx_moments_add_host_tiled(ptx_moments *m, const float *host_rgb_sum, const int64_t *tile_samples_total, int ntiles);
/* samples1: W*H int32 of the per-pixel W (one number per frame until a tiled add); waits for the handle's last work. */
int  ptx_moments_read_samples(ptx_moments *m, int32_t *samples1);
/* mean3: W*H*3 floats; cov6: W*H*6 floats of C (rr, gg, bb, rg, rb, gb), 0 where B < 2; batches1: W*H int32 of B; samples_out: W.
 * NULLs allowed; waits for the handle's last work. */
int  ptx_moments_read(ptx_moments *m, float *mean3, float *cov6, int32_t *batches1, int64_t *samples_out);
int  ptx_moments_summarize(ptx_moments *m, const ptx_moments_params *p, ptx_moments_summary *out);   /* p NULL = defaults; waits */
/* ptx_denoise_variance(t, NULL, ...) with the measured v0 above; min_batches <= 0 means 4, 1 is refused (C needs B >= 2).  The result
 * goes into the tracer's denoised frame and ptx_read_variance.  Refused like ptx_denoise_variance and ptx_moments_add, and before the
 * handle's first add. */
int  ptx_denoise_measured(ptx_tracer *t, ptx_moments *m, const ptx_denoise_params *dp, const ptx_variance_params *vp, int min_batches,
                          int spp);
/* ---- the temporal history and the measured variance together, csrc/pt_temporal.hip (k_reproject_measured) ---------------------------
 * ptx_denoise_variance(t, h, dp, tp, vp, spp) with one change: the V written into the state for a hit pixel.  Taps, acceptance tests,
 * n_h, h, mix, n, the segment rule, the state layout, the filter and the outputs (ptx_read_denoised, ptx_read_variance,
 * ptx_temporal_read) are that call's.  Definition (tests/temporal_measured_ref.py restates it):
 *   B = the moments handle's batch count (one number per handle: every add touches every pixel), min_batches <= 0 means 4, 1 is refused.
 *   B < min_batches: the call IS ptx_denoise_variance(t, h, ...), decided on the host: the same kernels, the same bits; the moments
 *   state is not read.
 *   B >= min_batches: q = max(g^T M g / (B - 1), 0), g_k = l_k / max(albedo_k, 1e-3): the per-sample variance of the demodulated
 *   luminance as ptx_denoise_measured takes it, an estimate with B - 1 degrees of freedom.
 *     A pixel that inherits a V (hist valid, hist carries V, n_h > 0), with e, V_h, mu_h of ptx_denoise_variance (their bilinear
 *     weights, and only theirs, from the projection evaluated in double: a measured V differs so much between neighbouring pixels that
 *     an fp32 ulp of u is up to 2 % of V_h; taps, n_h, h and mix keep the fp32 weights and that call's bits): e estimates the same
 *     per-sample variance with one degree of freedom, so the current view's share is the two pooled by degrees of freedom,
 *       V_c = ((B - 1) q + e) / B,   V = (n_h V_h + spp V_c) / (n_h + spp)       (ptx_denoise_variance: V_c = e).
 *     Every other hit pixel (no hist, a hist without V, n_h == 0, a specular pixel with specular_history == 0): V = q, where
 *     ptx_denoise_variance writes -1 for its spatial estimate; so no spatial estimate is taken anywhere.  Miss pixels: 0.
 *   v0 = V / n as there, and the state is marked as carrying V: ptx_denoise_variance and this call share a handle in any order.
 * Refused, with nothing enqueued: everything ptx_denoise_variance refuses with a handle (demodulate == 0 included) and everything
 * ptx_denoise_measured refuses (a NULL handle, no add yet, another device or size, tile_world > 1, min_batches == 1).  Both handles'
 * events are waited for and recorded.  The moments handle's W is not compared with spp (as in ptx_denoise_measured: q is per sample).
 * The caller resets the moments handle (ptx_moments_reset) whenever the accumulation restarts -- at every camera change in particular,
 * so that q describes the current view's samples alone -- exactly as for ptx_denoise_measured; the temporal handle is NOT reset there. */
int  ptx_denoise_temporal_measured(ptx_tracer *t, ptx_temporal *h, ptx_moments *m, const ptx_denoise_params *dp,
                                   const ptx_temporal_params *tp, const ptx_variance_params *vp, int min_batches, int spp);

/* ---- adaptive sampling by tiles: stop tracing the tiles whose measured error is low, csrc/pt_adaptive.hip ---------------------------
 * The loop is render k iterations -> ptx_adaptive_add -> ptx_adaptive_select, until no tile is active; ptx_adaptive_resolve then
 * gives the frame.  The handle holds, per tile (ptx_tile_pixels() pixels, as the active-tile mask above), the samples its pixels
 * hold, its batches, whether it is active, and its last error; and one W x H x 3 frame.  After create and reset every tile is active
 * with 0 samples.  Definition (tests/adaptive_ref.py restates it):
 *   ptx_adaptive_add(a, m, t, k) = "the last k iterations were rendered under the current mask": every active tile's samples += k and
 *   batches += 1, then the tiled moments add (ptx_moments_add_host_tiled's update) on t's accumulation buffer with these totals,
 *   ordered as ptx_moments_add is.  The first call finds every tile active, so it is exact for a frame rendered without a mask.
 *   ptx_adaptive_select: per pixel with B >= 2, rel = sqrt(max(g^T C g, 0) / W) / max(l(mean), floor) -- ptx_moments_summarize's, g =
 *   Rec. 709.  Tile error e_T = sqrt(sum rel^2 / n_T), n_T = the tile's pixels inside the frame; sums in double through a tree of fixed
 *   shape, no float atomics: the same bits on every run.  A tile none of whose pixels has B >= 2 has no estimate (e_T reads 0).
 *     active_T = samples_T < max_samples && (batches_T < min_batches || e_T > target)
 *   The flags then become t's mask without leaving the device (ptx_set_active_tiles' ordering and refusals), and the status comes back
 *   with them in one small read.  Counts are reduced in integers: exact.  A stopped tile receives no samples, so its error does not
 *   change: it stays stopped under the same parameters.
 *   ptx_adaptive_resolve: frame[p] = acc[p] / samples[tile(p)] in fp32, the mean radiance; 0 where the tile has no sample.
 * The handle and the moments handle count the same samples: reset both together (and ptx_clear_active_tiles the tracer) whenever the
 * accumulation restarts; an add that finds them out of step is refused.  Refused like ptx_moments_add: a handle of another device or
 * size, tile_world > 1.  Each enqueueing call makes t's stream wait for both handles' previous work and records after its own.
 * Not done: reactivating a stopped tile on purpose, masks finer than a tile, multi-device tracers. */
typedef struct ptx_adaptive ptx_adaptive;          /* opaque */
typedef struct ptx_adaptive_params {
    float   target;            /* > 0: a tile stops when its error <= target; default 0.02 (stated, not tuned) */
    float   floor;             /* as ptx_moments_params.floor; default 0.05 */
    int32_t min_batches;       /* >= 2: a tile stays active until it has this many batches; default 4 */
    int32_t max_samples;       /* > 0: a tile stops at this many samples whatever its error; default 1 << 20 */
} ptx_adaptive_params;
typedef struct ptx_adaptive_status {
    int64_t samples_total;     /* sum over tiles of samples_T * n_T: the pixel-samples the frame holds */
    int64_t pixels_active;     /* pixels of the active tiles */
    int32_t tiles, tiles_active;
    int32_t samples_min, samples_max;      /* over all tiles */
    float   worst_error;       /* largest e_T over the tiles with an estimate (0: none has one) */
    int32_t rounds;            /* selects since create / reset, this one included */
} ptx_adaptive_status;
void   ptx_default_adaptive_params(ptx_adaptive_params *p);
size_t ptx_sizeof_adaptive_params(void);
size_t ptx_sizeof_adaptive_status(void);
int  ptx_adaptive_create(int device, int width, int height, ptx_adaptive **out);   /* PTX_ERR_NODEVICE without a device */
void ptx_adaptive_destroy(ptx_adaptive *a);        /* NULL is a no-op; waits for its last use */
int  ptx_adaptive_reset(ptx_adaptive *a);          /* as after create; waits */
int  ptx_adaptive_num_tiles(const ptx_adaptive *a);
int  ptx_adaptive_add(ptx_adaptive *a, ptx_moments *m, ptx_tracer *t, int k);
int  ptx_adaptive_select(ptx_adaptive *a, ptx_moments *m, ptx_tracer *t, const ptx_adaptive_params *p, ptx_adaptive_status *status);   /* p NULL = defaults; waits */
int  ptx_adaptive_resolve(ptx_adaptive *a, ptx_tracer *t);
/* mean_rgb: W*H*3 floats, the last resolve's frame (zeros before one); samples_per_pixel: W*H int32; tile_error, tile_active: one per
 * tile.  NULLs allowed; waits for the handle's last work. */
int  ptx_adaptive_read(ptx_adaptive *a, float *mean_rgb, int32_t *samples_per_pixel, float *tile_error, uint8_t *tile_active);
float *ptx_adaptive_device_frame(ptx_adaptive *a); /* the resolved frame on the device, W*H*3 floats */
/* The variance-guided filter on an adaptive frame (k_adaptive_prep of csrc/pt_adaptive.hip): ptx_denoise_measured with the divisor, W
 * and B of every pixel's own tile in place of one spp and one B for the frame.  Definition (tests/adaptive_denoise_ref.py
 * restates it), with s = the samples of the pixel's tile:
 *   input c = acc / s (divided by max(albedo, 1e-3) on hit pixels when demodulating), in fp32 and in ptx_denoise_measured's order;
 *   v0 on a hit pixel with B >= min_batches: max(g^T C g, 0) / s, g_k = l_k (/ max(albedo_k, 1e-3)); on the other hit pixels the
 *   spatial estimate of ptx_denoise_variance (n = 1); on miss pixels 0.  min_batches <= 0 means 4, 1 is refused.
 *   Then the filter of ptx_denoise_variance.  A frame whose tiles all hold one count gives ptx_denoise_measured's bits.
 * The un-demodulated acc / s goes into the handle's frame as well: the call includes ptx_adaptive_resolve, and ptx_adaptive_read's
 * mean_rgb is current after it.  The result comes back through ptx_read_denoised and ptx_read_variance.  Nothing else moves: not the
 * accumulation buffer, the moments state, the counts, the flags or the tracer's mask.
 * Refused (PTX_ERR_INVALID, nothing enqueued): NULL handles, bad parameters, a handle of another device or size, tile_world > 1, no
 * add yet, a tile without a sample, and handles that do not count the same samples tile by tile (ptx_adaptive_add's comparison:
 * reset both together).  As for ptx_adaptive_resolve, the accumulation buffer must hold exactly what the last ptx_adaptive_add counted;
 * that is the caller's to keep and cannot be detected.  t's stream waits for both handles' previous work, and both record after the
 * prep.  Not done: combining with the temporal history (ptx_denoise_temporal_measured keeps refusing a tiled moments handle). */
int  ptx_denoise_adaptive(ptx_tracer *t, ptx_adaptive *a, ptx_moments *m, const ptx_denoise_params *dp, const ptx_variance_params *vp,
                          int min_batches);

/* ---- display transform: automatic exposure, tone curve, sRGB transfer, 8-bit codes, csrc/pt_display.hip ------------------------------
 * The accumulation buffer is scene-referred HDR; ptx_write_pbo (the reference's sendImageToPBO) shows it as clamp(int(mean * 255)),
 * linear, exposure 1.  This stage is the same last step with an exposure, a tone curve and a transfer function, on the device, as one
 * more opaque handle.  Nothing of ptx_write_pbo* changes.  Definition (tests/display_ref.py restates it in float64).
 * Input: a W*H*3 fp32 frame rgb and a divisor `samples`.
 *   1 Sanitise: c = rgb / samples (an IEEE fp32 division, as ptx_write_pbo does it); NaN -> 0; c clamped to [0, 65504] per channel
 *     (OIDN's HDR_Y_MAX, the largest half float -- not its pos_max -- so that a block's sum cannot overflow).
 *   2 Meter (meter == PTX_METER_BLOCKS; after OIDN's getAutoexposure, core/color.cpp:33-84, core/color.ispc:180-197): HK = (H + 8) / 16,
 *     WK = (W + 8) / 16; block (i, j) covers rows i*H/HK .. (i+1)*H/HK and columns j*W/WK .. (j+1)*W/WK (integer arithmetic; at most
 *     23 x 23 pixels); L_ij = the block's mean of l(c), l = 0.2126 r + 0.7152 g + 0.0722 b (this library's one luminance, not OIDN's
 *     weights).  Over the blocks with L_ij > 1e-8: m = the mean of log2 L_ij, metered = key / 2^m.  No such block (a black frame,
 *     W < 8 or H < 8: HK * WK = 0): metered = 1.  Block sums are fp32 in a fixed order, the sum over blocks is in double; no float
 *     atomics: the same bits on every run.  A per-pixel histogram is deliberately not the meter: most pixels of a path-traced frame
 *     at low sample counts are exactly zero, and its percentiles move by 10x between 1 and 16 spp where the block rule moves by 6 %.
 *   3 Adaptation: the first metered frame after create / reset: applied = metered.  Later frames:
 *     log2 applied += adapt * (log2 metered - log2 applied), in double, on the device; adapt in (0, 1], 1 = no inertia.
 *   4 Exposure: E = applied * exposure (PTX_METER_BLOCKS) or E = exposure (PTX_METER_MANUAL: nothing is metered, the state is not
 *     touched).  x = c * E in fp32.  The map reads `applied` from device memory: the host never waits for an exposure.
 *   5 Tone: PTX_TONE_CLAMP y = x; PTX_TONE_REINHARD y = x (1 + L / white^2) / (1 + L), L = l(x); PTX_TONE_ACES per channel
 *     y = x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14) (Narkowicz's fit).  Then y is clamped to [0, 1].  The curves are those of
 *     the real numbers for every x in [0, +inf], x = c E beyond fp32's range included: a channel they take to 1 or beyond reads
 *     transfer(1), never 0, and under Reinhard the ratios between a pixel's channels and L are kept there.
 *   6 Transfer: PTX_TRANSFER_LINEAR z = y; PTX_TRANSFER_SRGB z = 12.92 y for y <= 0.0031308, else 1.055 y^(1/2.4) - 0.055.
 *   7 Quantise, alpha 0 as ptx_write_pbo: quantize == 0: (int)((double)z * 255.0), the reference's truncation; quantize == 1:
 *     (int)(z * 255.f + 0.5f); with dither == 1 (read only when quantize == 1): (int)(z * 255.f + t[y & 7][x & 7]),
 *     t = (2 B + 1) / 128 from the 8 x 8 Bayer matrix B (exact in fp32).  The code is the quantisation of exactly the fp32 z that
 *     keep_float stores.
 * meter MANUAL, exposure 1, tone CLAMP, transfer LINEAR, quantize 0 is by construction ptx_write_pbo, byte for byte.
 * A handle serves one W x H on one device, across tracers and streams, like ptx_moments: each enqueueing call makes its stream wait
 * for the handle's previous work and records an event after its own. */
#define PTX_METER_MANUAL 0
#define PTX_METER_BLOCKS 1
#define PTX_TONE_CLAMP 0
#define PTX_TONE_REINHARD 1
#define PTX_TONE_ACES 2
#define PTX_TRANSFER_LINEAR 0
#define PTX_TRANSFER_SRGB 1
#define PTX_DISPLAY_IMAGE 0        /* ptx_display_tracer: the accumulation buffer, divided by spp */
#define PTX_DISPLAY_DENOISED 1     /* the last ptx_denoise* result, divisor 1 */
typedef struct ptx_display ptx_display;            /* opaque: block luminances, exposure state, last result; one W x H on one device */
typedef struct ptx_display_params {
    int   meter;               /* PTX_METER_*; default PTX_METER_BLOCKS */
    float exposure;            /* > 0: the whole exposure (MANUAL) or a factor on the metered one (BLOCKS); default 1 */
    float key;                 /* > 0: the luminance the geometric mean is mapped to; default 0.18 */
    float adapt;               /* in (0, 1]: the share of the way to the metered exposure taken per frame; default 1 */
    int   tone;                /* PTX_TONE_*; default PTX_TONE_ACES */
    float white;               /* > 0: Reinhard's white point; default 4 */
    int   transfer;            /* PTX_TRANSFER_*; default PTX_TRANSFER_SRGB */
    int   quantize;            /* 0 truncate (the reference's), 1 round; default 1 */
    int   dither;              /* 0 / 1: ordered dither of the rounding quantiser; default 0 */
    int   keep_float;          /* 0 / 1: keep z (W*H*3 floats) for ptx_display_read; default 0 */
} ptx_display_params;
typedef struct ptx_display_status {
    float   metered, applied;  /* the last metered frame's exposure and the adapted one the map multiplied by (1, 1 before any) */
    float   log2_mean;         /* m */
    int     blocks_used, blocks_total;     /* blocks with L > 1e-8, HK * WK */
    int64_t frames;            /* metered frames since create / reset */
} ptx_display_status;
void   ptx_default_display_params(ptx_display_params *p);
size_t ptx_sizeof_display_params(void);
size_t ptx_sizeof_display_status(void);
int  ptx_display_create(int device, int width, int height, ptx_display **out);   /* PTX_ERR_NODEVICE without a device */
void ptx_display_destroy(ptx_display *d);          /* NULL is a no-op; waits for its last use */
int  ptx_display_reset(ptx_display *d);            /* forget the adapted exposure: the next metered frame jumps */
/* Enqueues meter + map on t's stream, ordered after every iteration rendered so far and after the last ptx_denoise*, as
 * ptx_write_pbo_device is.  source = PTX_DISPLAY_IMAGE: the accumulation buffer over spp (>= 1); PTX_DISPLAY_DENOISED: the denoised
 * frame, divisor 1 (spp is not read), PTX_ERR_INVALID before the first denoise.  p NULL = defaults.  device_uchar4: W*H uchar4 on the
 * tracer's device; NULL leaves the codes in the handle's own buffer for ptx_display_read.  The accumulation buffer, statistics and
 * what later iterations compute are untouched.  Refused (PTX_ERR_INVALID, nothing enqueued): bad parameters, a handle of another
 * device or size, tile_world > 1. */
int  ptx_display_tracer(ptx_display *d, ptx_tracer *t, int source, int spp, const ptx_display_params *p, void *device_uchar4);
/* The same for any W*H*3 float frame on the handle's device (ptx_adaptive_device_frame; ptx_multi_device_image after
 * ptx_multi_assemble), on `stream` (a hipStream_t; NULL = the default stream): the caller orders the frame's producer before it on
 * that stream.  Pointers that are not 16-byte aligned take a per-pixel form of the map; same results. */
int  ptx_display_device(ptx_display *d, const float *device_rgb, float samples, const ptx_display_params *p, void *device_uchar4, void *stream);
/* The same from a host frame through a staging buffer the handle owns; host_rgba (W*H*4 bytes) may be NULL; waits */
int  ptx_display_host(ptx_display *d, const float *host_rgb, float samples, const ptx_display_params *p, uint8_t *host_rgba);
/* last result; either may be NULL; rgb3 (W*H*3 floats of z) needs keep_float in the last call, rgba4 (W*H*4 bytes) that the last call
 * left its codes in the handle's buffer (device_uchar4 NULL); waits */
int  ptx_display_read(ptx_display *d, float *rgb3, uint8_t *rgba4);
int  ptx_display_read_blocks(ptx_display *d, float *block_lum);                  /* HK*WK floats of the last metered frame; waits */
int  ptx_display_get_status(ptx_display *d, ptx_display_status *out);            /* waits */
/* Host only: the block grid of a w x h frame.  *hk, *wk = HK, WK (0, 0 when either is 0: no block); row_begin (HK + 1 entries) and
 * col_begin (WK + 1 entries), NULLs allowed, receive where each block starts, the last entry being h / w. */
int  ptx_debug_display_blocks(int w, int h, int *hk, int *wk, int32_t *row_begin, int32_t *col_begin);

/* ---- network denoiser: Open Image Denoise's RT filter (a U-Net) run from a caller's .tza weight file, csrc/pt_nn.hip ----------------
 * The reference denoises with OIDN's `RT` filter (apps/src/main.cpp: colour + albedo, hdr off).  This is that filter's data-parallel
 * part on the matrix cores, as one more opaque handle.  No trained weights ship: the caller brings an OIDN 1.4.x weight file, and
 * nothing here claims image quality.  Every other entry point, default and struct is unchanged.  Definition (DESIGN.md 10;
 * tests/unet_ref.py restates it):
 *   Blob: TZA format version 2 (magic 0x41D7; a uint64 table offset; per tensor a name, ndims, dims, a layout x / oihw, a type f / h,
 *     a uint64 data offset), read with every access checked (csrc/pt_tza.h).  A refused blob is PTX_ERR_INVALID and ptx_last_error
 *     names the tensor.
 *   Graph: enc_conv0, enc_conv1, pool, enc_conv2, pool, enc_conv3, pool, enc_conv4, pool, enc_conv5a, enc_conv5b, then for l = 4 .. 1
 *     {upsample (nearest, 2x), concat with the skip, dec_conv<l>a, dec_conv<l>b}, then dec_conv0.  Skips: pool3, pool2, pool1, the
 *     network's input; the upsampled tensor comes first in the channel order.  All convolutions are 3 x 3 with zero padding and a ReLU,
 *     except dec_conv0, which has none.  Channel counts are the blob's: enc_conv0 takes 3, 6 or 9, dec_conv0 gives 3, none above 256.
 *   Frame: W x H zero-padded on the right and bottom to multiples of 16, the image at the top left.  ptx_nn_create runs the frame as
 *     one tile, at most 7680 x 4320; ptx_nn_create_tiled splits it into overlapping tiles under a memory limit (Tiles, below), up to
 *     16384 x 16384.
 *   Arithmetic: activations are fp16 (round to nearest even), channels-last, each tensor's channel count zero-padded to a multiple of
 *     16 (the two sources of a concat separately).  Weights are rounded to fp16 once, at create; biases stay fp32.  A convolution's
 *     output = the fp32 sum, in any order, of the exact fp16 x fp16 products, plus the bias; ReLU; one rounding to fp16.  dec_conv0's
 *     three channels stay fp32.  Pool, upsample and concat are exact.  No atomics: the same bits on every run.  Subnormal fp16
 *     operands and results are kept, in activations and weights alike (measured on gfx950: the matrix core multiplies them exactly
 *     and the rounding of a sum below 2^-14 gives the subnormal); a sum of 65520 or more in magnitude rounds to +-inf.
 *   Input: colour c = rgb / samples (IEEE fp32 division) * scale; NaN -> 0; clamp to [0, 1] (hdr == 0) or [0, FLT_MAX]; then the
 *     forward transfer: hdr: PU(c) / PU(65504), PU(y) = 1412.83765 y (y <= 1.57945760e-6), 1.64593172 y^0.431384981 - 2.94139609e-3
 *     (y <= 3.22087631e-2), else 0.192653254 ln(y + 6.26026094e-3) + 0.998620152; hdr == 0 and srgb == 0: the sRGB curve of the display
 *     transform's step 6 (with powf); srgb != 0: c.  Albedo: NaN -> 0, clamp to [0, 1].  Normal: NaN -> 0, clamp to [-1, 1], * 0.5 + 0.5.
 *   Output: NaN -> 0, clamp to [0, FLT_MAX]; the inverse transfer; min(., 1) when hdr == 0; times 1 / scale (0 when scale is 0).
 *   scale: input_scale when it is not NaN; else, with hdr, the display transform's block meter at key 0.18 on rgb / samples (steps 1
 *     and 2 above, its kernels; the value stays on the device, and the meter's sanitising rule holds where it differs from OIDN's);
 *     else 1.
 *   Tiles (OIDN's maxMemoryMB, restated; csrc/pt_nn_tiles.h): scratch(tw, th) = the activations' bytes of a tw x th frame with this
 *     blob; the limit is max_memory_mb * 2^20 bytes, 0 = none.  From tiles_y = tiles_x = 1, tileH = pad16(H), tileW = pad16(W): while
 *     scratch(tileW, tileH) is above the limit or the tile above 7680 x 4320 -- if tileH > 288 and tileH > tileW, one more tile in y
 *     and tileH = max(pad16(ceil((H - 192) / tiles_y)) + 192, 288); else if tileW > 288 the same in x; else stop (a 288 x 288 tile
 *     above the limit is accepted).  Then tiles_y = H > tileH ? ceil((H - 192) / (tileH - 192)) : 1, and so in x.  Tile (i, j) reads
 *     the window at y = i (tileH - 192), h = min(H - y, tileH) (x, w likewise), zero-padded to multiples of 16 as a frame is, and
 *     keeps it minus 96 rows / columns on each side where another tile follows.  The kept rectangles cover the frame once; origins
 *     are multiples of 16 and a kept pixel is at least 96 pixels (half the receptive field of 174, rounded up to 16) from a cut, so
 *     it sees the data it sees in the whole frame: a tiled run gives the bits of a one-tile run.  The scale is the whole frame's:
 *     the meter runs once.  With more than one tile the result may not overlap the inputs in memory.
 * A handle serves one W x H on one device with one blob, across tracers and streams, with ptx_display's event ordering. */
#define PTX_NN_LAYERS 16
#define PTX_NN_MAX_WIDTH 7680                      /* of one tile */
#define PTX_NN_MAX_HEIGHT 4320
#define PTX_NN_TILE_ALIGN 16
#define PTX_NN_TILE_OVERLAP 96
#define PTX_NN_MIN_TILE 288                        /* 3 * PTX_NN_TILE_OVERLAP */
#define PTX_NN_MAX_FRAME 16384                     /* of a tiled handle, each way */
typedef struct ptx_nn ptx_nn;                      /* opaque: packed weights, scratch, the meter; one W x H on one device */
typedef struct ptx_nn_params {
    int   hdr;                 /* 0 / 1: the PU transfer and an unbounded colour; default 0 */
    int   srgb;                /* 0 / 1: the colour is sRGB-encoded already (read only when hdr == 0); default 0 */
    float input_scale;         /* NaN: automatic (hdr: the block meter; else 1); default NaN */
} ptx_nn_params;
typedef struct ptx_nn_info {
    int      width, height, padded_width, padded_height;
    int      input_channels;                       /* 3 colour, 6 + albedo, 9 + normal */
    int      layers;                               /* PTX_NN_LAYERS */
    int      cin[PTX_NN_LAYERS], cout[PTX_NN_LAYERS];      /* the blob's counts, in the graph's order */
    char     name[PTX_NN_LAYERS][16];
    uint64_t scratch_bytes;                        /* the activations' device memory, planned at create */
    uint64_t macs;                                 /* multiply-adds of one run: the sum over layers of 9 Cin Cout padded pixels at its level */
} ptx_nn_info;
typedef struct ptx_nn_tile {
    int x, y, w, h;                                /* the window read */
    int out_x, out_y, out_w, out_h;                /* the rectangle kept, in frame coordinates */
} ptx_nn_tile;
typedef struct ptx_nn_tiling {
    int      width, height;
    int      tile_width, tile_height;              /* the buffer every tile fits in, multiples of 16 */
    int      tiles_x, tiles_y;
    int      max_memory_mb;                        /* 0: no memory limit, only the tile cap */
    uint64_t scratch_bytes;                        /* of one tile_width x tile_height tile */
    uint64_t macs;                                 /* summed over the tiles' padded windows */
} ptx_nn_tiling;
void   ptx_default_nn_params(ptx_nn_params *p);
size_t ptx_sizeof_nn_params(void);
size_t ptx_sizeof_nn_info(void);
size_t ptx_sizeof_nn_tile(void);
size_t ptx_sizeof_nn_tiling(void);
int  ptx_nn_create(int device, int width, int height, const void *tza, size_t bytes, ptx_nn **out);
int  ptx_nn_create_from_file(int device, int width, int height, const char *path, ptx_nn **out);
/* The same under a memory limit (Tiles, above): frames up to 16384 x 16384; max_memory_mb 0 = no limit, < 0 refused.  With 0 and a
 * frame within 7680 x 4320 the handle is ptx_nn_create's.  On a tiled handle ptx_nn_get_info reports the tile buffer's padded size,
 * the tile's scratch_bytes and the summed macs. */
int  ptx_nn_create_tiled(int device, int width, int height, const void *tza, size_t bytes, int max_memory_mb, ptx_nn **out);
int  ptx_nn_create_from_file_tiled(int device, int width, int height, const char *path, int max_memory_mb, ptx_nn **out);
void ptx_nn_destroy(ptx_nn *n);                    /* NULL is a no-op; waits for its last use */
int  ptx_nn_get_info(ptx_nn *n, ptx_nn_info *out);
/* The handle's tile plan, and the first min(cap, tiles_x * tiles_y) tiles in execution order (row-major); tiles may be NULL */
int  ptx_nn_get_tiling(ptx_nn *n, ptx_nn_tiling *tiling, ptx_nn_tile *tiles, int cap);
/* One denoise of a W*H*3 float frame on the handle's device, on `stream` (NULL = the default stream): rgb / samples in, out_rgb out.
 * alb3 / nrm3 (W*H*3 floats each) are required exactly when the blob takes 6 / 9 inputs and refused otherwise.  p NULL = defaults.
 * On a handle with more than one tile, out_rgb's bytes may not overlap those of rgb, alb3 or nrm3 (PTX_ERR_INVALID): a later tile
 * reads pixels that an earlier tile's result would have replaced. */
int  ptx_nn_denoise_device(ptx_nn *n, const float *device_rgb, float samples, const float *device_alb3, const float *device_nrm3,
                           const ptx_nn_params *p, float *device_out_rgb, void *stream);
/* the same from host frames through staging buffers the handle owns; waits */
int  ptx_nn_denoise_host(ptx_nn *n, const float *rgb, float samples, const float *alb3, const float *nrm3, const ptx_nn_params *p, float *out_rgb);
int  ptx_nn_read_scale(ptx_nn *n, float *scale);   /* the scale the last denoise's input kernel used; waits */
/* The tracer's accumulation buffer over spp, with albedo and normals from its G-buffer in the guide mode that is set, through the
 * network into the tracer's denoised frame: ptx_read_denoised, ptx_device_denoised, ptx_write_denoised_pbo_from_device and
 * ptx_display_tracer(.. PTX_DISPLAY_DENOISED ..) then work as after ptx_denoise.  Enqueued on the tracer's stream; the accumulation
 * buffer, statistics and later iterations are untouched.  Refused like ptx_denoise: tile_world > 1, a handle of another size or device. */
int  ptx_denoise_nn(ptx_tracer *t, ptx_nn *n, const ptx_nn_params *p, int spp);
/* Known-answer entry points over host arrays; they run the production kernels.
 * One convolution: output w x h (before the pool).  src0: fp16 bits, [h][w][cin0], or [h/2][w/2][cin0] when upsample; src1 (cin1 > 0):
 * [h][w][cin1], the second source of a concat.  weights: fp32 [cout][cin0 + cin1][3][3], rounded to fp16 here; bias fp32 [cout].
 * out_half: fp16 bits [h][w][cout], or [h/2][w/2][cout] when pool (2 x 2 max).  out_f32 (optional, cout <= 4, no pool): [h][w][4]. */
int  ptx_kat_nn_conv(int device, int w, int h, int cin0, const uint16_t *src0, int upsample, int cin1, const uint16_t *src1, int cout,
                     const float *weights, const float *bias, int relu, int pool, uint16_t *out_half, float *out_f32);
/* The transfer functions alone on a w x h frame.  inverse == 0: the input kernel; out9 = w*h*9 floats, per pixel the colour, albedo
 * and normal as the network would get them, before the rounding to fp16 (alb3 / nrm3 NULL: zeros).  inverse != 0: rgb is the
 * network's output; the output kernel; out9 = w*h*3 floats.  scale as ptx_nn_params.input_scale, NaN excluded. */
int  ptx_kat_nn_transfer(int device, int w, int h, const float *rgb, const float *alb3, const float *nrm3, int hdr, int srgb, float scale,
                         int inverse, float *out9);
/* Host only: the blob's table as text, one line per tensor: name, ndims, the dims, layout, type, data offset, separated by blanks.
 * *needed = the text's length with its final 0; the text is written when cap >= *needed. */
int  ptx_debug_tza_list(const void *tza, size_t bytes, char *out, size_t cap, size_t *needed);
/* Host only: the plan of the blob (the refusals of ptx_nn_create that need no device); out may be NULL */
int  ptx_debug_nn_plan(const void *tza, size_t bytes, ptx_nn_info *out);
/* Host only: the tile plan ptx_nn_create_tiled would make (its refusals that need no device); tiles as in ptx_nn_get_tiling */
int  ptx_debug_nn_tiling(const void *tza, size_t bytes, int width, int height, int max_memory_mb, ptx_nn_tiling *tiling, ptx_nn_tile *tiles,
                         int cap);

/* ---- network denoiser: prefiltered guides (OIDN's cleanAux), csrc/pt_nn_aux.hip --------------------------------------------------------
 * The guides of a path tracer are noisy where they are honest (sampled guides, guides followed through glass).  OIDN's answer is to
 * denoise the albedo image and the normal image each on its own first -- the RT filter called without a colour image, with the weight
 * files rt_alb / rt_nrm -- and to give the main network, with weights trained for clean guides (rt_hdr_calb_cnrm, rt_ldr_calb_cnrm),
 * the results.  A ptx_nn_prefilter holds one or both of those 3-input networks for one W x H on one device; additive, like everything
 * in this section.  No trained weights ship and nothing here claims image quality.  Definition (tests/unet_aux_ref.py restates it):
 *   Network, frame, arithmetic, tiles: the network denoiser's, above, on a blob whose enc_conv0 takes 3 channels.
 *   scale = input_scale, or 1 when that is NaN; there is no meter.  Every step below is one IEEE fp32 operation.
 *   Albedo in:  v = (a / 1) * scale; NaN -> 0; clamp to [0, 1]; the sRGB curve (srgb == 0) or nothing (srgb != 0): the colour path of
 *     the network denoiser with hdr == 0 and samples == 1.  Albedo out: that path's output: NaN -> 0, clamp to [0, FLT_MAX], the inverse
 *     curve, min(., 1), times 1 / scale.
 *   Normal in:  v = n * scale; NaN -> 0; clamp to [-1, 1]; v * 0.5 + 0.5; no curve.  Normal out: NaN -> 0; clamp to [0, FLT_MAX];
 *     v * 2 - 1; max(., -1); min(., 1); times 1 / scale (0 when scale is 0).
 *   In both the three values fill channels 0 .. 2 of the network's input and the result is three floats per pixel.
 *   Refused, as the RT filter refuses them: an hdr prefilter (the params have no such field), srgb on a normal image, a blob that takes
 *     more than the image (6 or 9 input channels).
 *   Memory: both networks' packed weights, one W*H*3 clean image per network, and ONE activation scratch of the larger plan's size
 *     under the handle's tile limit -- the networks run one after the other on the caller's stream.
 *   Cache (ptx_denoise_nn_prefiltered): guides belong to a camera, not to a sample.  A tracer's G-buffer carries a serial from a
 *     process-wide counter, renewed whenever the G-buffer is computed again (a new camera, ptx_set_guide_samples / _bounces with other
 *     values).  The handle remembers the serial, the params and the networks of its last run through that call; a call with the same
 *     ones runs no prefilter network and leaves `runs` as it is.  ptx_nn_prefilter_run_* always run and forget the serial, as
 *     ptx_nn_prefilter_invalidate does. */
#define PTX_NN_AUX_ALBEDO 1
#define PTX_NN_AUX_NORMAL 2
typedef struct ptx_nn_prefilter ptx_nn_prefilter;  /* opaque: two networks' weights, their one scratch, the clean images */
typedef struct ptx_nn_prefilter_params {
    int   srgb;                /* albedo only: 0 = the sRGB curve (default), 1 = none */
    float input_scale;         /* NaN = 1 (default); else finite and > 0 */
} ptx_nn_prefilter_params;
typedef struct ptx_nn_prefilter_info {
    int         width, height, has_albedo, has_normal;
    ptx_nn_info albedo, normal;                    /* of each network that is there (scratch_bytes: its own plan's); else zeros */
    uint64_t    scratch_bytes;                     /* the one allocation: the larger of the two plans' */
    uint64_t    runs;                              /* calls that ran a prefilter network */
} ptx_nn_prefilter_info;
void   ptx_default_nn_prefilter_params(ptx_nn_prefilter_params *p);
size_t ptx_sizeof_nn_prefilter_params(void);
size_t ptx_sizeof_nn_prefilter_info(void);
/* Either blob may be NULL (no network for that image), not both.  max_memory_mb < 0: each network runs the frame as one tile
 * (ptx_nn_create's cap); else as ptx_nn_create_tiled. */
int  ptx_nn_prefilter_create(int device, int width, int height, const void *alb_tza, size_t alb_bytes, const void *nrm_tza, size_t nrm_bytes,
                             int max_memory_mb, ptx_nn_prefilter **out);
int  ptx_nn_prefilter_create_from_files(int device, int width, int height, const char *alb_path, const char *nrm_path, int max_memory_mb,
                                        ptx_nn_prefilter **out);
void ptx_nn_prefilter_destroy(ptx_nn_prefilter *pf);       /* NULL is a no-op; waits for its last use */
int  ptx_nn_prefilter_get_info(ptx_nn_prefilter *pf, ptx_nn_prefilter_info *out);
/* Both networks on `stream` (NULL = the default stream), into the clean images the handle owns.  An image is W*H pixels with a
 * stride of 3 or 4 floats (4: 16-byte aligned), required exactly where the handle has a network for it, NULL elsewhere. */
int  ptx_nn_prefilter_run_device(ptx_nn_prefilter *pf, const float *device_alb, int alb_stride, const float *device_nrm, int nrm_stride,
                                 const ptx_nn_prefilter_params *p, void *stream);
/* the same from host images of W*H*3 floats; waits; out_* (optional) receive the clean images */
int  ptx_nn_prefilter_run_host(ptx_nn_prefilter *pf, const float *alb3, const float *nrm3, const ptx_nn_prefilter_params *p, float *out_alb3,
                               float *out_nrm3);
/* the clean images on the device, W*H*3 floats each (NULL where the handle has no network); valid after the run's work */
int  ptx_nn_prefilter_device_clean(ptx_nn_prefilter *pf, const float **alb3, const float **nrm3);
int  ptx_nn_prefilter_read(ptx_nn_prefilter *pf, float *alb3, float *nrm3);       /* either may be NULL; waits */
int  ptx_nn_prefilter_invalidate(ptx_nn_prefilter *pf);    /* the next ptx_denoise_nn_prefiltered runs the networks again */
/* ptx_denoise_nn with the main network's guides prefiltered: a main network of 6 inputs gets the clean albedo (refused when pf has no
 * albedo network); one of 9 inputs gets each guide clean where pf has a network for it, else the G-buffer's own; one of 3 inputs is
 * refused.  The colour path, the scale and the meter are ptx_denoise_nn's, and so are its refusals, for both handles.  pp NULL =
 * defaults.  The clean images are cached per G-buffer (Cache, above). */
int  ptx_denoise_nn_prefiltered(ptx_tracer *t, ptx_nn *main_nn, ptx_nn_prefilter *pf, const ptx_nn_params *p, const ptx_nn_prefilter_params *pp,
                                int spp);
/* The two kernels of the prefilter alone on a w x h image of three floats per pixel.  inverse == 0: the input kernel, out3 = what the
 * network would get, before the rounding to fp16; inverse != 0: in3 is the network's output, out3 the output kernel's result.  scale
 * finite and >= 0. */
int  ptx_kat_nn_transfer_aux(int device, int w, int h, int kind, const float *in3, int srgb, float scale, int inverse, float *out3);
/* Host only: what ptx_nn_prefilter_create and a run would refuse without a device: the blobs (NULL: none), the params (NULL: defaults) */
int  ptx_debug_nn_prefilter_problem(const void *alb_tza, size_t alb_bytes, const void *nrm_tza, size_t nrm_bytes,
                                    const ptx_nn_prefilter_params *p);

/* ---- network denoiser: images (formats, strides, in place), csrc/pt_nn_image.hip ---------------------------------------------------------
 * ptx_nn_denoise_* take W*H*3 packed floats.  A renderer's framebuffer is float4 or half4, often with a row pitch, and wants the
 * result where the colour was.  These entry points run the same networks on images described as OIDN's setImage describes them
 * (core/image.h: a format, a byte offset, a byte pixel stride, a byte row stride); additive, like everything in this section.
 * Definition (tests/nn_image_ref.py restates it):
 *   Image: ptr NULL = no such image.  size = 4 (PTX_NN_FORMAT_FLOAT3) or 2 (PTX_NN_FORMAT_HALF3) bytes per channel; a pixel_stride of
 *     0 means 3 * size, a row_stride of 0 means width * pixel_stride.  Channel c (0 .. 2) of pixel (x, y) is the `size` bytes at
 *     ptr + byte_offset + y * row_stride + x * pixel_stride + c * size, all of it size_t arithmetic.  No other byte is written, and
 *     none is read but by the 16- / 8-byte load of a 16- / 8-byte aligned float / half image with a pixel stride of 16 / 8 bytes, which
 *     takes the pixel's fourth channel along and drops it.
 *   Refused (PTX_ERR_INVALID; ptx_last_error names the image and the rule), OIDN's checks: an unknown format; a pixel stride below the
 *     pixel's size; a row stride below width * pixel_stride; a row stride that is no multiple of the pixel stride.  Ours, not OIDN's --
 *     the device needs aligned channels: ptr + byte_offset, the pixel stride or the row stride no multiple of the channel size.
 *   Formats: the inputs are all Float3 or all Half3 (UNetFilter::init); the output may be either.
 *   Half in: widened exactly to fp32; every step after that is the packed path's.  Half out: fp16_rne(v > 65504 ? 65504 : v) of the fp32
 *     value v the packed path would store (numpy: np.minimum(v, 65504).astype(np.float16)): +inf is never written, subnormals are kept.
 *   Role, of a 3-input network's one image: PTX_NN_ROLE_COLOR is ptx_nn_denoise_device's arithmetic, whatever the input count.
 *     PTX_NN_ROLE_ALBEDO / _NORMAL are the prefilter's "Albedo in / out" / "Normal in / out", above: no meter, scale = input_scale or
 *     1; refused on a blob of 6 or 9 inputs, with hdr != 0, with samples != 1, and NORMAL with srgb != 0.
 *   Automatic hdr scale: the block meter on the fp32 values of the colour image (halves widened).  A packed Float3 colour is metered
 *     where it lies; any other layout is first gathered into a W*H*3 float buffer the handle owns (first need).
 *   In place: an image's byte interval is [first channel byte of (0, 0), last channel byte of (W - 1, H - 1) + 1).  Where the
 *     output's interval meets no input's, or the handle has one tile, every tile's result goes straight to the output (one tile: each
 *     read of the input stage precedes each write of the output stage on the stream).  Where it meets one and the handle has more
 *     than one tile, the tiles' results go to a W*H*3 fp32 temporary the handle owns -- allocated on first need beside the activation
 *     scratch and outside max_memory_mb -- and a copy kernel writes it through the output's descriptor after the last tile, the half
 *     conversion there.  All three ways give the same bits. */
#define PTX_NN_FORMAT_FLOAT3 1
#define PTX_NN_FORMAT_HALF3 2
#define PTX_NN_ROLE_COLOR 0
#define PTX_NN_ROLE_ALBEDO 1
#define PTX_NN_ROLE_NORMAL 2
typedef struct ptx_nn_image {
    const void *ptr;           /* NULL: no such image */
    int    format;             /* PTX_NN_FORMAT_FLOAT3 = 1, PTX_NN_FORMAT_HALF3 = 2 */
    size_t byte_offset;        /* of pixel (0,0) from ptr */
    size_t pixel_stride;       /* bytes; 0 = the pixel's size (12 / 6) */
    size_t row_stride;         /* bytes; 0 = width * pixel_stride */
} ptx_nn_image;
size_t ptx_sizeof_nn_image(void);
/* One denoise on `stream` (NULL = the default stream) of images on the handle's device.  albedo / normal (NULL, or ptr NULL: none) are
 * required exactly when the blob takes 6 / 9 inputs; output is written (its ptr is not const to the callee).  p NULL = defaults. */
int  ptx_nn_denoise_images_device(ptx_nn *n, const ptx_nn_image *color, const ptx_nn_image *albedo, const ptx_nn_image *normal,
                                  const ptx_nn_image *output, float samples, int role, const ptx_nn_params *p, void *stream);
/* The same on host images, through staging buffers the handle owns; waits.  Each image's byte interval is staged: the inputs up, the
 * output's interval up and back, so the bytes between its pixels come back unchanged.  Images whose intervals meet in the caller's
 * memory meet the same way on the device.  What needs no device is refused before any device call: the params, the role's rules, the
 * formats, then -- with a handle -- the images it needs and each descriptor. */
int  ptx_nn_denoise_images_host(ptx_nn *n, const ptx_nn_image *color, const ptx_nn_image *albedo, const ptx_nn_image *normal,
                                const ptx_nn_image *output, float samples, int role, const ptx_nn_params *p);
/* Host only: what a call would refuse of this descriptor for a width x height frame (is_output: it is named "output") */
int  ptx_debug_nn_image_problem(int width, int height, const ptx_nn_image *img, int is_output);

/* ---- network denoiser: the lightmap filter (OIDN's RTLightmap), csrc/pt_nn_lightmap.hip ----------------------------------------------------
 * OIDN's rtlightmap_hdr.tza and rtlightmap_dir.tza are the RT filter's U-Net with three inputs, so a lightmap network is a ptx_nn made
 * from such a blob: handle, tiles, scratch and convolutions are the ones above, and two kernels of this unit stand at the network's
 * ends.  Additive.  Images are ptx_nn_image descriptors under every rule of the section above: the refusals, the staging of host
 * images, half in and out, in place (with the temporary and the copy-out where the handle has more than one tile).
 * Definition (core/input_reorder.ispc, output_reorder.ispc, color.ispc restated; every step one IEEE fp32 operation; tests/nn_lightmap_ref.py
 * restates it), per channel:
 *   directional == 0, HDR: OIDN's Log transfer with hdr.  xmax = (float)log(65505.0) = 0x1.62e050p+3, norm = (float)(1.0 / (double)xmax)
 *     = 0x1.71587ep-4, both formed in double on the host and rounded once.
 *       in : v = in * scale; NaN -> 0; clamp to [0, FLT_MAX]; x = logf(v + 1.f) * norm
 *       out: NaN -> 0; clamp to [0, FLT_MAX]; y = expf(x * xmax) - 1.f; y * (1 / scale), or 0 for scale 0
 *     logf and expf are the correctly rounded functions (formed in double, rounded once): expf(a) - 1.f near 0 turns an ulp of expf
 *     into 2^-23 absolute, and only the correctly rounded value keeps the result within 2^-24 / scale of the exact one.
 *     scale: input_scale where it is set; with NaN the display unit's block meter at key 0.18 on the fp32 colour, exactly as
 *     ptx_nn_denoise_images_* meters an hdr frame (a layout that is not packed Float3 is gathered first).
 *   directional == 1: OIDN's Linear transfer with snorm, not hdr -- PTX_NN_ROLE_NORMAL's arithmetic to the bit:
 *       in : v = in * scale; NaN -> 0; clamp to [-1, 1]; v * 0.5f + 0.5f
 *       out: NaN -> 0; clamp to [0, FLT_MAX]; * 2 - 1; max(., -1); min(., 1); * (1 / scale)
 *     scale: input_scale, or 1 for NaN.
 *   Refused (PTX_ERR_INVALID), without a device: directional other than 0 or 1; an input_scale that is neither NaN nor finite and > 0;
 *   an unknown format; then, with a handle: a blob of 6 or 9 inputs; what ptx_nn_denoise_images_* refuses of a descriptor. */
int  ptx_nn_denoise_lightmap_device(ptx_nn *n, const ptx_nn_image *color, const ptx_nn_image *output, int directional, float input_scale,
                                    void *stream);
int  ptx_nn_denoise_lightmap_host(ptx_nn *n, const ptx_nn_image *color, const ptx_nn_image *output, int directional, float input_scale);
/* Host only: the HDR mode's two constants as the kernels get them */
void ptx_debug_nn_lightmap_constants(float *xmax, float *norm);

/* ---- network denoiser: progress and cancellation, csrc/pt_nn_progress.h --------------------------------------------------------------------
 * A monitor on a handle hears how far a denoise has come and may cancel it.  fn NULL: none (the default).
 * With no monitor every call enqueues exactly what it enqueued before this section existed and waits where it waited.
 * With a monitor, every ptx_nn_denoise_*, ptx_nn_denoise_images_* and ptx_nn_denoise_lightmap_* call on the handle RUNS TO COMPLETION
 * BEFORE IT RETURNS, the _device forms included, and reports:
 *   fn(user, 0.0) before any device work of the call is enqueued;
 *   then fn(user, n) after every unit of work has finished on the device (an owned event recorded behind each is waited for): per
 *   tile its input stage, each of its sixteen layers and its output stage, and the in-place copy-out where one runs.  n = finished
 *   units / all units: it never decreases, and it is exactly 1.0 on the last report, which comes after the result is complete on the
 *   device.  A frame of one tile reports 18 times after the first.  The host enqueues at most one tile beyond the tile whose reports
 *   it is delivering.
 * Cancel: when fn returns 0 nothing further is enqueued, the call waits for what is in flight and returns PTX_ERR_CANCELLED -- also
 *   on the last report (n == 1), as OIDN's Progress::update has it.  The handle stays usable; a later call gives the right bits.  A
 *   _host form has then not written the caller's output memory at all; after a _device form only bytes of the output's three
 *   channels may have been written.
 * The monitor is called on the calling thread and must not call into the same handle (ptx_nn_set_progress from it is refused).
 * ptx_nn_prefilter_* and ptx_denoise_nn* on a tracer ignore the monitor. */
#define PTX_ERR_CANCELLED 6    /* the progress monitor returned 0 */
typedef int (*ptx_nn_progress_fn)(void *user, double n);   /* 0 = cancel */
int  ptx_nn_set_progress(ptx_nn *n, ptx_nn_progress_fn fn, void *user);

/* ---- image metrics: MSE, PSNR, L1, MAPE, SMAPE, gradient, SSIM, MS-SSIM and the error count, csrc/pt_metrics.hip --------------------------
 * How good a frame is against a reference frame, on the device, every figure in one call.  It stands where OIDN's training/compare_image.py
 * (mse, psnr, ssim, msssim), training/ssim.py (SSIM, MS-SSIM), training/loss.py (l1, l2, mape, smape, ssim, msssim, l1_msssim, l1_grad)
 * and apps/utils/image_io.cpp:435-462 (compareImage: what oidnDenoise --ref prints) stand there.  Additive: one more handle, no existing
 * entry point, default or struct changes.  Definition (tests/metrics_ref.py restates it in float64 and in float32):
 *   Images: a (the test image) and b (the reference image) are ptx_nn_image descriptors of one W x H under every rule of "images" above
 *     (formats, strides, offset, refusals; halves widened exactly).  Each has a divisor, samples_a / samples_b, finite and > 0.
 *   Sanitise (training/image.py:69, np.nan_to_num): r = the channel as stored; s = r / samples (an IEEE division); NaN -> 0, +inf ->
 *     FLT_MAX, -inf -> -FLT_MAX.  nonfinite_a / nonfinite_b count the stored channels r that are NaN or +-inf.
 *   Transform t(s), every step one IEEE fp32 operation:
 *     PTX_METRICS_NONE  t = s.
 *     PTX_METRICS_SRGB  t = 12.92 s for s <= 0.0031308, else 1.055 powf(s, 1 / 2.4) - 0.055 (csrc/pt_nn_transfer.h's forward curve).
 *     PTX_METRICS_HDR   t = srgb(tonemap(s * exposure)) (training/dataset.py:200-205).  tonemap (training/color.py:181-194) is Hable's
 *       curve: e(v) = (v (0.22 v + 0.03) + 0.002) / (v (0.22 v + 0.30) + 0.06) - 0.01 / 0.30, tonemap(x) = min(e(x * 1.758141) / e(11.2), 1),
 *       the four constants and e(11.2) formed in double and rounded once.  x * 1.758141 is held to [-2^60, 2^60] inside the curve, where
 *       the curve has long been clamped: FLT_MAX does not become inf / inf.  An `exposure` of NaN is the automatic one: the display
 *       transform's block meter (above, steps 1 and 2) at key 0.18 on b over samples_b, i.e. 0.18 over the metered geometric-mean
 *       luminance -- ptx_display_status.metered of that frame, the scale the network's hdr path takes.  (A layout of b that is not
 *       packed Float3 is gathered first.)
 *     PTX_METRICS_SNORM t = s * 0.5 + 0.5 (dataset.py:206-208).
 *     Under SRGB and HDR an infinite t (12.92 * -FLT_MAX; the curve at one of its two poles below 0) is held to +-FLT_MAX.
 *   Pointwise, on ta = t(a), tb = t(b), over all N = 3 W H samples, each term in fp32: d = ta - tb;
 *     mse = mean d d; l1 = mean |d|; mape = mean |d| / (|tb| + 0.01f); smape = mean |d| / (|ta| + |tb| + 0.01f);
 *     psnr = 10 log10(1 / mse), in double on the host (+inf for mse 0).
 *     grad (image.py:34-38 under L1; needs W, H >= 2): over i < H - 1, j < W - 1 and the three channels, the mean of
 *     |(ta[i+1][j] - ta[i][j]) - (tb[i+1][j] - tb[i][j])| and |(ta[i][j+1] - ta[i][j]) - (tb[i][j+1] - tb[i][j])|, 6 (W-1)(H-1) terms.
 *     l1_msssim = 0.16 l1 + 0.84 (1 - msssim), in double on the host.
 *   compareImage, on sa, sb (after the divisor, before the transform), as image_io.cpp writes it: error = |sb - sa|; where sb != 0,
 *     error = (error / sb < error) ? error / sb : error -- a negative sb makes the error negative, as there; max_error = the maximum over
 *     max(0, error); num_errors = the count of error > threshold.
 *   SSIM (ssim.py, data_range 1) per channel on planar ta, tb: an 11-tap window g, the fp32 values of exp(-k^2 / 4.5) / sum (k = -5 .. 5;
 *     ptx_metrics_plan.taps), applied along x and then along y in valid mode, each filter a left-to-right fp32 sum of products, to
 *     x, y, x x, y y, x y.  With m1, m2 the filtered x, y: s1 = f(xx) - m1 m1, s2 = f(yy) - m2 m2, s12 = f(xy) - m1 m2,
 *     cs = (2 s12 + C2) / (s1 + s2 + C2), l = (2 m1 m2 + C1) / (m1 m1 + m2 m2 + C1), C1 = 0.01^2, C2 = 0.03^2 as floats; the map value is
 *     l cs.  ssim_c[c] = the mean of the (H - 10)(W - 10) map values, ssim = the mean over channels.  Needs min(W, H) >= 11.
 *   MS-SSIM (needs min(W, H) > 160): five scales, weights 0.0448, 0.2856, 0.3001, 0.2363, 0.1333 (as floats); between scales
 *     avg_pool2d(kernel 2, padding (H % 2, W % 2)) as PyTorch defines it: zeros on both sides, which count in the divisor of 4, output
 *     floor((H + 2 p - 2) / 2) + 1.  mcs[s][c] = the mean of cs on scales 0 .. 3 and of l cs on scale 4;
 *     msssim_c[c] = prod_s max(mcs[s][c], 0)^weight[s], msssim = the mean over channels (double, on the host).
 *   Sums: every mean is a sum in fp64 -- per-workgroup partials in a fixed tree, then one finishing workgroup in a fixed order -- divided
 *     on the host.  No floating-point atomics: two calls on the same data return the same bits.
 *   Where a metric is not defined for the size its fields are NaN and its bit of `valid` is clear; the call succeeds and fills the rest.
 *   A bit of `valid` is also clear where its metric came out NaN: samples near FLT_MAX (a sanitised infinity under NONE, SRGB, SNORM)
 *   have squares of +inf, and the window's f(xx) - m1 m1 is then inf - inf, here as in ssim.py.  A set bit means a number.
 *   The pointwise fields have no bit: an infinity in one image makes mse and l1 +inf, and +FLT_MAX against -FLT_MAX at one sample
 *   makes smape inf / inf = NaN, as in loss.py.
 * Calls WAIT for the result (psnr, msssim and the means are finished on the host).  A handle serves one W x H on one device with
 * ptx_display's event ordering. */
#define PTX_METRICS_NONE 0
#define PTX_METRICS_SRGB 1
#define PTX_METRICS_HDR 2
#define PTX_METRICS_SNORM 3
#define PTX_METRICS_VALID_SSIM 1
#define PTX_METRICS_VALID_MSSSIM 2
#define PTX_METRICS_VALID_GRAD 4
#define PTX_METRICS_SCALES 5
#define PTX_METRICS_TAPS 11
typedef struct ptx_metrics ptx_metrics;            /* opaque: the planar pyramid of both images, the partial sums; one W x H on one device */
typedef struct ptx_metrics_params {
    int   transform;           /* PTX_METRICS_*; default PTX_METRICS_NONE */
    float exposure;            /* HDR: finite and > 0, or NaN = metered on b; default NaN */
    float threshold;           /* compareImage's; finite, >= 0; default 0.01 */
    float samples_a, samples_b;/* the divisors; default 1 */
    int   pointwise_only;      /* 0 / 1: leave SSIM and MS-SSIM out (their fields NaN, their bits clear, no map); default 0 */
} ptx_metrics_params;
typedef struct ptx_metrics_result {
    size_t   struct_size;      /* set by the CALLER to sizeof(ptx_metrics_result) as it knows it: no byte beyond is written */
    double   mse, psnr, l1, mape, smape, grad, l1_msssim;
    double   ssim, msssim;
    double   ssim_c[3], msssim_c[3];
    double   mcs[PTX_METRICS_SCALES][3];           /* [scale][channel]; scale 4 holds l cs */
    double   max_error;
    uint64_t num_errors, nonfinite_a, nonfinite_b;
    float    exposure;         /* the one used (HDR), else 1 */
    int      valid;            /* PTX_METRICS_VALID_* */
} ptx_metrics_result;
typedef struct ptx_metrics_plan {
    int    ssim_valid, msssim_valid;
    int    scales;             /* levels held: 5 with MS-SSIM, else 1 (the pointwise terms and grad read level 0) */
    int    w[PTX_METRICS_SCALES], h[PTX_METRICS_SCALES];           /* of every scale the rule defines, held or not */
    int    tile_w, tile_h;     /* k_metrics_ssim's output tile */
    int    blocks[PTX_METRICS_SCALES];             /* its workgroups per scale (0: none run) */
    int    prep_blocks, grad_blocks;
    size_t level_offset[PTX_METRICS_SCALES];       /* floats, into one image's pyramid */
    size_t pyramid_floats;     /* one image's pyramid: 3 w h over the levels held */
    size_t partial_doubles;    /* all partial sums */
    size_t map_floats;         /* (W - 10)(H - 10), or 0 */
    float  taps[PTX_METRICS_TAPS];
    float  weights[PTX_METRICS_SCALES];
} ptx_metrics_plan;
void   ptx_default_metrics_params(ptx_metrics_params *p);
size_t ptx_sizeof_metrics_params(void);
size_t ptx_sizeof_metrics_result(void);
size_t ptx_sizeof_metrics_plan(void);
int  ptx_metrics_create(int device, int width, int height, ptx_metrics **out);   /* PTX_ERR_NODEVICE without a device; at most 16384 x 16384 */
void ptx_metrics_destroy(ptx_metrics *m);          /* NULL is a no-op; waits for its last use */
/* a, b: images on the handle's device, compared on `stream` (NULL = the default stream; the caller orders their producers before it
 * there).  p NULL = defaults.  map_or_null: (H - 10)(W - 10) floats on the device that receive the full-resolution SSIM map, the mean
 * over channels ((v0 + v1) + v2) / 3 in fp32; refused where SSIM is not defined.  out->struct_size is read first (a sized struct: a
 * later library with more fields writes no more than that).  Refused before any device call: bad params, a NULL image, a bad descriptor. */
int  ptx_metrics_compare_device(ptx_metrics *m, const ptx_nn_image *a, const ptx_nn_image *b, const ptx_metrics_params *p,
                                ptx_metrics_result *out, float *device_map_or_null, void *stream);
/* The same on host images: each image's byte interval is staged into a buffer the handle owns; host_map_or_null is host memory. */
int  ptx_metrics_compare_host(ptx_metrics *m, const ptx_nn_image *a, const ptx_nn_image *b, const ptx_metrics_params *p,
                              ptx_metrics_result *out, float *host_map_or_null);
/* The tracer's frame as a: source PTX_DISPLAY_IMAGE = the accumulation buffer over spp (samples_a is not read), PTX_DISPLAY_DENOISED =
 * the last ptx_denoise* result over 1.  b describes HOST memory and is staged.  Runs on the tracer's stream behind every iteration
 * rendered so far; the accumulation buffer, the statistics and what later iterations compute are untouched.  Refusals as
 * ptx_display_tracer's. */
int  ptx_metrics_tracer(ptx_metrics *m, ptx_tracer *t, int source, int spp, const ptx_nn_image *b, const ptx_metrics_params *p,
                        ptx_metrics_result *out);
/* Host only: the scale sizes, window taps and buffer sizes of a w x h handle */
int  ptx_debug_metrics_plan(int w, int h, ptx_metrics_plan *out);
/* Host only: what a compare call would refuse of these params (NULL: the defaults) and descriptors for a width x height frame */
int  ptx_debug_metrics_problem(int width, int height, const ptx_nn_image *a, const ptx_nn_image *b, const ptx_metrics_params *p);

/* ---- per-stage entry points (parity tests; same record layouts as the reference's PathSegment 44 B and
 *      ShadeableIntersection 32 B, host arrays in/out, the work runs on the device); ptx_kat_reproject, at the end, is the denoiser's
 *      reprojection alone and needs no tracer ------------------------------------------------------------------- */
int ptx_kat_geom_test(ptx_tracer *t, int geom, int n, const float *rays6, float *out10);
/* objTriIntersectionTest / triangleIntersectionLocalTest, src/intersections.h:175-205, 284-315: dead code in the reference (its call is
 * commented out, src/pathtrace.cu:313) and on no path here; a known-answer entry point only.  out8 per ray: t (object space), world
 * point, world normal, outside.  Non-OBJ geoms give t = -1. */
int ptx_kat_obj_tri_test(ptx_tracer *t, int geom, int n, const float *rays6, float *out8);
/* calculateJitteredDirectionHemisphere, src/interactions.h:46-85: dead code in the reference (JITTERED_SAMPLING 0, its call site does not
 * compile) and on no path here; a known-answer entry point only.  Per sample: a normal and (iter, index, depth), which seed the engine as
 * makeSeededRandomEngine does (src/pathtrace.cu:62-66); out3 = the direction. */
int ptx_kat_jittered_hemisphere(ptx_tracer *t, int n, const float *normals3, const int32_t *seeds3, int max_iter, float *out3);
int ptx_kat_compute_intersections(ptx_tracer *t, int n, const void *paths44, void *isects32);
/* computeIntersections (src/pathtrace.cu:261-344) through the functions the bounce kernels really run -- candidate masks from the
 * world boxes, the tile's (ray, geom) pairs tested by the key functions, 64-bit minimum, winner decoded (split != 0: the three
 * pieces of the split mesh search, BVH traversal with the stack included) -- where ptx_kat_compute_intersections runs the plain
 * per-ray loop over all geoms.  PTX_ERR_UNSUPPORTED for a scene that does not take that path (more than 32 geoms, no_cull, ...). */
int ptx_kat_tile_intersect(ptx_tracer *t, int n, const void *paths44, void *isects32, int split);
int ptx_kat_shade(ptx_tracer *t, int iter, int n, const int32_t *idx, const void *isects32, void *paths44);
int ptx_kat_generate(ptx_tracer *t, int iter, void *paths44);             /* all W*H camera rays */
int ptx_kat_libm(ptx_tracer *t, int n, const float *x, float *sin_out, float *cos_out,
                 const double *pw_in, double *pow5_out, const float *powf_xy, float *powf_out);
/* The device's guarded core square root / reciprocal (pt_device.h: pt_sqrt, pt_rsqrt_glm, pt_rcp_pos) against the compiler's IEEE
 * expansions of sqrtf(x), 1 / sqrtf(x) and 1 / a, on ALL 2^32 operand bit patterns: mismatches[3] = how many patterns differ
 * bitwise (two NaNs count as equal).  0, 0, 0 is the only acceptable answer. */
int ptx_kat_fast_exact(ptx_tracer *t, int64_t mismatches[3]);
/* Two more routines of pt_device.h against what they stand for, on the device.  counts[0]: bit patterns, of ALL 2^32, on which pt_rsqrt_unit
 * (1 / sqrt of an operand next to 1) differs from pt_rsqrt_glm; counts[1]: patterns inside its window (2 W + 1).  counts[2]: quotients of
 * pt_div_pairs3 (a cube's six slab quotients, one reciprocal per axis) that differ from the divisions a / d, over every pair of exponents for
 * numerator and denominator with exponent_reps random mantissas each, every triple of the special values (zeros, infinities, NaNs, subnormals,
 * the guard's bounds) and random_sets random sets from the slab test's range; counts[3]: sets that took the shared reciprocal.  Two NaNs
 * count as equal.  counts[0] == counts[2] == 0 is the only acceptable answer. */
int ptx_kat_unit_rsqrt(ptx_tracer *t, int exponent_reps, int64_t random_sets, int64_t counts[4]);
/* The reprojection and mix of ptx_denoise_temporal (variant 0), ptx_denoise_variance (1) and ptx_denoise_temporal_measured (2) alone,
 * over caller-owned host arrays of one W x H frame (as ptx_denoise_buffers; tests/test_gpu_temporal_grid.py): staged into the device
 * layouts and run through the same camera set-up and launch as those entry points, synchronously on `device`.
 *   hist_cam: the committed history's camera, resolution W x H; NULL = no history (the hist_* arrays are then not read).
 *   tp NULL = defaults; spp >= 1; rgb = the accumulation (W*H*3), nrm3 / pos3 / alb3 (W*H*3), ids2 (W*H*2: material, geom) and hit
 *   (W*H bytes) = the current guides; spec = nmats bytes (!= 0: reflective or refractive), may be NULL when nmats == 0.
 *   hist_*: the hist state: hit bytes, normal, position, sample count n, D, V (NULL = the state carries none) and ids.
 *   variant 2: scatter6 = W*H*6 floats (rr, gg, bb, rg, rb, gb) of a moments state's M and batches = its B >= 2.
 * Outputs (NULLs allowed), the records the kernel writes: the new state's nh4 (normal, hit), xn4 (position, n), dd4 (D, V) and ids2,
 * mix3 and hn4 (h, n_h).  Bad arguments: PTX_ERR_INVALID before the device is looked for; PTX_ERR_NODEVICE without one. */
int ptx_kat_reproject(int device, int w, int h, int variant, const ptx_camera *hist_cam, const ptx_temporal_params *tp, int spp,
                      const float *rgb, const float *nrm3, const float *pos3, const float *alb3, const int32_t *ids2, const uint8_t *hit,
                      const uint8_t *spec, int nmats, const uint8_t *hist_hit, const float *hist_nrm3, const float *hist_pos3,
                      const float *hist_n1, const float *hist_D3, const float *hist_V1, const int32_t *hist_ids2, const float *scatter6,
                      int batches, float *out_nh4, float *out_xn4, float *out_dd4, int32_t *out_ids2, float *out_mix3, float *out_hn4);
/* CPU-only (no device, no tracer): the per-tile geom masks the camera-ray bounce uses (bit g of masks_out[tile] clear = no camera ray of
 * that tile of 256 owned pixels can reach box g; boxes6 = lo xyz, hi xyz per geom, <= 32 geoms), for a camera, depth of field on / off and a
 * row-tile split.  Returns the number of tiles, -1 on a bad argument.  The CPU tests check the superset property ray by ray. */
int ptx_debug_tile_geoms(const ptx_camera *camera, int ngeoms, const float *boxes6, int depth_of_field, int tile_rows, int tile_rank,
                         int tile_world, uint32_t *masks_out, int max_tiles);
/* CPU-only: which material bins' stored paths carry what: masks[0] bit b = records of bin b carry the incoming direction
 * (reflective / refractive materials, materials of OBJ geoms), masks[1] bit b = they carry a 3-bit code instead of the normal (materials
 * only cubes have); bin = nmaterials - 1 - material when sorting by material, else 0; at most two runs of set bits in either.
 * geom_type: 0 sphere, 1 cube, 3 OBJ.  Returns 0, -1 on a bad argument (nmaterials 1..64). */
int ptx_debug_record_masks(int nmaterials, const ptx_material *materials, int ngeoms, const int32_t *geom_type, const int32_t *geom_material,
                           int sort_by_material, uint64_t masks[2]);
/* CPU-only: the table the candidate pre-test (the conservative world boxes every ray is tested against before the exact tests) reads on
 * the device, for n corner boxes (lo xyz, hi xyz): 8 floats per box = centre xyz, 0, half extent xyz, 0.  The CPU tests check that it
 * contains the corner box and that the device's slab arithmetic on it never rejects a ray that reaches the corner box. */
int ptx_debug_cull_boxes(int n, const float *boxes6, float *centre_half8);
/* CPU-only: the geoms a path can end on with radiance, as ptx_create works them out: bit g of *bits_out (g < 32) = the material of geom g
 * (geom_material[g]) has emittance > 0.  The last bounce of a path looks only for these geoms.  Returns 0, -1 on a bad argument. */
int ptx_debug_light_bits(int nmaterials, const ptx_material *materials, int ngeoms, const int32_t *geom_material, uint32_t *bits_out);
/* CPU-only: the object-space boxes of the small meshes (the meshes of a scene in which no mesh is large enough for a BVH), as ptx_create
 * builds them for the candidate pre-test: a ray is a candidate of such a mesh when it reaches the box of the mesh's faces in the mesh's own
 * space, which a rotated mesh fills where it fills a fraction of its world box.  geoms as ptx_create takes them (ngeoms <= 32), no_bvh as
 * ptx_options.no_bvh (no mesh gets a BVH, so every mesh counts as small); table16 = 16
 * floats per geom, zeros for a geom without an entry: three rows of (a row of the inverse transform's 3 x 3 part, the world point mapped to
 * the box's centre), the half extent xyz with its derived margins, the margin per unit of the ray origin's distance from the centre;
 * bit g of *bits_out = geom g has an entry.  margin = 1: the derived margins, 0: none (the CPU tests show with it that they can fail).
 * Returns 0, -1 on a bad argument.  The environment variable PTX_DEBUG_NO_OBJCULL, read by ptx_create, leaves every mesh without an entry:
 * candidates then come from the world boxes alone (A/B timing, tests of both paths; same results either way). */
int ptx_debug_cull_objboxes(int ngeoms, const ptx_geom *geoms, int no_bvh, float margin, float *table16, uint32_t *bits_out);
/* CPU-only: the tangent frames of the cubes' faces, as ptx_create tabulates them for the diffuse sampler.  A stored hit on a cube of a
 * material that only cubes have names one of the cube's six face normals by a code; the two vectors the sampler builds from a normal
 * (perp1, perp2 of calculateRandomDirectionInHemisphere) depend on that normal alone, so the bounce reads them from this table instead of
 * computing them per ray.  geoms as ptx_create takes them; out36_per_geom = 36 floats per geom: side (axis * 2 + (sign > 0)) at side * 6 =
 * perp1 xyz, perp2 xyz, computed from that side's tabulated normal with the sampler's own arithmetic (same bits); zeros for a geom that is
 * not a cube.  Returns 0, -1 on a bad argument.  The environment variable PTX_DEBUG_NO_TANGENTS, read by ptx_create, makes every ray
 * compute its frame (A/B timing, tests of both paths; same results either way). */
int ptx_debug_cube_tangents(int ngeoms, const ptx_geom *geoms, float *out36_per_geom);
/* Host-only (reads what ptx_create kept on the host, launches nothing): how mesh geom `geom` of a live tracer is searched.
 * out8 = { root of its BVH (-1: none, the plain loop over its faces), depth of the binary tree, root of its four-wide nodes (-1: none),
 * stack entries their walk needs, stack entries per lane the tracer's launches provide (bvh_stack), 1 if frames take the split mesh search
 * (k_mesh + k_finish) else 0, the walk a FRAME takes for this geom, the walk the single-ray search takes when it is handed a stack
 * (ptx_kat_tile_intersect with split = 1) }, walks as PTX_WALK_*.  A frame of an unsplit scene, k_finish (split: every mesh k_mesh leaves
 * to it), ptx_kat_geom_test, ptx_kat_compute_intersections and ptx_kat_tile_intersect with split = 0 search without a stack: PTX_WALK_LOOP
 * without a tree, PTX_WALK_SKIP with one.  Returns PTX_OK, or an error for a null argument or a geom that is not a mesh. */
#define PTX_WALK_LOOP 0        /* the reference's loop over all faces (fused into the bounce kernel, or in k_finish) */
#define PTX_WALK_SKIP 1        /* stackless walk over the skip links */
#define PTX_WALK_ORDERED 2     /* front-to-back walk of the binary tree */
#define PTX_WALK_WIDE 3        /* four-wide walk, one ray per lane from start to end */
#define PTX_WALK_WIDE_REFILL 4 /* four-wide walk under k_mesh's refilling schedule */
int ptx_debug_mesh_plan(ptx_tracer *t, int geom, int32_t out8[8]);
/* Debug: workgroups of the specialised later-bounce kernel that fit a CU with lds_bytes of dynamic LDS each (0: what this tracer launches). */
int ptx_debug_bounce_occupancy(ptx_tracer *t, int lds_bytes);
/* Host-only: the layout of the local index (the sort's output) this tracer's launches use.  out8 = { 1: bin-major, written in k_bounce's
 * tile loop / 0: chunk-compact, written by its tail; log2 N2; words allocated per entry; nbins * N2 (the bound an entry is checked
 * against); words of one segment's index; bytes per path and iteration the memory rule counted; the stage's slots; why not bin-major
 * (0: it is; 1 PTX_DEBUG_TAIL_INDEX, 2 split bounce, 3 more than 64 bins, 4 no direct epilogue, 5 offsets pass 32 bits, 6 memory rule) }. */
int ptx_debug_index_plan(ptx_tracer *t, int64_t out8[8]);
/* Debug: after waiting for the tracer's streams, the nonzero words left in the per-iteration "lit" bit-planes (out3[0]) and in the
 * per-bounce and group totals (out3[1]) of every lane's segments -- both 0 between launch sets, which clear what they read.  Segments
 * of a traced-ahead batch not yet gathered are not counted, nor are the lanes marked for a full clear before their next set (out3[2]). */
int ptx_debug_aux_nonzero(ptx_tracer *t, int64_t out3[3]);
/* Debug capture: the sorted stream of paths that will be shaded at bounce+1, as it stands after the given bounce
 * of the next iteration(s). */
int ptx_debug_set_capture(ptx_tracer *t, int bounce);   /* -1 = off */
/* CPU-only (no GPU call): the mesh BVH of csrc/pt_bvh.h against the reference's loop over all faces
   (src/intersections.h:213-233) on `nrays` object-space rays (6 floats: origin, direction).  stats4 = nodes, leaf
   triangles, nodes visited in total, rays on which the front-to-back traversal (the one k_mesh uses) disagrees with
   the skip-link traversal in face, distance or barycentrics (must be 0).  */
int ptx_debug_bvh_check(const float *faces15, int nfaces, const float *rays6, int nrays, int32_t *face_loop, float *t_loop,
                        int32_t *face_bvh, float *t_bvh, int64_t *stats4);
/* CPU-only: node visits of the last ptx_debug_bvh_check -- skip-link walk, front-to-back binary walk, four-wide walk (nodes),
   the stack entries the four-wide walk of that tree can need, the sum over groups of 64 consecutive rays of the longest four-wide
   walk in the group and the number of groups (what a wave of one-lane-per-ray walks costs), triangles tested by the four-wide walk;
   [7] unused */
int ptx_debug_bvh_visits(int64_t out8[8]);
/* zeros unless the library was built with -DPT_STAMPS (in-kernel phase timing, never in the shipped build) */
int ptx_debug_read_stamps(ptx_tracer *t, unsigned long long out48[48]);
/* fields14 (optional): 14 rows of min(n, cap) floats: px py pz (= origin + t*direction, the point that will be
 * shaded) dx dy dz cr cg cb nx ny nz u v (u, v only meaningful when the scene has textures) */
int ptx_debug_read_stream(ptx_tracer *t, int *n_out, int32_t *pixel_index, int32_t *stream_idx,
                          int32_t *material, float *fields14, int cap);

#ifdef __cplusplus
}
#endif
#endif
