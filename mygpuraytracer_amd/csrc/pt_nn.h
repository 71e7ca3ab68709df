// pt_nn.h -- internal interface of the network denoiser (pt_nn.hip: ptx_nn_* of include/mi355x_pathtracer.h) towards the tracer
// (pt_post.hip: ptx_denoise_nn, which needs the tracer's accumulation buffer, G-buffer, denoised frame and stream).  Not part of the C
// ABI; include/mi355x_pathtracer.h has the public side and the definition of the arithmetic.
//
// Device state of a handle:
//   per layer: the weights as fp16 in the convolution's fragment order (pack_weights) and the padded fp32 bias, written once at create
//   d_scratch: the activations of one tile (pt_nn_tiles.h: the whole frame, or the tile buffer of a handle made under a memory limit;
//              a smaller tile uses a prefix of each tensor), channels-last fp16, planned once at create: the network's input and the three pooled skips each in a
//              place of their own, every other tensor in one of two arenas that the layers write in turn (a layer reads one arena and
//              writes the other); dec_conv0's fp32 output, four floats per pixel, is the last tenant of the second arena
//              (`scratch` is where the handle's kernels find it: its own d_scratch, or -- a network of a prefilter handle -- the one
//              allocation the prefilter owns and both of its networks use in turn; DevBuf stays the one owner either way)
//   d_scale  : the scale the last input kernel used, written by it and read by the output kernel
//   meter    : a display handle for the block meter (hdr with automatic scale), made by the first call that needs it
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "pt_handle.h"
#include "pt_tza.h"
#include "pt_nn_tiles.h"
#include "pt_nn_progress.h"

struct ptx_display;

struct PtNnLayerDev {
    int cin0 = 0, cin1 = 0, cout = 0;             // the blob's counts
    int c0p = 0, c1p = 0, coutp = 0;              // padded to 16, the two sources separately
    int level = 0, src0 = -2, src1 = -2;
    bool relu = true, pool = false, upsample = false;
    DevBuf<uint16_t> w;                           // fp16 bits, fragment order
    DevBuf<float> b;
    size_t out_offset = 0;                        // of its output in d_scratch (bytes)
};

struct ptx_nn : PtHandle {
    int wp = 0, hp = 0, ic = 0;                   // the padded tile buffer (one tile: the padded frame), the network's input channels
    PtNnTiling tiling;                            // the frame's tiles (pt_nn_tiles.h); one tile unless made by ptx_nn_create_tiled
    PtNnLayerDev L[PT_NN_LAYERS];
    char names[PT_NN_LAYERS][16] = {};
    DevBuf<uint8_t> d_scratch;                    // empty where the scratch is another owner's
    uint8_t *scratch = nullptr;                   // not owned: d_scratch, or the prefilter's
    size_t scratch_bytes = 0;                     // the plan's (pt_nn_scratch of the tile buffer)
    size_t in_offset = 0;
    uint64_t macs = 0;                            // summed over the tiles
    DevBuf<float> d_scale;
    ptx_display *meter = nullptr;
    DevBuf<float> d_stage[4];                     // ptx_nn_denoise_host's rgb, albedo, normal, result (first use)
    // the image entry points' (pt_nn_image.hip), each on first need: the colour gathered for the meter and the in-place temporary,
    // W*H*3 floats each; ptx_nn_denoise_images_host's colour, albedo, normal and output (with the inputs that meet it), in bytes
    DevBuf<float> d_image_gather, d_image_tmp;
    DevBuf<uint8_t> d_image_stage[4];
    // the progress monitor (pt_nn_progress.h) and, made by the first call under one, the markers behind two tiles' stages and the copy-out
    PtNnProgress progress;
    std::vector<OwnedEvent> progress_ev;
    ~ptx_nn();
};

// NULL when the parameters are usable, else what is wrong with them (the ptx_last_error message)
const char *pt_nn_params_problem(const ptx_nn_params &p, float samples);

// One denoise on `st`: rgb = W*H*3 floats on the handle's device, divided by `samples`; alb / nrm with a stride of 3 or 4 floats per
// pixel (the tracer's G-buffer records are float4), NULL exactly when the network does not take them (the caller has checked).  Makes
// st wait for the handle's last work, enqueues the meter on the whole frame where the scale is automatic, then for every tile in
// row-major order the input kernel on its window, the sixteen convolutions and the output kernel on the rectangle it keeps, records the
// handle's event.  The caller has checked p and set the device, and with more than one tile that out_rgb overlaps no input.
int pt_nn_enqueue(ptx_nn *n, hipStream_t st, const float *rgb, float samples, const float *alb, int alb_stride, const float *nrm, int nrm_stride,
                  const ptx_nn_params &p, float *out_rgb);

// The per-tile loop of a denoise with the two end stages the caller's: for every tile in row-major order `input` on the tile's window
// (it writes the network's input record, [hp][wp][16] fp16, at net_in), the sixteen convolutions, `output` on the rectangle the tile
// keeps (it reads dec_conv0's [hp][wp][4] fp32 at net_out).  No wait and no record: those are the caller's, around one or more loops.
struct PtNnStages {
    void *ctx;
    int (*input)(void *ctx, hipStream_t st, const ptx_nn_tile &T, int wp, int hp, uint16_t *net_in);
    int (*output)(void *ctx, hipStream_t st, const ptx_nn_tile &T, int wp, const float *net_out);
};
int pt_nn_run_tiles(ptx_nn *n, hipStream_t st, const PtNnStages &stages);

// The progress monitor around one ptx_nn_denoise* call (`fn`).  begin: where the handle has a monitor and no call has begun yet, the
// first report (0, before anything is enqueued); *mine says that this call began it and ends it.  PTX_ERR_CANCELLED where the monitor
// cancels.  While a call has begun, pt_nn_run_tiles reports after every stage of every tile has finished and returns only then;
// pt_nn_progress_frame_unit does the same for what the caller has just enqueued on st behind the tiles (the copy-out).  A cancel waits
// for what is in flight on st.  end(mine, rc) hands rc back.  Without a monitor none of them enqueues, records or waits for anything.
int pt_nn_progress_begin(const char *fn, ptx_nn *n, bool copy_out, bool *mine);
int pt_nn_progress_frame_unit(ptx_nn *n, hipStream_t st);
int pt_nn_progress_end(ptx_nn *n, bool mine, int rc);

// ptx_nn_create_tiled's create path for a network whose scratch is `scratch`, the caller's allocation of at least the plan's bytes under
// this limit (pt_nn_scratch of pt_nn_tiling's tile buffer); max_memory_mb < 0: one tile, as ptx_nn_create.  `fn` names the entry point.
int pt_nn_create_shared(const char *fn, int device, int width, int height, const PtNnPlan &plan, int max_memory_mb, uint8_t *scratch, ptx_nn **out);
// what the create calls refuse without a device: the blob, the limit, the frame's size for this kind of handle
int pt_nn_blob_problem(const char *fn, const void *tza, size_t bytes, int width, int height, int max_memory_mb, PtNnPlan &plan);
int pt_nn_device_problem(const char *fn, int device);
int pt_nn_read_file(const char *fn, const char *path, std::vector<uint8_t> &blob);

// ---- the prefilter of the guides (pt_nn_aux.hip: ptx_nn_prefilter_* of include/mi355x_pathtracer.h) -------------------------------------
// Up to two 3-input networks, [0] for an albedo image and [1] for a normal image, that run one after the other in ONE activation
// scratch sized to the larger plan; per network a W*H*3 clean image.  The cache: the G-buffer serial (ptx_tracer::gbuf_serial), the
// params and the networks of the last ptx_denoise_nn_prefiltered; ptx_nn_prefilter_run_* and _invalidate forget it.
struct ptx_nn_prefilter : PtHandle {
    ptx_nn *net[2] = {nullptr, nullptr};
    DevBuf<uint8_t> d_scratch;
    DevBuf<float> d_clean[2];
    DevBuf<float> d_stage[2];                     // ptx_nn_prefilter_run_host's inputs (first use)
    uint64_t runs = 0;
    uint64_t cache_serial = 0;                    // 0: nothing cached
    int cache_mask = 0;                           // bit k: net[k] ran for that serial
    ptx_nn_prefilter_params cache_params = {};
    ~ptx_nn_prefilter();
};

const char *pt_nn_prefilter_params_problem(const ptx_nn_prefilter_params &p);
// The networks of `mask` (bit 0 albedo, bit 1 normal; each present in the handle) on st, between the handle's wait and record; an
// image with a stride of 3 or 4 floats per pixel, 16-byte aligned at a stride of 4.  The caller has checked p and set the device.
int pt_nn_prefilter_enqueue(ptx_nn_prefilter *pf, hipStream_t st, int mask, const float *alb, int alb_stride, const float *nrm, int nrm_stride,
                            const ptx_nn_prefilter_params &p);
