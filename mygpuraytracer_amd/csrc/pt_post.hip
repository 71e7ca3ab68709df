// pt_post.hip -- what happens to a tracer's frame after tracing, as host code: the ptx_* entry points that hand the tracer's buffers
// (pt_tracer.h) to the post-processing units -- the a-trous filter and its variance guidance (pt_denoise.hip), the temporal reprojection
// (pt_temporal.hip), the batch-means moments (pt_moments.hip), adaptive sampling (pt_adaptive.hip), the display transform
// (pt_display.hip) and the network denoiser (pt_nn.hip).  No __global__ function, no launch and no environment read: the kernels are
// those units', the G-buffer pass and the tile mask are pt_engine.hip's (pt_ensure_gbuffer, pt_set_tile_mask).  Errors go through
// pt_fail / PT_HC (pt_handle.h), which set the thread's ptx_last_error as pt_engine.hip's own do.
//
// The six ptx_denoise* entry points are one pipeline, denoise_run: each of them defaults its parameters, says in a DenoiseCall what it
// takes, and calls it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "../../include/mi355x_pathtracer.h"
#include "pt_tracer.h"
#include "pt_denoise.h"
#include "pt_adaptive.h"
#include "pt_display.h"
#include "pt_nn.h"
#include "pt_metrics.h"

namespace {

template <class P> P params_or_default(const P *given, void (*defaults)(P *)) {
    P p;
    if (given) p = *given;
    else defaults(&p);
    return p;
}

int bad_spp(const char *fn) {
    return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": spp must be >= 1 (the iterations summed in the accumulation buffer)");
}

// What the entry points that carry a history say while sampled guides are on ...
int guides_refuse_history(const char *fn, const ptx_tracer *t) {
    if (t->guide_count == 0)                             // ... or while the guides are followed through mirrors and glass
        return pt_fail(PTX_ERR_UNSUPPORTED, std::string(fn) + ": followed guides are on (ptx_set_guide_bounces, bounces > 0); reprojection and "
                                                 "history matching need the first surface -- set bounces 0 for the temporal path");
    return pt_fail(PTX_ERR_UNSUPPORTED, std::string(fn) + ": sampled guides are on (ptx_set_guide_samples, count > 0); reprojection and history "
                                             "matching need one surface per pixel -- set count 0 for the temporal path");
}

// A handle against the tracer it is used with: the tracer holds the whole frame, and the handle (`kind`: "temporal", "moments",
// "adaptive", "display") was made on its device and for its size.  same_tiles: the adaptive handle's tile count, part of its size.
int frame_handle_problem(const char *fn, const ptx_tracer *t, const char *kind, const PtHandle &x, bool same_tiles = true) {
    if (const int rc = pt_whole_frame_problem(fn, t)) return rc;
    if (x.device != t->device)
        return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": the " + kind + " handle was created on device " + std::to_string(x.device) +
                                            ", the tracer runs on device " + std::to_string(t->device));
    if (x.w != t->cam.resx || x.h != t->cam.resy || !same_tiles)
        return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": the " + kind + " handle's size " + std::to_string(x.w) + " x " + std::to_string(x.h) +
                                            " differs from the tracer's " + std::to_string(t->cam.resx) + " x " + std::to_string(t->cam.resy));
    return PTX_OK;
}
int moments_problem(const char *fn, const ptx_tracer *t, const ptx_moments *m) {
    return frame_handle_problem(fn, t, "moments", *m);
}
int adaptive_problem(const char *fn, const ptx_tracer *t, const ptx_adaptive *a) {
    return frame_handle_problem(fn, t, "adaptive", *a, a->ntiles == t->maxTiles);
}

const char *const TILED_HANDLE = "this moments handle has had a tiled add: its tiles hold different sample counts until ptx_moments_reset";

// The two handles count the same samples tile by tile, or the (k, W') table would not describe the moments' state.  k: the add's, with
// which no tile may pass 2^24 samples (0: no add).
int tile_samples_problem(const char *fn, const ptx_adaptive *a, const ptx_moments *m, int k) {
    for (int i = 0; i < a->ntiles; i++) {
        const long long have = m->tile_samples.empty() ? m->samples : m->tile_samples[(size_t)i];
        if (have != a->h_samples[(size_t)i])
            return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": tile " + std::to_string(i) + " holds " + std::to_string(a->h_samples[(size_t)i]) +
                                                " samples, the moments handle has " + std::to_string(have) + " of it: reset both together");
        if (k && (long long)a->h_samples[(size_t)i] + k > (1 << 24)) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": more than 2^24 samples in a tile");
    }
    return PTX_OK;
}

// The handle's step on the tracer's stream: wait for the handle's last work, start a new segment when the camera changed (cur becomes
// hist), then reproject hist into the current view and mix (with V when variance; moments: ptx_denoise_temporal_measured's V, from that
// state with its `batches`).
int temporal_step(ptx_tracer *t, ptx_temporal *h, const ptx_temporal_params &tp, int spp, bool variance, const PtMomentsState *moments,
                  int batches) {
    PT_HC(h->wait_stream(t->stream));
    ptx_camera cam;
    memcpy(&cam, &t->cam, sizeof cam);
    if (!h->cur_valid || memcmp(&cam, &h->cam[h->cur], sizeof cam) != 0) {
        if (h->cur_valid) { h->cur ^= 1; h->hist_valid = true; }
        h->cam[h->cur] = cam;
        h->cur_valid = true;
    }
    const int hi = h->cur ^ 1;
    const size_t n = (size_t)t->cam.resx * t->cam.resy;
    const float4 *g = t->d_gbuf;
    PtTemporalCamD camd;
    const PtTemporalCam hcam = pt_temporal_camera(h->cam[hi], h->hist_valid, &camd);
    PT_HC(pt_temporal_enqueue(t->stream, t->cam.resx, t->cam.resy, hcam, tp, t->d_image,
                              (float)spp, g, g + n, g + 2 * n, reinterpret_cast<const int2 *>(g + 3 * n), t->d_spec,
                              (int)t->h_spec.size(), h->st[h->cur], h->st[hi], h->d_mix, h->d_hn, variance ? 1 : 0,
                              variance && h->hist_valid && h->has_v[hi] ? 1 : 0, moments, batches, &camd));
    return PTX_OK;
}

// One call of the denoiser.  The kinds in the order the entry points came; from VARIANCE on the filter is the variance-guided one,
// from MEASURED on the call has a moments handle and a min_batches.
enum DenoiseKind { PLAIN, TEMPORAL, VARIANCE, MEASURED, TEMPORAL_MEASURED, ADAPTIVE };
struct DenoiseCall {
    DenoiseKind kind;
    const char *fn;                       // the entry point's name, for its messages
    const char *nulls;                    // ... and what it says when `missing`: one of the arguments it cannot do without is NULL
    bool missing;
    ptx_tracer *t;
    ptx_temporal *h;                      // TEMPORAL, TEMPORAL_MEASURED; VARIANCE: or NULL
    ptx_moments *m;                       // MEASURED, TEMPORAL_MEASURED, ADAPTIVE
    ptx_adaptive *a;                      // ADAPTIVE
    ptx_denoise_params dp;                // the three as the caller gave them or at their defaults; tp and vp where the kind has them
    ptx_temporal_params tp;
    ptx_variance_params vp;
    int min_batches, spp;                 // (ADAPTIVE has no spp: every tile has its own count)
};

// Every ptx_denoise* call: refuse what cannot run, in one order; the filter's buffers and the G-buffer; the filter's input on the
// tracer's stream, between the handles' events; the filter.
int denoise_run(const DenoiseCall &c) {
    const char *fn = c.fn;
    const bool takes_tp = c.kind == TEMPORAL || c.kind == VARIANCE || c.kind == TEMPORAL_MEASURED, variance = c.kind >= VARIANCE;
    if (const char *why = pt_denoise_params_problem(c.dp)) return pt_fail(PTX_ERR_INVALID, why);
    if (const char *why = takes_tp ? pt_temporal_params_problem(c.tp) : nullptr) return pt_fail(PTX_ERR_INVALID, why);
    if (const char *why = variance ? pt_variance_params_problem(c.vp) : nullptr) return pt_fail(PTX_ERR_INVALID, why);
    if (c.kind != ADAPTIVE && c.spp < 1) return bad_spp(fn);
    if (c.kind >= MEASURED && c.min_batches == 1) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": min_batches must be >= 2 (<= 0: the default, 4)");
    if (!c.dp.demodulate && (c.kind == TEMPORAL_MEASURED || (c.kind == VARIANCE && c.h)))
        return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": " + (c.kind == VARIANCE ? "with a temporal handle " : "") +
                                            "ptx_denoise_params.demodulate must be != 0 (the state's moments are in demodulated space)");
    if (c.missing) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": " + c.nulls);
    ptx_tracer *t = c.t;
    ptx_temporal *h = c.h;
    ptx_moments *m = c.m;
    ptx_adaptive *a = c.a;
    if (h && (t->guide_count > 0 || t->guide_bounces > 0)) return guides_refuse_history(fn, t);
    const int min_batches = c.min_batches <= 0 ? 4 : c.min_batches;
    if (a) {
        if (const int rc = moments_problem(fn, t, m)) return rc;
        if (const int rc = adaptive_problem(fn, t, a)) return rc;
        // the two handles count the same samples tile by tile (ptx_adaptive_add's comparison), and every tile holds some
        if (const int rc = tile_samples_problem(fn, a, m, 0)) return rc;
        if (m->samples == 0) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": no add on these handles yet");
        for (int i = 0; i < a->ntiles; i++)
            if (a->h_samples[(size_t)i] < 1) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": tile " + std::to_string(i) + " holds no sample");
    } else if (m) {
        if (m->samples == 0) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": no add on this moments handle yet");
        if (m->tiled) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": " + TILED_HANDLE);      // (one spp, one B per frame)
        if (const int rc = moments_problem(fn, t, m)) return rc;
        // too few batches for the measured variance: ptx_denoise_variance itself, so the same bits and, from here on, its name in the
        // messages (the moments state is not read: the handle is neither waited for nor marked)
        if (h && m->batches < min_batches) return ptx_denoise_variance(t, h, &c.dp, &c.tp, &c.vp, c.spp);
    }
    if (const int rc = h ? frame_handle_problem(fn, t, "temporal", *h) : pt_whole_frame_problem(fn, t)) return rc;

    // the buffers the filter needs, allocated on first use (d_var: by the variance-guided calls; the specular flags: by the first call
    // with a temporal handle), and the G-buffer of the current camera
    PT_HC(hipSetDevice(t->device));
    const int W = t->cam.resx, H = t->cam.resy;
    const size_t n = (size_t)W * H;
    if (!t->d_dn_tmp) PT_HC(t->d_dn_tmp.alloc(2 * n));
    if (!t->d_dn_out) PT_HC(t->d_dn_out.alloc(3 * n));
    if (variance && !t->d_var) PT_HC(t->d_var.alloc(2 * n));
    if (h && !t->d_spec) {
        PT_HC(t->d_spec.alloc(t->h_spec.size()));
        PT_HC(hipMemcpyAsync(t->d_spec, t->h_spec.data(), t->h_spec.size(), hipMemcpyHostToDevice, t->stream));
    }
    if (const int rc = pt_ensure_gbuffer(t)) return rc;
    const float4 *g = t->d_gbuf;
    const int2 *gids = reinterpret_cast<const int2 *>(g + 3 * n);
    const int demod = c.dp.demodulate ? 1 : 0;

    // the filter's input into d_dn_tmp.  The accumulation buffer is read on the tracer's stream, where every gather runs, those of
    // iterations traced ahead included.
    if (a) PT_HC(a->wait_stream(t->stream));
    if (m) PT_HC(m->wait_stream(t->stream));
    const enum { ACCUMULATED, HISTORY, MOMENTS, TILES } input = h ? HISTORY : c.kind == MEASURED ? MOMENTS : c.kind == ADAPTIVE ? TILES : ACCUMULATED;
    switch (input) {
    case ACCUMULATED:                                    // PLAIN, VARIANCE without a handle
        PT_HC(pt_atrous_prep_enqueue(t->stream, (int)n, t->d_image, (float)c.spp, g, g + 2 * n, demod, variance ? 1 : 0, nullptr, t->d_dn_tmp));
        break;
    case HISTORY: {                                      // TEMPORAL: the mix; VARIANCE with a handle, TEMPORAL_MEASURED: the state, with its V
        if (const int rc = temporal_step(t, h, c.tp, c.spp, variance, m ? &m->st : nullptr, m ? m->batches : 0)) return rc;
        if (m) PT_HC(m->record(t->stream));              // (the handle's next add, maybe on another stream, waits for this read)
        const PtTemporalState &cur = h->st[h->cur];
        if (!variance) PT_HC(pt_atrous_prep_enqueue(t->stream, (int)n, h->d_mix, 1.0f, g, g + 2 * n, demod, 0, nullptr, t->d_dn_tmp));
        // the spatial estimate where hist supplied no V (with the moments none: every hit pixel's dd.w is a V already, nothing is -1)
        else if (!m) PT_HC(pt_variance_spatial_enqueue(t->stream, W, H, c.dp, c.vp, cur.nh, cur.xn, cur.ids, 1, cur.dd));
        if (variance) PT_HC(pt_variance_prep_state_enqueue(t->stream, (int)n, cur, t->d_dn_tmp));
        h->has_v[h->cur] = variance;                     // false: dd.w = 0, a later ptx_denoise_variance takes its spatial estimate
        break;
    }
    case MOMENTS:
        PT_HC(pt_moments_prep_enqueue(t->stream, W, H, t->d_image, (float)c.spp, g, g + 2 * n, demod, m->st, min_batches, t->d_dn_tmp));
        PT_HC(m->record(t->stream));                     // (the handle's next add, maybe on another stream, waits for this read)
        break;
    case TILES:                                          // k_adaptive_prep in place of k_moments_prep, the rest as there
        PT_HC(pt_adaptive_prep_enqueue(t->stream, *a, t->d_image, g, g + 2 * n, demod, m->st, min_batches, t->d_dn_tmp));
        PT_HC(a->record(t->stream));                     // (the handle's frame was written: ptx_adaptive_read waits for it)
        PT_HC(m->record(t->stream));                     // (the handle's next add, maybe on another stream, waits for this read)
        break;
    }
    // the spatial estimate for the hit pixels the input left at -1
    if (variance && input != HISTORY) PT_HC(pt_variance_spatial_enqueue(t->stream, W, H, c.dp, c.vp, g, g + n, gids, 0, t->d_dn_tmp));

    if (variance) PT_HC(pt_atrous_enqueue(t->stream, W, H, g, g + n, g + 2 * n, t->d_dn_tmp, t->d_dn_tmp + n, t->d_dn_out, c.dp, &c.vp, t->d_var, t->d_var + n));
    else PT_HC(pt_atrous_enqueue(t->stream, W, H, g, g + n, g + 2 * n, t->d_dn_tmp, t->d_dn_tmp + n, t->d_dn_out, c.dp));
    if (h) {                                             // the handle's end of a call: its event after the call's work
        PT_HC(h->record(t->stream));
        h->done = true;
    }
    t->dn_done = true;
    if (variance) t->var_done = true;
    return PTX_OK;
}

}  // namespace

extern "C" {

// ---- denoiser (pt_denoise.hip, pt_temporal.hip, pt_moments.hip, pt_adaptive.hip; definitions in include/mi355x_pathtracer.h) ---------
int ptx_denoise(ptx_tracer *t, const ptx_denoise_params *params, int spp) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    if (spp < 1) return bad_spp("ptx_denoise");           // (this one looks at spp before the parameters)
    return denoise_run({PLAIN, "ptx_denoise", "", false, t, nullptr, nullptr, nullptr, params_or_default(params, ptx_default_denoise_params), {}, {}, 0, spp});
}

int ptx_denoise_temporal(ptx_tracer *t, ptx_temporal *h, const ptx_denoise_params *dparams, const ptx_temporal_params *tparams, int spp) {
    return denoise_run({TEMPORAL, "ptx_denoise_temporal", "null tracer or temporal handle", !t || !h, t, h, nullptr, nullptr,
                        params_or_default(dparams, ptx_default_denoise_params), params_or_default(tparams, ptx_default_temporal_params), {}, 0, spp});
}

int ptx_denoise_variance(ptx_tracer *t, ptx_temporal *h, const ptx_denoise_params *dparams, const ptx_temporal_params *tparams,
                         const ptx_variance_params *vparams, int spp) {
    return denoise_run({VARIANCE, "ptx_denoise_variance", "null tracer", !t, t, h, nullptr, nullptr,
                        params_or_default(dparams, ptx_default_denoise_params), params_or_default(tparams, ptx_default_temporal_params),
                        params_or_default(vparams, ptx_default_variance_params), 0, spp});
}

int ptx_denoise_measured(ptx_tracer *t, ptx_moments *m, const ptx_denoise_params *dparams, const ptx_variance_params *vparams, int min_batches,
                         int spp) {
    return denoise_run({MEASURED, "ptx_denoise_measured", "null tracer or moments handle", !t || !m, t, nullptr, m, nullptr,
                        params_or_default(dparams, ptx_default_denoise_params), {}, params_or_default(vparams, ptx_default_variance_params),
                        min_batches, spp});
}

// the two together: the temporal history's V pooled with the measured variance
int ptx_denoise_temporal_measured(ptx_tracer *t, ptx_temporal *h, ptx_moments *m, const ptx_denoise_params *dparams,
                                  const ptx_temporal_params *tparams, const ptx_variance_params *vparams, int min_batches, int spp) {
    return denoise_run({TEMPORAL_MEASURED, "ptx_denoise_temporal_measured", "null tracer, temporal handle or moments handle", !t || !h || !m, t, h, m,
                        nullptr, params_or_default(dparams, ptx_default_denoise_params), params_or_default(tparams, ptx_default_temporal_params),
                        params_or_default(vparams, ptx_default_variance_params), min_batches, spp});
}

// ptx_denoise_measured on a frame of unequal counts
int ptx_denoise_adaptive(ptx_tracer *t, ptx_adaptive *a, ptx_moments *m, const ptx_denoise_params *dparams, const ptx_variance_params *vparams,
                         int min_batches) {
    return denoise_run({ADAPTIVE, "ptx_denoise_adaptive", "null tracer, adaptive handle or moments handle", !t || !a || !m, t, nullptr, m, a,
                        params_or_default(dparams, ptx_default_denoise_params), {}, params_or_default(vparams, ptx_default_variance_params),
                        min_batches, 1});
}

int ptx_read_variance(ptx_tracer *t, float *input_var1, float *output_var1) {
    if (!t) return pt_fail(PTX_ERR_INVALID, "null tracer");
    if (!t->var_done) return pt_fail(PTX_ERR_INVALID, "ptx_read_variance: no ptx_denoise_variance on this tracer yet");
    PT_HC(hipSetDevice(t->device));
    const size_t n = (size_t)t->cam.resx * t->cam.resy;
    if (input_var1) PT_HC(hipMemcpyAsync(input_var1, t->d_var, sizeof(float) * n, hipMemcpyDeviceToHost, t->stream));
    if (output_var1) PT_HC(hipMemcpyAsync(output_var1, t->d_var + n, sizeof(float) * n, hipMemcpyDeviceToHost, t->stream));
    PT_HC(hipStreamSynchronize(t->stream));
    return PTX_OK;
}

int ptx_read_denoised(ptx_tracer *t, float *host_rgb) {
    if (!t || !host_rgb) return pt_fail(PTX_ERR_INVALID, "null argument");
    if (!t->dn_done) return pt_fail(PTX_ERR_INVALID, "ptx_read_denoised: no ptx_denoise on this tracer yet");
    PT_HC(hipSetDevice(t->device));
    PT_HC(hipMemcpyAsync(host_rgb, t->d_dn_out, sizeof(float) * 3 * (size_t)t->cam.resx * t->cam.resy, hipMemcpyDeviceToHost, t->stream));
    PT_HC(hipStreamSynchronize(t->stream));
    return PTX_OK;
}

float *ptx_device_denoised(ptx_tracer *t) { return t && t->dn_done ? t->d_dn_out : nullptr; }

// ---- network denoiser (pt_nn.hip; definition in include/mi355x_pathtracer.h) -----------------------------------------------------------
// Colour = the accumulation buffer over spp; albedo and normals = the G-buffer's float4 records in the guide mode that is set.  On the
// tracer's stream, the order ptx_denoise's read of the accumulation buffer has; the result is the tracer's denoised frame.
int ptx_denoise_nn(ptx_tracer *t, ptx_nn *nn, const ptx_nn_params *params, int spp) {
    const char *fn = "ptx_denoise_nn";
    const ptx_nn_params p = params_or_default(params, ptx_default_nn_params);
    if (spp < 1) return bad_spp(fn);
    if (const char *why = pt_nn_params_problem(p, (float)spp)) return pt_fail(PTX_ERR_INVALID, why);
    if (!t || !nn) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": null tracer or network handle");
    if (const int rc = frame_handle_problem(fn, t, "network", *nn)) return rc;
    PT_HC(hipSetDevice(t->device));
    const size_t n = (size_t)t->cam.resx * t->cam.resy;
    if (!t->d_dn_out) PT_HC(t->d_dn_out.alloc(3 * n));
    const float *alb = nullptr, *nrm = nullptr;
    if (nn->ic >= 6) {
        if (const int rc = pt_ensure_gbuffer(t)) return rc;
        const float4 *g = t->d_gbuf;
        alb = reinterpret_cast<const float *>(g + 2 * n);
        if (nn->ic >= 9) nrm = reinterpret_cast<const float *>(g);
    }
    if (const int rc = pt_nn_enqueue(nn, t->stream, t->d_image, (float)spp, alb, 4, nrm, 4, p, t->d_dn_out)) return rc;
    t->dn_done = true;
    return PTX_OK;
}

// The same with the guides prefiltered (pt_nn_aux.hip): the prefilter's networks on the G-buffer's arrays unless its clean images are
// of this G-buffer already (the serial pt_ensure_gbuffer stamps, the params, the networks that ran), then the main network with a
// clean image wherever pf has a network, all on the tracer's stream.
int ptx_denoise_nn_prefiltered(ptx_tracer *t, ptx_nn *nn, ptx_nn_prefilter *pf, const ptx_nn_params *params, const ptx_nn_prefilter_params *pparams,
                               int spp) {
    const char *fn = "ptx_denoise_nn_prefiltered";
    const ptx_nn_params p = params_or_default(params, ptx_default_nn_params);
    const ptx_nn_prefilter_params pp = params_or_default(pparams, ptx_default_nn_prefilter_params);
    if (spp < 1) return bad_spp(fn);
    if (const char *why = pt_nn_params_problem(p, (float)spp)) return pt_fail(PTX_ERR_INVALID, why);
    if (const char *why = pt_nn_prefilter_params_problem(pp)) return pt_fail(PTX_ERR_INVALID, why);
    if (!t || !nn || !pf) return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": null tracer, network handle or prefilter handle");
    if (const int rc = frame_handle_problem(fn, t, "network", *nn)) return rc;
    if (const int rc = frame_handle_problem(fn, t, "prefilter", *pf)) return rc;
    if (nn->ic < 6)
        return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": the main weights take 3 input channels: there is no guide to prefilter (ptx_denoise_nn)");
    if (nn->ic < 9 && !pf->net[0])
        return pt_fail(PTX_ERR_INVALID, std::string(fn) + ": the main weights take colour and albedo, and the prefilter handle has no albedo network");
    PT_HC(hipSetDevice(t->device));
    const size_t n = (size_t)t->cam.resx * t->cam.resy;
    if (!t->d_dn_out) PT_HC(t->d_dn_out.alloc(3 * n));
    if (const int rc = pt_ensure_gbuffer(t)) return rc;
    const float4 *g = t->d_gbuf;
    const float *raw_alb = reinterpret_cast<const float *>(g + 2 * n), *raw_nrm = reinterpret_cast<const float *>(g);
    const int mask = (pf->net[0] ? 1 : 0) | (pf->net[1] && nn->ic >= 9 ? 2 : 0);
    const bool cached = pf->cache_serial != 0 && pf->cache_serial == t->gbuf_serial && (pf->cache_mask & mask) == mask &&
                        memcmp(&pf->cache_params, &pp, sizeof pp) == 0;
    if (!cached) {
        pf->cache_serial = 0; pf->cache_mask = 0;
        if (const int rc = pt_nn_prefilter_enqueue(pf, t->stream, mask, raw_alb, 4, raw_nrm, 4, pp)) return rc;
        pf->cache_serial = t->gbuf_serial; pf->cache_mask = mask; pf->cache_params = pp;
    } else {
        PT_HC(pf->wait_stream(t->stream));                // (the clean images may have been written on another tracer's stream)
    }
    const bool clean_alb = (mask & 1) != 0, clean_nrm = (mask & 2) != 0;
    const float *alb = clean_alb ? pf->d_clean[0].p : raw_alb, *nrm = nn->ic >= 9 ? (clean_nrm ? pf->d_clean[1].p : raw_nrm) : nullptr;
    if (const int rc = pt_nn_enqueue(nn, t->stream, t->d_image, (float)spp, alb, clean_alb ? 3 : 4, nrm, clean_nrm ? 3 : 4, p, t->d_dn_out)) return rc;
    PT_HC(pf->record(t->stream));                         // the handle's next run waits for this read of its clean images
    t->dn_done = true;
    return PTX_OK;
}

// ---- sample moments by batch means (pt_moments.hip; definition in include/mi355x_pathtracer.h) ---------------------------------------
// The accumulation buffer is read on the tracer's stream, where every gather runs, those of iterations traced ahead included
// (ahead_finish_segment): the order ptx_denoise's read of it has.
int ptx_moments_add(ptx_moments *m, ptx_tracer *t, int64_t samples_total) {
    if (samples_total < 1) return pt_fail(PTX_ERR_INVALID, "ptx_moments_add: samples_total must be >= 1");
    if (!m || !t) return pt_fail(PTX_ERR_INVALID, "ptx_moments_add: null moments handle or tracer");
    if (samples_total <= m->samples)
        return pt_fail(PTX_ERR_INVALID, "ptx_moments_add: samples_total " + std::to_string(samples_total) + " does not exceed the last add's " +
                                            std::to_string(m->samples));
    if (m->tiled) return pt_fail(PTX_ERR_INVALID, "ptx_moments_add: " + std::string(TILED_HANDLE));
    if (samples_total > (1 << 24))                       // (W and k are held as floats: exact to 2^24)
        return pt_fail(PTX_ERR_INVALID, "ptx_moments_add: samples_total " + std::to_string(samples_total) + " is above 2^24");
    if (const int rc = moments_problem("ptx_moments_add", t, m)) return rc;
    PT_HC(hipSetDevice(t->device));
    PT_HC(m->wait_stream(t->stream));
    PT_HC(pt_moments_add_enqueue(t->stream, m->w, m->h, t->d_image, (float)(samples_total - m->samples), (float)samples_total,
                                 m->samples == 0, m->st));
    PT_HC(m->record(t->stream));
    m->samples = samples_total;
    m->batches++;
    return PTX_OK;
}

// ---- adaptive sampling by tiles (pt_adaptive.hip; definition in include/mi355x_pathtracer.h) ------------------------------------------
int ptx_adaptive_add(ptx_adaptive *a, ptx_moments *m, ptx_tracer *t, int k) {
    if (k < 1 || k > (1 << 24)) return pt_fail(PTX_ERR_INVALID, "ptx_adaptive_add: k must be in 1 .. 2^24");
    if (!a || !m || !t) return pt_fail(PTX_ERR_INVALID, "ptx_adaptive_add: null adaptive handle, moments handle or tracer");
    if (const int rc = moments_problem("ptx_adaptive_add", t, m)) return rc;
    if (const int rc = adaptive_problem("ptx_adaptive_add", t, a)) return rc;
    if (const int rc = tile_samples_problem("ptx_adaptive_add", a, m, k)) return rc;
    PT_HC(hipSetDevice(t->device));
    PT_HC(a->wait_stream(t->stream));
    PT_HC(m->wait_stream(t->stream));
    PT_HC(pt_adaptive_advance_enqueue(t->stream, *a, k));
    for (int i = 0; i < a->ntiles; i++) {
        a->h_k[(size_t)i] = a->h_active[(size_t)i] ? k : 0;
        a->h_samples[(size_t)i] += a->h_k[(size_t)i];
    }
    const int rc = pt_moments_add_tiled(m, t->stream, t->d_image, a->d_kt, a->h_k.data());
    PT_HC(a->record(t->stream));
    PT_HC(m->record(t->stream));
    return rc;
}

int ptx_adaptive_select(ptx_adaptive *a, ptx_moments *m, ptx_tracer *t, const ptx_adaptive_params *params, ptx_adaptive_status *status) {
    const ptx_adaptive_params p = params_or_default(params, ptx_default_adaptive_params);
    if (const char *why = pt_adaptive_params_problem(p)) return pt_fail(PTX_ERR_INVALID, why);
    if (!a || !m || !t || !status) return pt_fail(PTX_ERR_INVALID, "ptx_adaptive_select: null adaptive handle, moments handle, tracer or status");
    if (m->samples == 0) return pt_fail(PTX_ERR_INVALID, "ptx_adaptive_select: no add on this moments handle yet");
    if (const int rc = moments_problem("ptx_adaptive_select", t, m)) return rc;
    if (const int rc = adaptive_problem("ptx_adaptive_select", t, a)) return rc;
    int code = 0;
    if (const char *why = pt_active_tiles_problem(t, a->ntiles, code)) return pt_fail(code, std::string("ptx_adaptive_select: ") + why);
    PT_HC(hipSetDevice(t->device));
    PT_HC(a->wait_stream(t->stream));
    PT_HC(m->wait_stream(t->stream));
    PT_HC(pt_adaptive_select_enqueue(t->stream, *a, m->st, p, a->rounds + 1));
    PT_HC(m->record(t->stream));                         // (the handle's next add, maybe on another stream, waits for this read)
    const size_t bytes = sizeof(ptx_adaptive_status) + (size_t)a->ntiles;
    PT_HC(hipMemcpyAsync(a->h_out, a->d_out, bytes, hipMemcpyDeviceToHost, t->stream));      // the one small read: status and flags
    const int rc = pt_set_tile_mask(t, a->d_active());   // (waits for the stream: h_out is there)
    PT_HC(a->record(t->stream));                         // behind k_tile_mask, which reads the flags
    if (rc != PTX_OK) return rc;
    a->rounds++;
    memcpy(status, a->h_out, sizeof *status);
    memcpy(a->h_active.data(), a->h_out + sizeof(ptx_adaptive_status), (size_t)a->ntiles);
    return PTX_OK;
}

int ptx_adaptive_resolve(ptx_adaptive *a, ptx_tracer *t) {
    if (!a || !t) return pt_fail(PTX_ERR_INVALID, "ptx_adaptive_resolve: null adaptive handle or tracer");
    if (const int rc = adaptive_problem("ptx_adaptive_resolve", t, a)) return rc;
    PT_HC(hipSetDevice(t->device));
    PT_HC(a->wait_stream(t->stream));
    PT_HC(pt_adaptive_resolve_enqueue(t->stream, *a, t->d_image));
    PT_HC(a->record(t->stream));
    return PTX_OK;
}

// ---- display transform (pt_display.hip; definition in include/mi355x_pathtracer.h) -------------------------------------------------
// Meter + map on the tracer's stream, where every gather and the denoiser run.
int ptx_display_tracer(ptx_display *d, ptx_tracer *t, int source, int spp, const ptx_display_params *params, void *device_uchar4) {
    ptx_display_params p = params_or_default(params, ptx_default_display_params);
    if (source != PTX_DISPLAY_IMAGE && source != PTX_DISPLAY_DENOISED)
        return pt_fail(PTX_ERR_INVALID, "ptx_display_tracer: source must be PTX_DISPLAY_IMAGE or PTX_DISPLAY_DENOISED");
    const float samples = source == PTX_DISPLAY_IMAGE ? (float)spp : 1.f;
    if (source == PTX_DISPLAY_IMAGE && spp < 1) return bad_spp("ptx_display_tracer");
    if (const char *why = pt_display_params_problem(p, samples)) return pt_fail(PTX_ERR_INVALID, why);
    if (!d || !t) return pt_fail(PTX_ERR_INVALID, "ptx_display_tracer: null display handle or tracer");
    if (const int rc = frame_handle_problem("ptx_display_tracer", t, "display", *d)) return rc;
    if (source == PTX_DISPLAY_DENOISED && !t->dn_done) return pt_fail(PTX_ERR_INVALID, "ptx_display_tracer: no ptx_denoise on this tracer yet");
    PT_HC(hipSetDevice(t->device));
    return pt_display_enqueue(d, t->stream, source == PTX_DISPLAY_IMAGE ? (const float *)t->d_image : (const float *)t->d_dn_out, samples, p,
                              device_uchar4);
}

// ---- image metrics (pt_metrics.hip; definition in include/mi355x_pathtracer.h) -------------------------------------------------------
// The tracer's frame against a host reference, on the tracer's stream: reads the accumulation buffer or the denoised frame, writes
// only the handle's own buffers.
int ptx_metrics_tracer(ptx_metrics *m, ptx_tracer *t, int source, int spp, const ptx_nn_image *b, const ptx_metrics_params *params,
                       ptx_metrics_result *out) {
    ptx_metrics_params p = params_or_default(params, ptx_default_metrics_params);
    if (source != PTX_DISPLAY_IMAGE && source != PTX_DISPLAY_DENOISED)
        return pt_fail(PTX_ERR_INVALID, "ptx_metrics_tracer: source must be PTX_DISPLAY_IMAGE or PTX_DISPLAY_DENOISED");
    if (source == PTX_DISPLAY_IMAGE && spp < 1) return bad_spp("ptx_metrics_tracer");
    p.samples_a = source == PTX_DISPLAY_IMAGE ? (float)spp : 1.f;
    if (!m || !t || !out) return pt_fail(PTX_ERR_INVALID, "ptx_metrics_tracer: null metrics handle, tracer or result");
    if (out->struct_size < sizeof(size_t)) return pt_fail(PTX_ERR_INVALID, "ptx_metrics_tracer: ptx_metrics_result.struct_size is not set");
    PtNnImageView va, vb, db;
    if (const int rc = pt_metrics_problem("ptx_metrics_tracer", m->w, m->h, nullptr, false, b, p, &va, &vb)) return rc;
    if (const int rc = frame_handle_problem("ptx_metrics_tracer", t, "metrics", *m)) return rc;
    if (source == PTX_DISPLAY_DENOISED && !t->dn_done) return pt_fail(PTX_ERR_INVALID, "ptx_metrics_tracer: no ptx_denoise on this tracer yet");
    PT_HC(hipSetDevice(t->device));
    if (const int rc = pt_metrics_stage(m, 1, vb, &db)) return rc;
    va.base = (uintptr_t)(source == PTX_DISPLAY_IMAGE ? (const float *)t->d_image : (const float *)t->d_dn_out);
    va.format = PTX_NN_FORMAT_FLOAT3; va.pixel_stride = 12; va.row_stride = 12 * (size_t)m->w;
    return pt_metrics_compare(m, t->stream, va, db, p, out, nullptr);
}

}  // extern "C"
