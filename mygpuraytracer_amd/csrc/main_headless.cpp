// main_headless.cpp -- the reference's main.cpp/preview.cpp without the window (src/main.cpp:36-152):
// load the scene, recompute the camera as the first runCuda() does, pathtraceFree/pathtraceInit, run
// state.iterations iterations of pathtrace, print "time: <ms>" (sum of the bounce-loop timer, main.cpp:141-146) and
// save <FILE>.<utc>.<n>samp.png with saveImage's mirroring (main.cpp:81-102).
//
//   mi355x_pathtrace SCENEFILE.txt [--res W H] [--depth D] [--iterations N] [--out PREFIX] [--pfm] [--hdr]
//                                  [--no-aa] [--dof] [--no-sort] [--no-cache] [--device K] [--arith 0|1|2]   (ptx_options.arith: 0 exact, the default)
//                                  [--checkpoint FILE [--checkpoint-every N]] [--resume FILE]
//                                  [--orbit "left:DX,DY;right:DY;middle:DX,DY;space"]   (the mouse of main.cpp:166-212, scripted)
//                                  [--per-call [--no-render-ahead]]   (one pathtrace(pbo, frame, iter) per iteration with the frame read
//                                                                      back after each, exactly the reference's runCuda loop)
//                                  [--denoise [--denoise-passes N]]   (also <out>.denoised.png / .pfm: the a-trous denoiser, ptx_denoise)
//                                  [--frames K --frame-step "left:DX,DY;..."]   (K frames of an orbit: frame f applies the --orbit
//                                                                      script, then the step script f-1 times, and runs the reference's
//                                                                      camera-change loop: pathtraceFree/Init, --iterations N pathtrace
//                                                                      calls, GPUdenoise with --denoise; <out>.fNNN.png [.denoised.png])
//                                  [--temporal]   (with --denoise: GPUdenoise reuses the previous frame's samples, ptx_denoise_temporal)
//                                  [--variance [--phi-luminance X]]   (with --denoise: the variance-guided filter, ptx_denoise_variance;
//                                                                      combines with --temporal and --frames)
//                                  [--until-error E [--error-floor F]]   (render in batches of 16 iterations, one ptx_moments_add after
//                                                                      each; stop at the first check with mean_rel_se <= E, or at
//                                                                      --iterations; F = ptx_moments_params.floor; not with --frames)
//                                  [--adaptive E [--measure-every K] [--error-floor F]]   (adaptive sampling by tiles, ptx_adaptive_*: render
//                                                                      in batches of K iterations (16), after each stop tracing the tiles of
//                                                                      256 pixels whose error is at E; ends when no tile is left, or at
//                                                                      --iterations.  One line per round, a closing line against the uniform
//                                                                      render that gives every tile the worst tile's count; the frame saved is
//                                                                      the one normalised tile by tile.  Not with --frames, --per-call,
//                                                                      --checkpoint, --until-error or --denoise.)
//                                  [--adaptive-denoise [--denoise-passes N] [--phi-luminance X]]   (with --adaptive E: also
//                                                                      <out>.denoised.png / .pfm, the variance-guided filter on that frame
//                                                                      with the variance the rounds measured, every tile with its own count:
//                                                                      ptx_denoise_adaptive)
//                                  [--measured [--measure-every K]]   (with --denoise: the variance-guided filter on the variance the
//                                                                      run measured, ptx_denoise_measured: a batch every K iterations,
//                                                                      16 unless given.  Implies --variance.  With --frames the moments
//                                                                      start again at every view; with --temporal as well the history's
//                                                                      variance is pooled with them, ptx_denoise_temporal_measured.  A view
//                                                                      that ends with fewer than 4 batches falls back to the unmeasured
//                                                                      estimate and says so.)
//                                  [--guide-samples K]   (with --denoise -- plain, --variance, --measured -- or --adaptive E --adaptive-denoise:
//                                                                      the filter's guides averaged over the camera rays of iterations
//                                                                      1 .. min(K, iterations), jitter and lens included, instead of the
//                                                                      pixel-centre pinhole ray: ptx_set_guide_samples.  Not with --temporal.)
//                                  [--guide-bounces B]   (with the same: every guide ray followed through at most B mirrors / glass surfaces to the
//                                                                      surface seen in them: ptx_set_guide_bounces.  Not with --temporal.)
//                                  [--compare REF.pfm [--compare-denoised] [--compare-transform none|srgb|hdr|snorm] [--compare-exposure E]
//                                   [--compare-threshold T]]   (after the render: the frame on the device -- with --compare-denoised the
//                                                                      denoised one -- against REF.pfm, a file as --pfm writes them, read
//                                                                      back by the writer's own rule; one line `metrics: {json}`:
//                                                                      ptx_metrics_tracer.  Not with --frames or --adaptive.)
//   mi355x_pathtrace --compare-files A.pfm B.pfm [--compare-transform ..] [--compare-exposure E] [--compare-threshold T] [--device K]
//                                                                     (no scene: A against the reference B, the same line)
//                                  [--tonemap clamp|reinhard|aces] [--exposure auto|<scale>] [--srgb] [--dither] [--adapt A]   (the display
//                                                                      transform, ptx_display_*: when any is given, every .png and
//                                                                      .denoised.png takes its bytes from it -- automatic exposure from block
//                                                                      luminances (auto, the default once a flag is given) or a fixed scale, a
//                                                                      tone curve (aces unless named), the sRGB transfer with --srgb, rounding
//                                                                      to the nearest code, with an ordered dither with --dither; A in (0, 1] is the share of the way
//                                                                      to the metered exposure taken per frame with --frames.  One line per file
//                                                                      with the metered and applied exposure.  .pfm, .hdr and checkpoints are
//                                                                      untouched; without these flags every file is what it was.)
//
// RES / DEPTH / ITERATIONS overrides and the four switches are what the reference can only change by editing the
// scene file or the #defines of src/pathtrace.cu:36-40.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <sstream>
#include <algorithm>
#include <string>
#include <vector>

#include "pathtrace_api.h"
#include "pt_image.h"

static std::string currentTimeString() {          // src/preview.cpp:13-19
    time_t now;
    time(&now);
    char buf[sizeof "0000-00-00_00-00-00z"];
    strftime(buf, sizeof buf, "%Y-%m-%d_%H-%M-%Sz", gmtime(&now));
    return std::string(buf);
}

// The display transform of the --tonemap / --exposure / --srgb / --dither / --adapt flags: a handle for the frames and one for the
// denoised frames (each adapts to its own sequence), created on first use.
struct DisplayOut {
    bool on = false;
    int device = 0;
    ptx_display_params params;
    ptx_display *handle[2] = {nullptr, nullptr};
    std::vector<uint8_t> rgba;
    // rgb8 as to_rgb8_mirrored lays it out, from the display stage's codes for sum_rgb / samples; false (message printed) on failure
    bool rgb8_mirrored(int which, int w, int h, const float *sum_rgb, float samples, const std::string &file, std::vector<uint8_t> &out) {
        if (!handle[which] && ptx_display_create(device, w, h, &handle[which]) != PTX_OK) { fprintf(stderr, "display failed: %s\n", ptx_last_error()); return false; }
        rgba.resize((size_t)w * h * 4);
        ptx_display_status st;
        if (ptx_display_host(handle[which], sum_rgb, samples, &params, rgba.data()) != PTX_OK || ptx_display_get_status(handle[which], &st) != PTX_OK) {
            fprintf(stderr, "display failed: %s\n", ptx_last_error());
            return false;
        }
        out.resize((size_t)w * h * 3);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                for (int k = 0; k < 3; k++) out[((size_t)(w - 1 - x) + (size_t)y * w) * 3 + k] = rgba[((size_t)x + (size_t)y * w) * 4 + k];
        if (params.meter == PTX_METER_BLOCKS)
            printf("display %s: metered exposure %.6g, applied %.6g (x %g), %d of %d blocks\n", file.c_str(), (double)st.metered, (double)st.applied,
                   (double)params.exposure, (int)st.blocks_used, (int)st.blocks_total);
        else
            printf("display %s: manual exposure %.6g (nothing metered)\n", file.c_str(), (double)params.exposure);
        return true;
    }
    void release() { ptx_display_destroy(handle[0]); ptx_display_destroy(handle[1]); handle[0] = handle[1] = nullptr; }
};
static DisplayOut g_display;

// a frame's 8-bit pixels as the file takes them: the reference's preview rule, or the display stage when its flags are given
static bool frame_rgb8(int which, int w, int h, const float *sum_rgb, float samples, const std::string &file, std::vector<uint8_t> &out) {
    if (g_display.on) return g_display.rgb8_mirrored(which, w, h, sum_rgb, samples, file, out);
    ptimg::to_rgb8_mirrored(w, h, sum_rgb, samples, out);
    return true;
}

// --frames: the camera-change loop of apps/src/main.cpp:221-271 over an orbit, one tracer per frame, the denoiser's history (with
// --temporal) kept across them by the veneer.  measured: one batch of moments after every measure_every-th pathtrace() of a view
// (pathtraceInit starts them again), and GPUdenoise filters with them.
static int run_frames(Scene *scene, int frames, const std::string &orbit_script, const std::string &frame_step, const std::string &out_prefix,
                      bool denoise, bool temporal, bool variance, bool measured, int measure_every, bool pfm) {
    denoiseTemporal() = temporal;
    denoiseVariance() = variance || measured;
    if (measured) momentsBatch() = measure_every;
    const Camera base = scene->state.camera;
    const int width = base.resolution[0], height = base.resolution[1], n = (int)scene->state.iterations;
    if (n < 1) { fprintf(stderr, "--frames needs --iterations N >= 1\n"); return 1; }
    const std::string prefix = out_prefix.empty() ? scene->state.imageName : out_prefix;
    std::string script = orbit_script;
    std::vector<uint8_t> rgb8;
    for (int f = 1; f <= frames; f++) {
        if (f > 1) script += ";" + frame_step;
        scene->state.camera = base;
        if (!scene->runOrbitScript(script)) { fprintf(stderr, "bad --orbit / --frame-step script: %s\n", script.c_str()); return 1; }
        pathtraceFree();                         // the camera changed: iteration = 0, a new tracer (main.cpp:229-240)
        pathtraceInit(scene);
        for (int it = 1; it <= n; it++) pathtrace(nullptr, 0, it);
        char tag[16];
        snprintf(tag, sizeof tag, ".f%03d", f);
        const std::string name = prefix + tag;
        if (!frame_rgb8(0, width, height, &scene->state.image[0].x, (float)n, name + ".png", rgb8)) return 1;
        if (!ptimg::write_png_rgb8(name + ".png", width, height, rgb8.data())) { fprintf(stderr, "cannot write %s.png\n", name.c_str()); return 1; }
        printf("Saved %s.png.\n", name.c_str());
        if (pfm) { ptimg::write_pfm(name + ".pfm", width, height, &scene->state.image[0].x, (float)n); printf("Saved %s.pfm.\n", name.c_str()); }
        if (denoise) {
            const int nbatches = measured ? n / measure_every : 0;
            if (measured && nbatches < 4)
                printf("frame %d: %d batch(es) of %d iterations, fewer than 4: fell back to the unmeasured variance estimate\n", f, nbatches,
                       measure_every);
            denoiseMeasured() = nbatches > 0;    // (no batch at all: there is no moments handle to hand over)
            GPUdenoise();                        // state.output = the denoised mean radiance
            if (!frame_rgb8(1, width, height, &scene->state.output[0].x, 1.0f, name + ".denoised.png", rgb8)) return 1;
            if (!ptimg::write_png_rgb8(name + ".denoised.png", width, height, rgb8.data())) { fprintf(stderr, "cannot write %s.denoised.png\n", name.c_str()); return 1; }
            printf("Saved %s.denoised.png.\n", name.c_str());
            if (pfm) { ptimg::write_pfm(name + ".denoised.pfm", width, height, &scene->state.output[0].x, 1.0f); printf("Saved %s.denoised.pfm.\n", name.c_str()); }
        }
    }
    g_display.release();
    GPUdenoiseRelease();
    pathtraceFree();
    delete scene;
    return 0;
}

// --compare / --compare-files: the image metrics (ptx_metrics_*) as one line `metrics: {json}`; NaN, Infinity and -Infinity as Python's
// json module reads them.
struct CompareFlags {
    std::string ref, file_a, file_b;
    bool denoised = false;
    ptx_metrics_params params;
};
static bool compare_flag(CompareFlags &c, const std::string &a, int argc, char **argv, int &i) {
    auto need = [&](int n) { if (i + n >= argc) { fprintf(stderr, "%s needs %d value(s)\n", a.c_str(), n); exit(1); } };
    if (a == "--compare") { need(1); c.ref = argv[++i]; }
    else if (a == "--compare-denoised") c.denoised = true;
    else if (a == "--compare-transform") {
        need(1);
        const std::string v = argv[++i];
        c.params.transform = v == "none" ? PTX_METRICS_NONE : v == "srgb" ? PTX_METRICS_SRGB : v == "hdr" ? PTX_METRICS_HDR : v == "snorm" ? PTX_METRICS_SNORM : -1;
        if (c.params.transform < 0) { fprintf(stderr, "--compare-transform needs none, srgb, hdr or snorm\n"); exit(1); }
    }
    else if (a == "--compare-exposure") { need(1); c.params.exposure = (float)atof(argv[++i]); }
    else if (a == "--compare-threshold") { need(1); c.params.threshold = (float)atof(argv[++i]); }
    else return false;
    return true;
}
static std::string json_number(double v) {
    if (v != v) return "NaN";
    if (v > 1.7976931348623157e308) return "Infinity";
    if (v < -1.7976931348623157e308) return "-Infinity";
    char buf[40];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}
static void print_metrics(const ptx_metrics_result &r) {
    std::ostringstream o;
    auto triple = [&](const double *v) { return "[" + json_number(v[0]) + ", " + json_number(v[1]) + ", " + json_number(v[2]) + "]"; };
    o << "{\"mse\": " << json_number(r.mse) << ", \"psnr\": " << json_number(r.psnr) << ", \"l1\": " << json_number(r.l1) << ", \"mape\": "
      << json_number(r.mape) << ", \"smape\": " << json_number(r.smape) << ", \"grad\": " << json_number(r.grad) << ", \"l1_msssim\": "
      << json_number(r.l1_msssim) << ", \"ssim\": " << json_number(r.ssim) << ", \"msssim\": " << json_number(r.msssim) << ", \"ssim_c\": "
      << triple(r.ssim_c) << ", \"msssim_c\": " << triple(r.msssim_c) << ", \"mcs\": [";
    for (int s = 0; s < PTX_METRICS_SCALES; s++) o << (s ? ", " : "") << triple(r.mcs[s]);
    o << "], \"max_error\": " << json_number(r.max_error) << ", \"num_errors\": " << (unsigned long long)r.num_errors << ", \"nonfinite_a\": "
      << (unsigned long long)r.nonfinite_a << ", \"nonfinite_b\": " << (unsigned long long)r.nonfinite_b << ", \"exposure\": "
      << json_number((double)r.exposure) << ", \"valid\": " << r.valid << "}";
    printf("metrics: %s\n", o.str().c_str());
}
static ptx_nn_image packed_image(const std::vector<float> &rgb) {
    ptx_nn_image img = ptx_nn_image();
    img.ptr = rgb.data();
    img.format = PTX_NN_FORMAT_FLOAT3;
    return img;
}
// --compare-files A.pfm B.pfm: a against the reference b, no scene -- the counterpart of OIDN's training/compare_image.py
static int compare_files(const CompareFlags &c, int device) {
    std::vector<float> a, b;
    int wa, ha, wb, hb;
    std::string why;
    if (!ptimg::read_pfm(c.file_a, wa, ha, a, why) || !ptimg::read_pfm(c.file_b, wb, hb, b, why)) { fprintf(stderr, "%s\n", why.c_str()); return 1; }
    if (wa != wb || ha != hb) { fprintf(stderr, "--compare-files: %s is %d x %d, %s is %d x %d\n", c.file_a.c_str(), wa, ha, c.file_b.c_str(), wb, hb); return 1; }
    ptx_metrics *m = nullptr;
    ptx_metrics_result r = ptx_metrics_result();
    r.struct_size = sizeof r;
    const ptx_nn_image ia = packed_image(a), ib = packed_image(b);
    const bool ok = ptx_metrics_create(device, wa, ha, &m) == PTX_OK && ptx_metrics_compare_host(m, &ia, &ib, &c.params, &r, nullptr) == PTX_OK;
    ptx_metrics_destroy(m);
    if (!ok) { fprintf(stderr, "compare failed: %s\n", ptx_last_error()); return 1; }
    print_metrics(r);
    return 0;
}

int main(int argc, char **argv) {
    const std::string startTimeString = currentTimeString();
    if (argc < 2 || !strcmp(argv[1], "--help")) {
        printf("Usage: %s SCENEFILE.txt [--res W H] [--depth D] [--iterations N] [--out PREFIX] [--pfm] [--hdr] [--no-aa] [--dof] [--no-sort] [--no-cache] [--device K] [--arith 0|1|2] [--checkpoint FILE [--checkpoint-every N]] [--resume FILE] [--orbit SCRIPT] [--per-call [--no-render-ahead]] [--denoise [--denoise-passes N]] [--frames K --frame-step SCRIPT] [--temporal] [--variance [--phi-luminance X]] [--until-error E [--error-floor F]] [--measured [--measure-every K]] [--adaptive E [--measure-every K] [--error-floor F] [--adaptive-denoise [--denoise-passes N] [--phi-luminance X]]] [--guide-samples K] [--guide-bounces B] [--tonemap clamp|reinhard|aces] [--exposure auto|<scale>] [--srgb] [--dither] [--adapt A] [--compare REF.pfm [--compare-denoised] [--compare-transform none|srgb|hdr|snorm] [--compare-exposure E] [--compare-threshold T]]\n       %s --compare-files A.pfm B.pfm [--compare-transform ..] [--compare-exposure E] [--compare-threshold T] [--device K]\n", argv[0], argv[0]);
        return argc < 2;
    }
    CompareFlags cmp;
    ptx_default_metrics_params(&cmp.params);
    if (!strcmp(argv[1], "--compare-files")) {   // no scene: mi355x_pathtrace --compare-files A.pfm B.pfm [--compare-transform ..] [--device K]
        if (argc < 4) { fprintf(stderr, "--compare-files needs A.pfm B.pfm\n"); return 1; }
        cmp.file_a = argv[2]; cmp.file_b = argv[3];
        int device = 0;
        for (int i = 4; i < argc; i++) {
            const std::string a = argv[i];
            if (a == "--device" && i + 1 < argc) device = atoi(argv[++i]);
            else if (!compare_flag(cmp, a, argc, argv, i) || !cmp.ref.empty() || cmp.denoised) { fprintf(stderr, "unknown option %s with --compare-files\n", a.c_str()); return 1; }
        }
        return compare_files(cmp, device);
    }
    int resw = 0, resh = 0, depth = 0, iterations = 0;
    bool pfm = false, hdr = false, per_call = false, denoise = false, temporal = false, variance = false, measured = false, adaptive_denoise = false;
    double until_error = -1.0, adaptive = -1.0;
    ptx_moments_params mparams;
    ptx_default_moments_params(&mparams);
    ptx_denoise_params &dparams = denoiseParams();
    std::string out_prefix, ckpt_path, resume_path, orbit_script, frame_step, nn_path, nn_albedo_path, nn_normal_path;
    int ckpt_every = 0, frames = 0, measure_every = 16, guide_samples = 0, guide_bounces = 0, nn_max_memory = 0;
    bool nn_max_memory_set = false;
    ptx_options &opt = pathtraceOptions();
    ptx_display_params &disp = g_display.params;
    ptx_default_display_params(&disp);
    disp.transfer = PTX_TRANSFER_LINEAR;         // the library's defaults (metered exposure, ACES, rounding) but for the transfer: --srgb names it
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto need = [&](int n) { if (i + n >= argc) { fprintf(stderr, "%s needs %d value(s)\n", a.c_str(), n); exit(1); } };
        if (a == "--res") { need(2); resw = atoi(argv[++i]); resh = atoi(argv[++i]); }
        else if (a == "--depth") { need(1); depth = atoi(argv[++i]); }
        else if (a == "--iterations") { need(1); iterations = atoi(argv[++i]); }
        else if (a == "--out") { need(1); out_prefix = argv[++i]; }
        else if (a == "--device") { need(1); opt.device = atoi(argv[++i]); }
        else if (a == "--arith") { need(1); opt.arith = atoi(argv[++i]); }
        else if (a == "--pfm") pfm = true;
        else if (a == "--hdr") hdr = true;
        else if (a == "--checkpoint") { need(1); ckpt_path = argv[++i]; }
        else if (a == "--checkpoint-every") { need(1); ckpt_every = atoi(argv[++i]); }
        else if (a == "--resume") { need(1); resume_path = argv[++i]; }
        else if (a == "--orbit") { need(1); orbit_script = argv[++i]; }
        else if (a == "--no-aa") opt.antialiasing = 0;
        else if (a == "--dof") opt.depth_of_field = 1;
        else if (a == "--no-sort") opt.sort_by_material = 0;
        else if (a == "--no-cache") opt.cache_first_bounce = 0;
        else if (a == "--per-call") per_call = true;
        else if (a == "--no-render-ahead") pathtraceRenderAhead() = false;
        else if (a == "--denoise") denoise = true;
        else if (a == "--nn") { need(1); nn_path = argv[++i]; }
        else if (a == "--nn-hdr") nnParams().hdr = 1;
        else if (a == "--nn-albedo") { need(1); nn_albedo_path = argv[++i]; }      // the guides prefiltered (ptx_denoise_nn_prefiltered): rt_alb / rt_nrm
        else if (a == "--nn-normal") { need(1); nn_normal_path = argv[++i]; }
        else if (a == "--nn-max-memory") { need(1); nn_max_memory = atoi(argv[++i]); nn_max_memory_set = true; }
        else if (a == "--denoise-passes") { need(1); dparams.passes = atoi(argv[++i]); }
        else if (a == "--frames") { need(1); frames = atoi(argv[++i]); }
        else if (a == "--frame-step") { need(1); frame_step = argv[++i]; }
        else if (a == "--temporal") temporal = true;
        else if (a == "--variance") variance = true;
        else if (a == "--phi-luminance") { need(1); varianceParams().phi_luminance = (float)atof(argv[++i]); }
        else if (a == "--until-error") { need(1); until_error = atof(argv[++i]); }
        else if (a == "--error-floor") { need(1); mparams.floor = (float)atof(argv[++i]); }
        else if (a == "--adaptive") { need(1); adaptive = atof(argv[++i]); }
        else if (a == "--adaptive-denoise") adaptive_denoise = true;
        else if (a == "--measured") measured = true;
        else if (a == "--guide-bounces") { need(1); guide_bounces = atoi(argv[++i]); if (guide_bounces < 1 || guide_bounces > 64) { fprintf(stderr, "--guide-bounces needs 1 <= B <= 64\n"); return 1; } }
        else if (a == "--guide-samples") { need(1); guide_samples = atoi(argv[++i]); if (guide_samples < 1) { fprintf(stderr, "--guide-samples needs K >= 1\n"); return 1; } }
        else if (a == "--tonemap") {
            need(1);
            const std::string v = argv[++i];
            if (v == "clamp") disp.tone = PTX_TONE_CLAMP;
            else if (v == "reinhard") disp.tone = PTX_TONE_REINHARD;
            else if (v == "aces") disp.tone = PTX_TONE_ACES;
            else { fprintf(stderr, "--tonemap needs clamp, reinhard or aces\n"); return 1; }
            g_display.on = true;
        }
        else if (a == "--exposure") {
            need(1);
            const std::string v = argv[++i];
            if (v == "auto") disp.meter = PTX_METER_BLOCKS;
            else {
                disp.meter = PTX_METER_MANUAL;
                disp.exposure = (float)atof(v.c_str());
                if (!(disp.exposure > 0.f)) { fprintf(stderr, "--exposure needs auto or a scale > 0\n"); return 1; }
            }
            g_display.on = true;
        }
        else if (a == "--srgb") { disp.transfer = PTX_TRANSFER_SRGB; g_display.on = true; }
        else if (a == "--dither") { disp.dither = 1; g_display.on = true; }
        else if (a == "--adapt") {
            need(1);
            disp.adapt = (float)atof(argv[++i]);
            if (!(disp.adapt > 0.f) || disp.adapt > 1.f) { fprintf(stderr, "--adapt needs A in (0, 1]\n"); return 1; }
            g_display.on = true;
        }
        else if (a == "--measure-every") { need(1); measure_every = atoi(argv[++i]); }
        else if (compare_flag(cmp, a, argc, argv, i)) {}
        else { fprintf(stderr, "unknown option %s\n", a.c_str()); return 1; }
    }
    g_display.device = opt.device < 0 ? 0 : opt.device;
    if (cmp.denoised && (cmp.ref.empty() || !denoise)) { fprintf(stderr, "--compare-denoised needs --compare REF.pfm and --denoise\n"); return 1; }
    if (!cmp.ref.empty() && (frames > 0 || adaptive >= 0.0)) { fprintf(stderr, "--compare does not combine with --frames or --adaptive\n"); return 1; }
    const bool batches = until_error >= 0.0 || measured;      // the render goes in batches of measure_every iterations, a ptx_moments_add after each
    if (!nn_path.empty() && !denoise) { fprintf(stderr, "--nn needs --denoise\n"); return 1; }
    if (nnParams().hdr && nn_path.empty()) { fprintf(stderr, "--nn-hdr needs --nn FILE\n"); return 1; }
    if (!nn_albedo_path.empty() && nn_path.empty()) { fprintf(stderr, "--nn-albedo needs --nn FILE\n"); return 1; }
    if (!nn_normal_path.empty() && nn_path.empty()) { fprintf(stderr, "--nn-normal needs --nn FILE\n"); return 1; }
    if (nn_max_memory_set && nn_path.empty()) { fprintf(stderr, "--nn-max-memory needs --nn FILE\n"); return 1; }
    if (nn_max_memory_set && nn_max_memory < 0) { fprintf(stderr, "--nn-max-memory needs MB >= 0 (0: no memory limit)\n"); return 1; }
    if (!nn_path.empty() && (temporal || variance || measured || frames > 0)) { fprintf(stderr, "--nn does not combine with --temporal, --variance, --measured or --frames\n"); return 1; }
    if (measured && !denoise) { fprintf(stderr, "--measured needs --denoise\n"); return 1; }
    if (measure_every < 1) { fprintf(stderr, "--measure-every needs K >= 1\n"); return 1; }
    if (until_error >= 0.0 && frames > 0) { fprintf(stderr, "--until-error does not combine with --frames\n"); return 1; }
    if (batches && (per_call || !ckpt_path.empty())) {
        fprintf(stderr, "--until-error and --measured do not combine with --per-call or --checkpoint\n");
        return 1;
    }
    if (adaptive_denoise && adaptive < 0.0) { fprintf(stderr, "--adaptive-denoise needs --adaptive E\n"); return 1; }
    if (adaptive >= 0.0) {
        if (!(adaptive > 0.0)) { fprintf(stderr, "--adaptive needs E > 0\n"); return 1; }
        if (frames > 0 || per_call || !ckpt_path.empty() || until_error >= 0.0 || denoise) {
            fprintf(stderr, "--adaptive does not combine with --frames, --per-call, --checkpoint, --until-error or --denoise\n");
            return 1;
        }
        adaptiveTarget() = (float)adaptive;
        adaptiveParams().floor = mparams.floor;
        adaptiveDenoise() = adaptive_denoise;
    }
    if (guide_samples > 0 && !denoise && !adaptive_denoise) { fprintf(stderr, "--guide-samples needs --denoise or --adaptive-denoise\n"); return 1; }
    if (guide_samples > 0 && temporal) {
        fprintf(stderr, "--guide-samples does not combine with --temporal: reprojection and history matching need one surface per pixel\n");
        return 1;
    }
    if (guide_bounces > 0 && !denoise && !adaptive_denoise) { fprintf(stderr, "--guide-bounces needs --denoise or --adaptive-denoise\n"); return 1; }
    if (guide_bounces > 0 && temporal) {
        fprintf(stderr, "--guide-bounces does not combine with --temporal: reprojection and history matching need the first surface\n");
        return 1;
    }
    guideBounces() = guide_bounces;
    guideSamples() = guide_samples;              // (GPUdenoise with --frames, adaptiveDenoisedFrame; the single frame below sets it itself)
    if (temporal && !denoise) { fprintf(stderr, "--temporal needs --denoise\n"); return 1; }
    if (variance && !denoise) { fprintf(stderr, "--variance needs --denoise\n"); return 1; }
    if (frames < 0 || (frames == 0 && !frame_step.empty())) { fprintf(stderr, "--frame-step needs --frames K, K >= 1\n"); return 1; }
    if (frames > 0 && (per_call || hdr || !ckpt_path.empty() || !resume_path.empty())) {
        fprintf(stderr, "--frames does not combine with --per-call, --hdr, --checkpoint or --resume\n");
        return 1;
    }
    Scene *scene = nullptr;
    try {
        scene = new Scene(argv[1]);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    if (resw > 0 && resh > 0) scene->setResolution(resw, resh);
    if (depth > 0) scene->state.traceDepth = depth;
    if (iterations > 0) scene->state.iterations = (unsigned)iterations;
    if (frames > 0) return run_frames(scene, frames, orbit_script, frame_step, out_prefix, denoise, temporal, variance, measured, measure_every, pfm);
    if (orbit_script.empty()) scene->applyRunCudaCamera();
    else if (!scene->runOrbitScript(orbit_script)) { fprintf(stderr, "bad --orbit script: %s\n", orbit_script.c_str()); return 1; }
    const int width = scene->state.camera.resolution[0], height = scene->state.camera.resolution[1];

    pathtraceFree();
    pathtraceInit(scene);
    ptx_tracer *t = pathtraceHandle();
    int n = (int)scene->state.iterations;
    int done = 0;
    if (!resume_path.empty()) {                 // continue a render: the buffer and the iteration count are all the state
        long long it = 0;
        std::string why;
        if (!ptimg::read_checkpoint(resume_path, width, height, it, &scene->state.image[0].x, why)) { fprintf(stderr, "%s\n", why.c_str()); return 1; }
        if (ptx_write_image(t, &scene->state.image[0].x) != PTX_OK) { fprintf(stderr, "resume failed: %s\n", ptx_last_error()); return 1; }
        done = (int)std::min<long long>(it, n);
        printf("Resumed %s at %d of %d samples.\n", resume_path.c_str(), done, n);
    }
    const int rendered = std::max(n - done, 0);
    const int chunk = (batches || adaptive > 0.0) ? measure_every : (!ckpt_path.empty() && ckpt_every > 0) ? ckpt_every : n;
    double per_call_ms = 0.0;
    if (per_call) {
        // the reference's own loop (runCuda, src/main.cpp:128-148): one pathtrace(pbo, frame, iteration) per frame, the fp32 frame
        // in state.image after each, the timer summed per call.  No window, so no PBO.
        for (int it = done + 1; it <= n; it++) {
            pathtrace(nullptr, 0, it);
            per_call_ms += timer().getGpuElapsedTimeForPreviousOperation();
        }
        done = n;
    }
    while (done < n) {
        const int count = std::min(chunk, n - done);
        if (ptx_render(t, done + 1, count) != PTX_OK || ptx_read_image(t, &scene->state.image[0].x) != PTX_OK) {
            fprintf(stderr, "render failed: %s\n", ptx_last_error());
            return 1;
        }
        done += count;
        if (!ckpt_path.empty()) {
            if (!ptimg::write_checkpoint(ckpt_path, width, height, done, &scene->state.image[0].x)) { fprintf(stderr, "cannot write %s\n", ckpt_path.c_str()); return 1; }
        }
        if (batches) pathtraceMomentsAdd(done);
        if (adaptive > 0.0) {
            pathtraceAdaptiveStep(count);
            const ptx_adaptive_status &as = adaptiveStatus();
            printf("round %d: %d iterations, %d of %d tiles active, %lld pixel-samples so far, worst tile error %.6g\n", (int)as.rounds, done,
                   (int)as.tiles_active, (int)as.tiles, (long long)as.samples_total, (double)as.worst_error);
            if (as.tiles_active == 0 || done >= n) {
                const long long uniform = (long long)as.samples_max * width * height;
                printf("adaptive: %s after %d iterations: %lld pixel-samples, %.1f %% of the %lld of a uniform render at the worst tile's %d\n",
                       as.tiles_active == 0 ? "every tile at its target" : "stopped by --iterations", done, (long long)as.samples_total,
                       100.0 * (double)as.samples_total / (double)uniform, uniform, (int)as.samples_max);
                n = done;
            }
        }
        if (until_error >= 0.0) {
            ptx_moments_summary sum;
            if (ptx_moments_summarize(pathtraceMoments(), &mparams, &sum) != PTX_OK) { fprintf(stderr, "summary failed: %s\n", ptx_last_error()); return 1; }
            const bool stop = sum.pixels > 0 && sum.mean_rel_se <= until_error;
            printf("check: %d iterations, %d batches, mean rel se %.6g, rms %.6g, max %.6g, %lld of %lld pixels over %g\n", done, (int)sum.batches,
                   sum.mean_rel_se, sum.rms_rel_se, sum.max_rel_se, (long long)sum.pixels_over, (long long)sum.pixels, (double)mparams.threshold);
            if (stop || done >= n) {
                printf("until-error: %d iterations, mean rel se %.6g %s %g\n", done, sum.mean_rel_se, stop ? "<=" : ">", until_error);
                n = done;
            }
        }
    }
    ptx_stats st;
    ptx_get_stats(t, &st);
    printf("time: %g\n", per_call ? per_call_ms : st.loop_ms_total);                    // main.cpp:146
    if (rendered > 0)
        printf("%d x %d, depth %d, %d samples (%d traced now): %.3f ms/iteration, %.1f Mrays/s\n", width, height, scene->state.traceDepth, n,
               rendered, st.loop_ms_total / rendered, st.rays_total / (st.loop_ms_total * 1e-3) / 1e6);

    std::ostringstream ss;                                                              // saveImage, main.cpp:94-97
    ss << (out_prefix.empty() ? scene->state.imageName : out_prefix) << "." << startTimeString << "." << n << "samp";
    std::vector<uint8_t> rgb8;
    float divisor = (float)n;
    if (adaptive > 0.0) {                       // the frame normalised tile by tile: mean radiance already, so divided by 1
        const float *frame = adaptiveFrame();
        if (!frame) { fprintf(stderr, "--adaptive: no round was rendered\n"); return 1; }
        memcpy(&scene->state.image[0].x, frame, sizeof(float) * 3 * (size_t)width * height);
        divisor = 1.0f;
    }
    if (!frame_rgb8(0, width, height, &scene->state.image[0].x, divisor, ss.str() + ".png", rgb8)) return 1;
    if (!ptimg::write_png_rgb8(ss.str() + ".png", width, height, rgb8.data())) { fprintf(stderr, "cannot write %s.png\n", ss.str().c_str()); return 1; }
    printf("Saved %s.png.\n", ss.str().c_str());
    if (pfm) { ptimg::write_pfm(ss.str() + ".pfm", width, height, &scene->state.image[0].x, divisor); printf("Saved %s.pfm.\n", ss.str().c_str()); }
    if (denoise && n > 0) {                     // the denoised frame next to it: mean radiance already, so divided by 1
        std::vector<float> den((size_t)width * height * 3);
        if (guide_bounces > 0 && ptx_set_guide_bounces(t, guide_bounces) != PTX_OK) { fprintf(stderr, "denoise failed: %s\n", ptx_last_error()); return 1; }
        if (guide_samples > 0 && ptx_set_guide_samples(t, 1, std::min(guide_samples, n)) != PTX_OK) { fprintf(stderr, "denoise failed: %s\n", ptx_last_error()); return 1; }
        ptx_nn *nn = nullptr;
        const int nn_device = opt.device < 0 ? 0 : opt.device;
        if (!nn_path.empty() && (nn_max_memory_set ? ptx_nn_create_from_file_tiled(nn_device, width, height, nn_path.c_str(), nn_max_memory, &nn)
                                                   : ptx_nn_create_from_file(nn_device, width, height, nn_path.c_str(), &nn)) != PTX_OK) { fprintf(stderr, "denoise failed: %s\n", ptx_last_error()); return 1; }
        ptx_nn_prefilter *pf = nullptr;
        if (nn && (!nn_albedo_path.empty() || !nn_normal_path.empty()) &&
            ptx_nn_prefilter_create_from_files(nn_device, width, height, nn_albedo_path.empty() ? nullptr : nn_albedo_path.c_str(),
                                               nn_normal_path.empty() ? nullptr : nn_normal_path.c_str(), nn_max_memory_set ? nn_max_memory : -1, &pf) != PTX_OK) {
            fprintf(stderr, "denoise failed: %s\n", ptx_last_error()); return 1;
        }
        const int rc = pf ? ptx_denoise_nn_prefiltered(t, nn, pf, &nnParams(), nullptr, n)
                     : nn ? ptx_denoise_nn(t, nn, &nnParams(), n)
                     : measured ? ptx_denoise_measured(t, pathtraceMoments(), &dparams, &varianceParams(), 0, n)
                     : variance ? ptx_denoise_variance(t, nullptr, &dparams, nullptr, &varianceParams(), n) : ptx_denoise(t, &dparams, n);
        if (rc != PTX_OK || ptx_read_denoised(t, den.data()) != PTX_OK) { fprintf(stderr, "denoise failed: %s\n", ptx_last_error()); return 1; }
        ptx_nn_destroy(nn);
        ptx_nn_prefilter_destroy(pf);
        if (!frame_rgb8(1, width, height, den.data(), 1.0f, ss.str() + ".denoised.png", rgb8)) return 1;
        if (!ptimg::write_png_rgb8(ss.str() + ".denoised.png", width, height, rgb8.data())) { fprintf(stderr, "cannot write %s.denoised.png\n", ss.str().c_str()); return 1; }
        printf("Saved %s.denoised.png.\n", ss.str().c_str());
        if (pfm) { ptimg::write_pfm(ss.str() + ".denoised.pfm", width, height, den.data(), 1.0f); printf("Saved %s.denoised.pfm.\n", ss.str().c_str()); }
    }
    if (adaptive_denoise) {                     // ptx_denoise_adaptive on the frame just saved: mean radiance, so divided by 1
        const float *den = adaptiveDenoisedFrame();
        if (!den) { fprintf(stderr, "--adaptive-denoise: no round was rendered\n"); return 1; }
        if (!frame_rgb8(1, width, height, den, 1.0f, ss.str() + ".denoised.png", rgb8)) return 1;
        if (!ptimg::write_png_rgb8(ss.str() + ".denoised.png", width, height, rgb8.data())) { fprintf(stderr, "cannot write %s.denoised.png\n", ss.str().c_str()); return 1; }
        printf("Saved %s.denoised.png.\n", ss.str().c_str());
        if (pfm) { ptimg::write_pfm(ss.str() + ".denoised.pfm", width, height, den, 1.0f); printf("Saved %s.denoised.pfm.\n", ss.str().c_str()); }
    }
    if (!cmp.ref.empty() && n > 0) {            // the frame (or the denoised one) on the device against REF.pfm, a file as --pfm writes them
        std::vector<float> ref;
        int wr, hr;
        std::string why;
        if (!ptimg::read_pfm(cmp.ref, wr, hr, ref, why)) { fprintf(stderr, "%s\n", why.c_str()); return 1; }
        if (wr != width || hr != height) { fprintf(stderr, "--compare: %s is %d x %d, the frame is %d x %d\n", cmp.ref.c_str(), wr, hr, width, height); return 1; }
        ptx_metrics *m = nullptr;
        ptx_metrics_result r = ptx_metrics_result();
        r.struct_size = sizeof r;
        const ptx_nn_image ib = packed_image(ref);
        const bool ok = ptx_metrics_create(opt.device < 0 ? 0 : opt.device, width, height, &m) == PTX_OK &&
                        ptx_metrics_tracer(m, t, cmp.denoised ? PTX_DISPLAY_DENOISED : PTX_DISPLAY_IMAGE, n, &ib, &cmp.params, &r) == PTX_OK;
        ptx_metrics_destroy(m);
        if (!ok) { fprintf(stderr, "compare failed: %s\n", ptx_last_error()); return 1; }
        print_metrics(r);
    }
    if (hdr) {                                                                          // img.saveHDR, main.cpp:101
        std::vector<float> mean;
        ptimg::to_mean_mirrored(width, height, &scene->state.image[0].x, divisor, mean);
        if (!ptimg::write_hdr(ss.str() + ".hdr", width, height, mean.data())) { fprintf(stderr, "cannot write %s.hdr\n", ss.str().c_str()); return 1; }
        printf("Saved %s.hdr.\n", ss.str().c_str());
    }
    g_display.release();
    GPUdenoiseRelease();
    pathtraceFree();
    delete scene;
    return 0;
}
