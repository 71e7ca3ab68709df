// pathtrace_api.cpp -- the reference's four free functions (src/pathtrace.h:6-9) over the C ABI.
// Keeps the reference's module-static, one-scene-per-process contract (src/pathtrace.cu:91-98) and its
// print-and-exit error policy (checkCUDAError, src/pathtrace.cu:42-60); the C ABI underneath returns codes.
#include "pathtrace_api.h"

#include "pt_handle.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace {
Scene *hst_scene = nullptr;          // borrowed, must outlive pathtraceFree (src/pathtrace.cu:91,102)
ptx_tracer *g_tracer = nullptr;
ptx_multi *g_multi = nullptr;        // != NULL: several devices (pathtraceDevices()); g_tracer is then device 0's tracer
bool g_albedo_read = false;          // several devices, apps variant: state.albedo holds the merged AOV of iteration 1
void *g_pinned[3] = {nullptr, nullptr, nullptr};      // state.image / state.albedo page-locked for the per-iteration read-back
ptx_options g_options;
bool g_options_init = false;
int g_last_iter = 0;                 // iteration of the last pathtrace() call: the spp GPUdenoise divides by
bool g_output_on_device = false;     // GPUdenoise(true) ran since the last pathtrace(): sendToGPU shows the device frame
ptx_denoise_params g_denoise;
bool g_denoise_init = false;
ptx_temporal_params g_temporal_params;
bool g_temporal_params_init = false;
ptx_variance_params g_variance_params;
bool g_variance_params_init = false;
ptx_temporal *g_temporal = nullptr;  // GPUdenoise's history with denoiseTemporal() on: kept across pathtraceFree / pathtraceInit
int g_temporal_key[3] = {0, 0, 0};   // its device, width, height
ptx_nn *g_nn = nullptr;              // GPUdenoise's network with nnWeights() set: kept like g_temporal
int g_nn_key[4] = {0, 0, 0, 0};      // its device, width, height, nnMaxMemoryMB()
std::string g_nn_path;               // ... and the weight file it was made from
ptx_nn_prefilter *g_nn_pf = nullptr; // ... and the prefilter of its guides with nnAlbedoWeights() / nnNormalWeights() set, under the same key
int g_nn_pf_key[4] = {0, 0, 0, 0};
std::string g_nn_pf_path[2];         // ... and the weight files it was made from
int g_device = 0;                    // the device of g_tracer
ptx_moments *g_moments = nullptr;    // pathtrace()'s batch means with momentsBatch() > 0: created on first use
int g_moments_key[3] = {0, 0, 0};    // its device, width, height
ptx_adaptive *g_adaptive = nullptr;  // pathtrace()'s adaptive sampling with adaptiveTarget() > 0: created on first use, with g_moments' key
ptx_adaptive_status g_adaptive_status = {};
std::vector<float> g_adaptive_frame; // adaptiveFrame()'s host copy
std::vector<float> g_adaptive_denoised;      // adaptiveDenoisedFrame()'s
ptx_display *g_display = nullptr;    // the preview's display transform with displayTransform() on: created on first use
int g_display_key[3] = {0, 0, 0};    // its device, width, height
ptx_display_status g_display_status = {};
ptx_metrics *g_metrics = nullptr;    // compareToReference's handle: created on first use
int g_metrics_key[3] = {0, 0, 0};    // its device, width, height
std::vector<uint8_t> g_display_codes;        // sendToGPU's codes of a host frame on their way to the pbo
int g_calls = 0;                     // pathtrace() calls since pathtraceInit

void check(int rc, const char *what) {
    if (rc == PTX_OK) return;
    fprintf(stderr, "mi355x pathtracer error (%s): %s\n", what, ptx_last_error());
    exit(EXIT_FAILURE);
}
}  // namespace

Scene::Scene(const std::string &filename, const std::string &base_dir) : impl_(nullptr) {
    int rc = ptx_scene_load(filename.c_str(), base_dir.empty() ? nullptr : base_dir.c_str(), &impl_);
    if (rc != PTX_OK) throw std::runtime_error(std::string("Scene: ") + ptx_last_error());
    int ng = ptx_scene_num_geoms(impl_), nm = ptx_scene_num_materials(impl_);
    if (ng) geoms.assign(ptx_scene_geoms(impl_), ptx_scene_geoms(impl_) + ng);
    if (nm) materials.assign(ptx_scene_materials(impl_), ptx_scene_materials(impl_) + nm);
    state.camera = *ptx_scene_camera(impl_);
    state.iterations = (unsigned)ptx_scene_iterations(impl_);
    state.traceDepth = ptx_scene_trace_depth(impl_);
    state.imageName = ptx_scene_image_name(impl_);
    state.image.assign((size_t)state.camera.resolution[0] * state.camera.resolution[1], mi355x::vec3{0.f, 0.f, 0.f});
    state.albedo = state.image;            // apps/src/scene.cpp:380-383
    state.output = state.image;
}

Scene::~Scene() { ptx_scene_free(impl_); }

void Scene::applyRunCudaCamera() {
    *ptx_scene_camera(impl_) = ptx_camera(state.camera);
    ptx_scene_apply_runcuda_camera(impl_);
    state.camera = *ptx_scene_camera(impl_);
}

bool Scene::runOrbitScript(const std::string &script) {
    *ptx_scene_camera(impl_) = ptx_camera(state.camera);
    ptx_orbit o;
    ptx_orbit_init(impl_, &o);
    ptx_orbit_apply(impl_, &o);
    const int w = state.camera.resolution[0], h = state.camera.resolution[1];
    size_t pos = 0;
    bool ok = true;
    while (pos <= script.size() && ok) {
        size_t end = script.find(';', pos);
        if (end == std::string::npos) end = script.size();
        std::string ev = script.substr(pos, end - pos);
        pos = end + 1;
        while (!ev.empty() && ev.front() == ' ') ev.erase(ev.begin());
        while (!ev.empty() && ev.back() == ' ') ev.pop_back();
        if (ev.empty()) continue;
        double a = 0.0, b = 0.0;
        if (ev == "space") ptx_orbit_recenter(impl_, &o);
        else if (sscanf(ev.c_str(), "left:%lf,%lf", &a, &b) == 2) ptx_orbit_left_drag(&o, a, b, w, h);
        else if (sscanf(ev.c_str(), "middle:%lf,%lf", &a, &b) == 2) ptx_orbit_middle_drag(impl_, a, b);
        else if (sscanf(ev.c_str(), "right:%lf", &a) == 1) ptx_orbit_right_drag(&o, a, h);
        else ok = false;
        if (ok) ptx_orbit_apply(impl_, &o);
    }
    state.camera = *ptx_scene_camera(impl_);
    return ok;
}

void Scene::setResolution(int w, int h) {
    ptx_scene_set_resolution(impl_, w, h);
    state.camera = *ptx_scene_camera(impl_);
    state.image.assign((size_t)w * h, mi355x::vec3{0.f, 0.f, 0.f});
    state.albedo = state.image;
    state.output = state.image;
}

ptx_options &pathtraceOptions() {
    if (!g_options_init) { ptx_default_options(&g_options); g_options_init = true; }
    return g_options;
}

bool &pathtraceRenderAhead() {
    static bool on = true;
    return on;
}

PerformanceTimer &timer() {
    static PerformanceTimer *t = new PerformanceTimer;      // (never destroyed: no HIP call from a static destructor, after the runtime may have gone)
    return *t;
}

std::vector<int> &pathtraceDevices() {
    static std::vector<int> devices;
    return devices;
}

// ---- PerformanceTimer, src/timer.h:17-100 ---------------------------------------------------------------------------------
// (the two events of a GPU interval live from startGpuTimer to endGpuTimer; pathtraceFree() releases what the module's timer still
// holds, the destructor what any other does)
PerformanceTimer::PerformanceTimer() {}
PerformanceTimer::~PerformanceTimer() { mi355x_timer_release(*this); }
void mi355x_timer_release(PerformanceTimer &t) { delete t.gpu_region; t.gpu_region = nullptr; }

void PerformanceTimer::startCpuTimer() {
    if (cpu_timer_started) throw std::runtime_error("CPU timer already started");
    cpu_timer_started = true;
    time_start_cpu_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::high_resolution_clock::now().time_since_epoch()).count();
}

void PerformanceTimer::endCpuTimer() {
    const long long now = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::high_resolution_clock::now().time_since_epoch()).count();
    if (!cpu_timer_started) throw std::runtime_error("CPU timer not started");
    prev_elapsed_time_cpu_milliseconds = (float)((double)(now - time_start_cpu_ns) * 1e-6);
    cpu_timer_started = false;
}

// The reference records on the null stream, which every one of ITS launches runs on.  Here the work runs on the tracer's own
// (non-blocking) stream, so that is where the events go while a tracer exists: the interval then covers the pathtrace() calls
// between start and end, as it does in the reference.
static hipStream_t timer_stream() { return g_tracer ? (hipStream_t)ptx_stream(g_tracer) : (hipStream_t) nullptr; }

// The events are made where they are recorded: with the tracer's device current, or on the current device while there is no tracer.
// A create or record that fails leaves no region, and the interval at 0.
void PerformanceTimer::startGpuTimer() {
    if (gpu_timer_started) throw std::runtime_error("GPU timer already started");
    gpu_timer_started = true;
    mi355x_timer_release(*this);
    gpu_region = new TimedRegion;
    if ((g_tracer && hipSetDevice(g_device) != hipSuccess) || gpu_region->begin(timer_stream()) != hipSuccess) {
        (void)hipGetLastError();
        mi355x_timer_release(*this);
    }
}

void PerformanceTimer::endGpuTimer() {
    float ms = 0.f;
    if (gpu_region && gpu_region->end(&ms) != hipSuccess) { ms = 0.f; (void)hipGetLastError(); }
    mi355x_timer_release(*this);
    if (!gpu_timer_started) throw std::runtime_error("GPU timer not started");
    prev_elapsed_time_gpu_milliseconds = ms;
    gpu_timer_started = false;
    gpu_interval_is_callers = true;
}

// pathtrace() ran: the module's timer answers with ITS bounce loop again, as after the reference's own start/endGpuTimer pair
// inside pathtrace (src/pathtrace.cu:489, 545)
void mi355x_timer_note_pathtrace(PerformanceTimer &t) { t.gpu_interval_is_callers = false; }

float PerformanceTimer::getGpuElapsedTimeForPreviousOperation() {
    if (gpu_interval_is_callers || this != &timer()) return prev_elapsed_time_gpu_milliseconds;
    if (!g_tracer) return 0.f;
    if (!g_multi) return (float)ptx_last_loop_ms(g_tracer);
    double ms = 0.0;                 // several devices work side by side: the slowest one's bounce loop
    for (int i = 0; i < ptx_multi_device_count(g_multi); i++) ms = std::max(ms, ptx_last_loop_ms(ptx_multi_tracer(g_multi, i)));
    return (float)ms;
}

ptx_denoise_params &denoiseParams() {
    if (!g_denoise_init) { ptx_default_denoise_params(&g_denoise); g_denoise_init = true; }
    return g_denoise;
}

bool &denoiseTemporal() {
    static bool on = false;
    return on;
}

ptx_temporal_params &temporalParams() {
    if (!g_temporal_params_init) { ptx_default_temporal_params(&g_temporal_params); g_temporal_params_init = true; }
    return g_temporal_params;
}

bool &denoiseVariance() {
    static bool on = false;
    return on;
}

int &guideSamples() {
    static int k = 0;
    return k;
}

// guideSamples() onto the tracer before a filter call: the camera rays of iterations 1 .. min(K, the iterations rendered)
static void apply_guide_samples(const char *what, int rendered) {
    static bool applied = false;      // (while the switch has never been on, the tracer's own setting is left alone)
    const int k = guideSamples() > 0 ? std::min(guideSamples(), std::max(rendered, 1)) : 0;
    if (k == 0 && !applied) return;
    check(ptx_set_guide_samples(g_tracer, 1, k), what);
    applied = k > 0;
}

int &guideBounces() {
    static int b = 0;
    return b;
}

// guideBounces() onto the tracer before a filter call, next to guideSamples()
static void apply_guide_bounces(const char *what) {
    static bool applied = false;      // (while the switch has never been on, the tracer's own setting is left alone)
    const int b = guideBounces();
    if (b == 0 && !applied) return;
    check(ptx_set_guide_bounces(g_tracer, b), what);
    applied = b != 0;
}

ptx_variance_params &varianceParams() {
    if (!g_variance_params_init) { ptx_default_variance_params(&g_variance_params); g_variance_params_init = true; }
    return g_variance_params;
}

int &momentsBatch() {
    static int k = 0;
    return k;
}

ptx_moments *pathtraceMoments() { return g_moments; }

bool &denoiseMeasured() {
    static bool on = false;
    return on;
}

std::string &nnWeights() {
    static std::string path;
    return path;
}

int &nnMaxMemoryMB() {
    static int mb = -1;
    return mb;
}

std::string &nnAlbedoWeights() {
    static std::string path;
    return path;
}

std::string &nnNormalWeights() {
    static std::string path;
    return path;
}

ptx_nn_prefilter_params &nnPrefilterParams() {
    static ptx_nn_prefilter_params p;
    static bool init = false;
    if (!init) { ptx_default_nn_prefilter_params(&p); init = true; }
    return p;
}

ptx_nn_params &nnParams() {
    static ptx_nn_params p;
    static bool init = false;
    if (!init) { ptx_default_nn_params(&p); init = true; }
    return p;
}

float &adaptiveTarget() {
    static float e = 0.f;
    return e;
}

ptx_adaptive_params &adaptiveParams() {
    static ptx_adaptive_params p;
    static bool init = false;
    if (!init) { ptx_default_adaptive_params(&p); init = true; }
    return p;
}

ptx_adaptive *pathtraceAdaptive() { return g_adaptive; }
const ptx_adaptive_status &adaptiveStatus() { return g_adaptive_status; }

bool &displayTransform() {
    static bool on = false;
    return on;
}

ptx_display_params &displayParams() {
    static ptx_display_params p;
    static bool init = false;
    if (!init) { ptx_default_display_params(&p); init = true; }
    return p;
}

const ptx_display_status &displayStatus() {
    g_display_status = ptx_display_status();
    g_display_status.metered = g_display_status.applied = 1.f;
    if (g_display) check(ptx_display_get_status(g_display, &g_display_status), "displayStatus");
    return g_display_status;
}

// the module-level display handle for the current device and resolution
static void display_handle(const char *what) {
    if (g_multi) { fprintf(stderr, "%s: the display transform runs on one device; pathtraceDevices() names several\n", what); exit(EXIT_FAILURE); }
    const int w = hst_scene->state.camera.resolution[0], h = hst_scene->state.camera.resolution[1];
    const int key[3] = {g_device, w, h};
    if (g_display && memcmp(key, g_display_key, sizeof key) != 0) { ptx_display_destroy(g_display); g_display = nullptr; }
    if (!g_display) {
        check(ptx_display_create(g_device, w, h, &g_display), what);
        memcpy(g_display_key, key, sizeof key);
    }
}

// pathtrace()'s preview: the reference's rule, or the display stage on the same buffer
static void write_preview(int iter, void *pbo) {
    if (!displayTransform() || !pbo) { check(ptx_write_pbo_device(g_tracer, iter, pbo), "sendImageToPBO"); return; }
    display_handle("pathtrace");
    check(ptx_display_tracer(g_display, g_tracer, PTX_DISPLAY_IMAGE, iter, &displayParams(), pbo), "pathtrace display");
}

ptx_metrics_params &metricsParams() {
    static ptx_metrics_params p;
    static bool init = false;
    if (!init) { ptx_default_metrics_params(&p); init = true; }
    return p;
}

ptx_metrics_result compareToReference(const float *rgb, int iter, bool denoised) {
    if (g_multi) { fprintf(stderr, "compareToReference: the metrics run on one device; pathtraceDevices() names several\n"); exit(EXIT_FAILURE); }
    const int w = hst_scene->state.camera.resolution[0], h = hst_scene->state.camera.resolution[1];
    const int key[3] = {g_device, w, h};
    if (g_metrics && memcmp(key, g_metrics_key, sizeof key) != 0) { ptx_metrics_destroy(g_metrics); g_metrics = nullptr; }
    if (!g_metrics) {
        check(ptx_metrics_create(g_device, w, h, &g_metrics), "compareToReference");
        memcpy(g_metrics_key, key, sizeof key);
    }
    ptx_nn_image ref = ptx_nn_image();
    ref.ptr = rgb;
    ref.format = PTX_NN_FORMAT_FLOAT3;
    ptx_metrics_result r = ptx_metrics_result();
    r.struct_size = sizeof r;
    check(ptx_metrics_tracer(g_metrics, g_tracer, denoised ? PTX_DISPLAY_DENOISED : PTX_DISPLAY_IMAGE, iter, &ref, &metricsParams(), &r), "compareToReference");
    return r;
}

void GPUdenoiseRelease() {
    ptx_metrics_destroy(g_metrics);
    g_metrics = nullptr;
    ptx_display_destroy(g_display);
    g_display = nullptr;
    ptx_temporal_destroy(g_temporal);
    g_temporal = nullptr;
    ptx_nn_destroy(g_nn);
    g_nn = nullptr;
    ptx_nn_prefilter_destroy(g_nn_pf);
    g_nn_pf = nullptr;
    ptx_moments_destroy(g_moments);
    g_moments = nullptr;
    ptx_adaptive_destroy(g_adaptive);
    g_adaptive = nullptr;
}

// the module-level moments handle for the current device and resolution, fresh when it had to be made
static void moments_handle() {
    const int w = hst_scene->state.camera.resolution[0], h = hst_scene->state.camera.resolution[1];
    const int key[3] = {g_device, w, h};
    if (g_moments && memcmp(key, g_moments_key, sizeof key) != 0) {
        ptx_moments_destroy(g_moments); g_moments = nullptr;
        ptx_adaptive_destroy(g_adaptive); g_adaptive = nullptr;      // (the two are used together: one key)
    }
    if (!g_moments) {
        check(ptx_moments_create(g_device, w, h, &g_moments), "pathtrace moments");
        memcpy(g_moments_key, key, sizeof key);
    }
}

// one round: the last k iterations into both handles, then the next mask
void pathtraceAdaptiveStep(int k) {
    if (!g_tracer || !hst_scene) { fprintf(stderr, "pathtraceAdaptiveStep called before pathtraceInit\n"); exit(EXIT_FAILURE); }
    if (g_multi) { fprintf(stderr, "adaptive sampling does not run on several devices\n"); exit(EXIT_FAILURE); }
    moments_handle();
    if (!g_adaptive) check(ptx_adaptive_create(g_device, g_moments_key[1], g_moments_key[2], &g_adaptive), "pathtrace adaptive");
    ptx_adaptive_params p = adaptiveParams();
    p.target = adaptiveTarget();
    check(ptx_adaptive_add(g_adaptive, g_moments, g_tracer, k), "pathtrace adaptive");
    check(ptx_adaptive_select(g_adaptive, g_moments, g_tracer, &p, &g_adaptive_status), "pathtrace adaptive");
}

const float *adaptiveFrame() {
    if (!g_tracer || !g_adaptive) return nullptr;
    check(ptx_adaptive_resolve(g_adaptive, g_tracer), "adaptiveFrame");
    g_adaptive_frame.resize((size_t)g_moments_key[1] * g_moments_key[2] * 3);
    check(ptx_adaptive_read(g_adaptive, g_adaptive_frame.data(), nullptr, nullptr, nullptr), "adaptiveFrame");
    return g_adaptive_frame.data();
}

bool &adaptiveDenoise() {
    static bool on = false;
    return on;
}

const float *adaptiveDenoisedFrame() {
    if (!adaptiveDenoise() || !g_tracer || !g_adaptive || !g_moments || g_adaptive_status.rounds < 1) return nullptr;
    apply_guide_samples("adaptiveDenoisedFrame", (int)g_adaptive_status.samples_max);      // (the worst tile's count: the iterations rendered)
    apply_guide_bounces("adaptiveDenoisedFrame");
    check(ptx_denoise_adaptive(g_tracer, g_adaptive, g_moments, &denoiseParams(), &varianceParams(), 0), "adaptiveDenoisedFrame");
    g_adaptive_denoised.resize((size_t)g_moments_key[1] * g_moments_key[2] * 3);
    check(ptx_read_denoised(g_tracer, g_adaptive_denoised.data()), "adaptiveDenoisedFrame");
    return g_adaptive_denoised.data();
}

// one batch: everything the frame gained since the last one
void pathtraceMomentsAdd(int iter) {
    if (!g_tracer || !hst_scene) { fprintf(stderr, "pathtraceMomentsAdd called before pathtraceInit\n"); exit(EXIT_FAILURE); }
    moments_handle();
    if (g_multi) check(ptx_moments_add_host(g_moments, &hst_scene->state.image[0].x, iter), "pathtrace moments");   // the assembled frame
    else check(ptx_moments_add(g_moments, g_tracer, iter), "pathtrace moments");
}

// after every momentsBatch()-th call
static void moments_step(int iter) {
    const int k = momentsBatch();
    g_calls++;
    if (k > 0 && g_calls % k == 0) {
        if (adaptiveTarget() > 0.f) pathtraceAdaptiveStep(k);       // (the tiled add in place of the plain one, then the next mask)
        else pathtraceMomentsAdd(iter);
    }
}

void pathtraceInit(Scene *scene) {
    hst_scene = scene;
    g_albedo_read = false;
    g_last_iter = 0;
    g_output_on_device = false;
    g_calls = 0;
    if (g_moments) ptx_moments_reset(g_moments);
    if (g_adaptive) ptx_adaptive_reset(g_adaptive);      // (the tracer made below has no mask)
    g_adaptive_status = ptx_adaptive_status();
    const std::vector<int> &devs = pathtraceDevices();
    if (devs.size() > 1) {
        // the C ABI's multi-device layer takes the loaded scene: hand it the caller's camera and depth first
        *ptx_scene_camera(scene->handle()) = ptx_camera(scene->state.camera);
        ptx_scene_set_trace_depth(scene->handle(), scene->state.traceDepth);
        check(ptx_multi_create(scene->handle(), &pathtraceOptions(), devs.data(), (int)devs.size(), 0, &g_multi), "pathtraceInit");
        g_tracer = ptx_multi_tracer(g_multi, 0);
        g_device = devs[0];
        check(ptx_multi_set_render_ahead(g_multi, pathtraceRenderAhead() ? 1 : 0), "pathtraceInit");
    } else {
        ptx_options o = pathtraceOptions();
        if (devs.size() == 1) o.device = devs[0];
        const ptx_camera cam = scene->state.camera;
        check(ptx_create((int)scene->geoms.size(), scene->geoms.data(), (int)scene->materials.size(), scene->materials.data(),
                         &cam, scene->state.traceDepth, &o, nullptr, nullptr, &g_tracer),
              "pathtraceInit");
        check(ptx_set_render_ahead(g_tracer, pathtraceRenderAhead() ? 1 : 0), "pathtraceInit");
        g_device = o.device;
        if (g_device < 0 && hipGetDevice(&g_device) != hipSuccess) g_device = 0;     // -1: the current device, which ptx_create used
    }
    // the reference copies the whole fp32 frame into scene->state.image after every iteration (src/pathtrace.cu:555-556):
    // page-lock the destination once, so that each of those copies is one DMA at PCIe rate (not fatal if it cannot be)
    const size_t bytes = scene->state.image.size() * sizeof(mi355x::vec3);
    if (bytes && ptx_pin_host_buffer(scene->state.image.data(), bytes) == PTX_OK) g_pinned[0] = scene->state.image.data();
    if (pathtraceOptions().apps_variant && bytes && scene->state.albedo.size() == scene->state.image.size() &&
        ptx_pin_host_buffer(scene->state.albedo.data(), bytes) == PTX_OK) g_pinned[1] = scene->state.albedo.data();
}

void pathtraceFree() {          // safe before init and idempotent, as main.cpp:129 relies on
    mi355x_timer_release(timer());      // (an interval begun and not ended: its events go before the stream they were recorded on)
    for (void *&p : g_pinned) { if (p) ptx_unpin_host_buffer(p); p = nullptr; }
    if (g_multi) ptx_multi_destroy(g_multi);
    else ptx_destroy(g_tracer);
    g_multi = nullptr;
    g_tracer = nullptr;
}

void mi355x::pathtrace_raw(void *pbo, int frame, int iter) {
    (void)frame;                 // unused by the reference as well
    if (!g_tracer || !hst_scene) { fprintf(stderr, "pathtrace called before pathtraceInit\n"); exit(EXIT_FAILURE); }
    mi355x_timer_note_pathtrace(timer());
    g_last_iter = iter;
    g_output_on_device = false;
    // the reference re-reads camera and traceDepth on every call (src/pathtrace.cu:434-436)
    const bool apps = pathtraceOptions().apps_variant != 0;
    const ptx_camera cam = hst_scene->state.camera;
    if (g_multi) {               // several devices: every device its tile, then the row blocks into device 0's frame
        check(ptx_multi_set_camera(g_multi, &cam, hst_scene->state.traceDepth), "pathtrace camera");
        check(ptx_multi_iterate(g_multi, iter), "pathtrace");
        check(ptx_multi_read_image(g_multi, &hst_scene->state.image[0].x), "image readback");      // assemble + :555-556
        if (!apps) write_preview(iter, pbo);                                                       // from the assembled frame
        // the AOV is written by iteration 1 alone (apps/src/pathtrace.cu:412-462): merged from the devices once, when it is new,
        // not n full-frame reads and a host merge per call
        if (apps && (iter == 1 || !g_albedo_read)) {
            check(ptx_multi_read_albedo(g_multi, &hst_scene->state.albedo[0].x), "albedo readback");
            g_albedo_read = true;
        }
        check(ptx_synchronize(g_tracer), "pathtrace");
        moments_step(iter);
        return;
    }
    check(ptx_set_camera(g_tracer, &cam, hst_scene->state.traceDepth), "pathtrace camera");
    check(ptx_iterate(g_tracer, iter), "pathtrace");
    // apps/src builds with AI_DENOISE: no preview from here (sendToGPU shows the denoised frame), the albedo AOV comes back
    // with the image (apps/src/pathtrace.cu:658-669)
    if (!apps) write_preview(iter, pbo);
    check(ptx_read_image(g_tracer, &hst_scene->state.image[0].x), "image readback");     // :555-556
    if (apps) check(ptx_read_albedo(g_tracer, &hst_scene->state.albedo[0].x), "albedo readback");
    moments_step(iter);
}

// apps/src/pathtrace.cu:673-685: the denoised frame in state.output -> the pbo, scaled by 255 and clamped, no division by iter
void mi355x::sendToGPU_raw(void *pbo, int iter) {
    (void)iter;                  // passed to the kernel but unused there as well (apps/src/pathtrace.cu:96-116)
    if (!g_tracer || !hst_scene) { fprintf(stderr, "sendToGPU called before pathtraceInit\n"); exit(EXIT_FAILURE); }
    if (displayTransform() && pbo) {
        display_handle("sendToGPU");
        if (g_output_on_device) {
            check(ptx_display_tracer(g_display, g_tracer, PTX_DISPLAY_DENOISED, 1, &displayParams(), pbo), "sendToGPU display");
            check(ptx_synchronize(g_tracer), "sendToGPU");
            return;
        }
        // a host frame: through the handle's staging buffer, then the codes into the pbo
        g_display_codes.resize(hst_scene->state.output.size() * 4);
        check(ptx_display_host(g_display, &hst_scene->state.output[0].x, 1.f, &displayParams(), g_display_codes.data()), "sendToGPU display");
        if (hipMemcpy(pbo, g_display_codes.data(), g_display_codes.size(), hipMemcpyHostToDevice) != hipSuccess) {
            fprintf(stderr, "mi355x pathtracer error (sendToGPU display): the codes could not be copied into the pbo\n");
            exit(EXIT_FAILURE);
        }
        return;
    }
    if (g_output_on_device) {
        check(ptx_write_denoised_pbo_from_device(g_tracer, pbo), "sendToGPU");
        check(ptx_synchronize(g_tracer), "sendToGPU");
        return;
    }
    check(ptx_write_denoised_pbo_device(g_tracer, &hst_scene->state.output[0].x, pbo), "sendToGPU");
}

void GPUdenoise(bool keep_on_device) {
    if (!g_tracer || !hst_scene) { fprintf(stderr, "GPUdenoise called before pathtraceInit\n"); exit(EXIT_FAILURE); }
    if (g_multi) { fprintf(stderr, "GPUdenoise: the denoiser runs on one device; pathtraceDevices() names several\n"); exit(EXIT_FAILURE); }
    if (g_last_iter < 1) { fprintf(stderr, "GPUdenoise called before the first pathtrace\n"); exit(EXIT_FAILURE); }
    if (denoiseMeasured() && !g_moments) {
        fprintf(stderr, "GPUdenoise: denoiseMeasured() needs momentsBatch() > 0 and at least one batch\n");
        exit(EXIT_FAILURE);
    }
    apply_guide_samples("GPUdenoise", g_last_iter);
    apply_guide_bounces("GPUdenoise");
    if (nnWeights().empty() && (!nnAlbedoWeights().empty() || !nnNormalWeights().empty())) {
        fprintf(stderr, "GPUdenoise: nnAlbedoWeights() / nnNormalWeights() prefilter the guides of the network denoiser: they need nnWeights()\n");
        exit(EXIT_FAILURE);
    }
    if (!nnWeights().empty()) {
        if (denoiseTemporal() || denoiseVariance() || denoiseMeasured()) {
            fprintf(stderr, "GPUdenoise: nnWeights() does not combine with denoiseTemporal(), denoiseVariance() or denoiseMeasured()\n");
            exit(EXIT_FAILURE);
        }
        const int w = hst_scene->state.camera.resolution[0], h = hst_scene->state.camera.resolution[1];
        const int key[4] = {g_device, w, h, nnMaxMemoryMB()};
        if (g_nn && (memcmp(key, g_nn_key, sizeof key) != 0 || g_nn_path != nnWeights())) {
            ptx_nn_destroy(g_nn);
            g_nn = nullptr;
        }
        if (!g_nn) {
            check(nnMaxMemoryMB() < 0 ? ptx_nn_create_from_file(g_device, w, h, nnWeights().c_str(), &g_nn)
                                      : ptx_nn_create_from_file_tiled(g_device, w, h, nnWeights().c_str(), nnMaxMemoryMB(), &g_nn), "GPUdenoise");
            memcpy(g_nn_key, key, sizeof key);
            g_nn_path = nnWeights();
        }
        const bool prefilter = !nnAlbedoWeights().empty() || !nnNormalWeights().empty();
        if (g_nn_pf && (!prefilter || memcmp(key, g_nn_pf_key, sizeof key) != 0 || g_nn_pf_path[0] != nnAlbedoWeights() || g_nn_pf_path[1] != nnNormalWeights())) {
            ptx_nn_prefilter_destroy(g_nn_pf);
            g_nn_pf = nullptr;
        }
        if (prefilter && !g_nn_pf) {
            check(ptx_nn_prefilter_create_from_files(g_device, w, h, nnAlbedoWeights().empty() ? nullptr : nnAlbedoWeights().c_str(),
                                                     nnNormalWeights().empty() ? nullptr : nnNormalWeights().c_str(), nnMaxMemoryMB(), &g_nn_pf), "GPUdenoise");
            memcpy(g_nn_pf_key, key, sizeof key);
            g_nn_pf_path[0] = nnAlbedoWeights(); g_nn_pf_path[1] = nnNormalWeights();
        }
        if (g_nn_pf) check(ptx_denoise_nn_prefiltered(g_tracer, g_nn, g_nn_pf, &nnParams(), &nnPrefilterParams(), g_last_iter), "GPUdenoise");
        else
        check(ptx_denoise_nn(g_tracer, g_nn, &nnParams(), g_last_iter), "GPUdenoise");
    } else if (denoiseMeasured() && !denoiseTemporal()) {
        check(ptx_denoise_measured(g_tracer, g_moments, &denoiseParams(), &varianceParams(), 0, g_last_iter), "GPUdenoise");
    } else if (denoiseTemporal()) {
        const int w = hst_scene->state.camera.resolution[0], h = hst_scene->state.camera.resolution[1];
        const int key[3] = {g_device, w, h};
        if (g_temporal && memcmp(key, g_temporal_key, sizeof key) != 0) {     // another device or resolution (g_moments looks after itself)
            ptx_temporal_destroy(g_temporal);
            g_temporal = nullptr;
        }
        if (!g_temporal) {
            check(ptx_temporal_create(g_device, w, h, &g_temporal), "GPUdenoise");
            memcpy(g_temporal_key, key, sizeof key);
        }
        if (denoiseMeasured())       // (pathtraceInit reset g_moments with the accumulation: its batches are this view's alone)
            check(ptx_denoise_temporal_measured(g_tracer, g_temporal, g_moments, &denoiseParams(), &temporalParams(), &varianceParams(), 0,
                                                g_last_iter), "GPUdenoise");
        else if (denoiseVariance())
            check(ptx_denoise_variance(g_tracer, g_temporal, &denoiseParams(), &temporalParams(), &varianceParams(), g_last_iter), "GPUdenoise");
        else
            check(ptx_denoise_temporal(g_tracer, g_temporal, &denoiseParams(), &temporalParams(), g_last_iter), "GPUdenoise");
    } else if (denoiseVariance()) {
        check(ptx_denoise_variance(g_tracer, nullptr, &denoiseParams(), nullptr, &varianceParams(), g_last_iter), "GPUdenoise");
    } else {
        check(ptx_denoise(g_tracer, &denoiseParams(), g_last_iter), "GPUdenoise");
    }
    g_output_on_device = keep_on_device;
    if (!keep_on_device) check(ptx_read_denoised(g_tracer, &hst_scene->state.output[0].x), "GPUdenoise readback");
}

// the same two under the reference's names, for translation units without HIP's vector types (see pathtrace_api.h)
void pathtrace(void *pbo, int frame, int iter) { mi355x::pathtrace_raw(pbo, frame, iter); }
void sendToGPU(void *pbo, int iter) { mi355x::sendToGPU_raw(pbo, iter); }

ptx_tracer *pathtraceHandle() { return g_tracer; }
