// metrics_plan_check.cpp -- the image metrics' host-only arithmetic (mygpuraytracer_amd/csrc/pt_metrics.h) under the sanitizers, as a
// stand-alone program: the scale sizes of every frame from 1 x 1 to 400 x 400 against the pool's rule stated again here, buffer sizes
// that never under-cover a scale or a job, and the size_t arithmetic at 16384 x 16384.  tests/test_metrics_plan.py builds and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pt_metrics.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { failures++; if (failures < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// avg_pool2d(kernel 2, padding n % 2) counted window by window: windows start at -p, -p + 2, ... and must begin inside the padded row's
// first n + 2 p - 1 places
static int pooled_by_counting(int n) {
    const int p = n % 2;
    int count = 0;
    for (int start = -p; start + 2 <= n + p; start += 2) count++;
    return count;
}

static void check_frame(int w, int h) {
    ptx_metrics_plan p;
    CHECK(pt_metrics_plan(w, h, &p));
    const int smaller = w < h ? w : h;
    CHECK(p.ssim_valid == (smaller >= 11) && p.msssim_valid == (smaller > 160));
    CHECK(p.scales == (p.msssim_valid ? 5 : 1));
    int ws = w, hs = h;
    size_t floats = 0;
    for (int s = 0; s < PTX_METRICS_SCALES; s++) {
        if (s) { ws = pooled_by_counting(ws); hs = pooled_by_counting(hs); }
        CHECK(p.w[s] == ws && p.h[s] == hs && ws >= 1 && hs >= 1);
        if (s < p.scales) {
            CHECK(p.level_offset[s] == floats);                               // levels follow each other and none overlaps the next
            floats += 3 * (size_t)ws * (size_t)hs;
            CHECK(p.level_offset[s] + 3 * (size_t)ws * (size_t)hs <= p.pyramid_floats);
        }
        if (p.msssim_valid) CHECK(ws >= 11 && hs >= 11);                      // every scale of a valid MS-SSIM holds a window
        // the tiles cover the map of the scale, and no tile lies wholly outside it
        if (p.blocks[s]) {
            const size_t mw = (size_t)ws - 10, mh = (size_t)hs - 10;
            const size_t gx = (mw + p.tile_w - 1) / p.tile_w, gy = (mh + p.tile_h - 1) / p.tile_h;
            CHECK((size_t)p.blocks[s] == gx * gy && gx * p.tile_w >= mw && (gx - 1) * p.tile_w < mw && gy * p.tile_h >= mh && (gy - 1) * p.tile_h < mh);
        } else {
            CHECK(s >= p.scales || !p.ssim_valid);
        }
    }
    CHECK(p.pyramid_floats == floats);
    CHECK((size_t)p.prep_blocks * PT_METRICS_NT >= (size_t)w * h && ((size_t)p.prep_blocks - 1) * PT_METRICS_NT < (size_t)w * h);
    if (w >= 2 && h >= 2) CHECK((size_t)p.grad_blocks * PT_METRICS_NT >= ((size_t)w - 1) * ((size_t)h - 1));
    else CHECK(p.grad_blocks == 0);
    CHECK(p.map_floats == (p.ssim_valid ? ((size_t)w - 10) * ((size_t)h - 10) : 0));
    // the jobs' partials tile the partial buffer exactly
    size_t off[PT_METRICS_JOBS];
    unsigned cnt[PT_METRICS_JOBS];
    pt_metrics_jobs(p, off, cnt);
    size_t at = 0;
    for (int j = 0; j < PT_METRICS_JOBS; j++) { CHECK(off[j] == at); at += cnt[j]; }
    CHECK(at == p.partial_doubles);
    for (int j = 0; j < PT_METRICS_POINT_JOBS; j++) CHECK(cnt[j] == (unsigned)p.prep_blocks);
    CHECK(cnt[PT_METRICS_JOB_GRAD] == (unsigned)p.grad_blocks);
    for (int c = 0; c < 3; c++) CHECK(cnt[PT_METRICS_JOB_SSIM + c] == (unsigned)p.blocks[0]);
    for (int s = 0; s < PTX_METRICS_SCALES; s++)
        for (int c = 0; c < 3; c++) CHECK(cnt[PT_METRICS_JOB_MCS + 3 * s + c] == (p.msssim_valid ? (unsigned)p.blocks[s] : 0u));
}

int main() {
    for (int h = 1; h <= 400; h++)
        for (int w = 1; w <= 400; w++) check_frame(w, h);
    for (int n = 1; n <= 20000; n++) CHECK(pt_metrics_pooled(n) == pooled_by_counting(n) && pt_metrics_pooled(n) == (n + 1) / 2);

    // 16384 x 16384: 3 * 2^28 floats in level 0 alone are 3 GiB, the pyramid 4 MiB short of 4 GiB -- beyond a signed 32-bit byte count
    check_frame(16384, 16384);
    check_frame(16384, 161);
    check_frame(16383, 16381);
    ptx_metrics_plan p;
    CHECK(pt_metrics_plan(16384, 16384, &p));
    CHECK(p.pyramid_floats == 3 * ((size_t)16384 * 16384 + (size_t)8192 * 8192 + (size_t)4096 * 4096 + (size_t)2048 * 2048 + (size_t)1024 * 1024));
    CHECK(p.pyramid_floats * sizeof(float) > 0x7fffffffull && p.level_offset[4] * sizeof(float) > 0xf0000000ull);
    CHECK(p.prep_blocks == 1 << 20 && p.map_floats == (size_t)16374 * 16374);
    CHECK(p.level_offset[1] == (size_t)3 << 28);

    ptx_metrics_plan untouched;
    memset(&untouched, 0x5a, sizeof untouched);
    ptx_metrics_plan q = untouched;
    CHECK(!pt_metrics_plan(0, 4, &q) && !pt_metrics_plan(4, 0, &q) && !pt_metrics_plan(16385, 4, &q) && !pt_metrics_plan(4, -1, &q) && !pt_metrics_plan(4, 4, nullptr));
    CHECK(memcmp(&q, &untouched, sizeof q) == 0);

    float sum = 0.f;
    for (int k = 0; k < PT_METRICS_WIN; k++) { sum += PT_METRICS_TAPS_F[k]; CHECK(PT_METRICS_TAPS_F[k] == PT_METRICS_TAPS_F[PT_METRICS_WIN - 1 - k]); }
    CHECK(sum > 0.999999f && sum < 1.000001f);
    const PtMetricsTone t = pt_metrics_tone();
    CHECK(t.cb == 0.03f && t.de == 0.002f && t.df == 0.06f && t.inv_white_div > 0.8673f && t.inv_white_div < 0.8674f);
    CHECK(pt_metrics_c1() == 1e-4f && pt_metrics_c2() == 9e-4f);

    ptx_metrics_params ok = {PTX_METRICS_NONE, NAN, 0.01f, 1.f, 1.f, 0};
    CHECK(pt_metrics_params_problem(ok) == nullptr);
    ptx_metrics_params bad = ok; bad.transform = 4; CHECK(pt_metrics_params_problem(bad) != nullptr);
    bad = ok; bad.exposure = -1.f; CHECK(pt_metrics_params_problem(bad) != nullptr);
    bad = ok; bad.samples_b = 0.f; CHECK(pt_metrics_params_problem(bad) != nullptr);
    bad = ok; bad.pointwise_only = 2; CHECK(pt_metrics_params_problem(bad) != nullptr);

    printf("metrics_plan_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
