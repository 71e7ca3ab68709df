// pt_guides.hip -- the denoiser's sampled guides (ptx_set_guide_samples; definition in include/mi355x_pathtracer.h and DESIGN.md 10):
// the G-buffer averaged over the camera rays the frame itself was rendered with, antialiasing jitter and lens included, in place of
// k_gbuffer's one pixel-centre pinhole ray (pt_engine.hip).  A unit of its own, compiled once at the exact level with pt_engine.hip's
// flags: pt_engine.hip holds exactly the kernels tests/test_build_resources.py lists.  The entry points are pt_engine.hip's, which
// owns the tracer; this unit exports the launcher ensure_gbuffer calls (pt_denoise.h).
#include "pt_kernels.h"
#include "pt_denoise.h"

namespace {

// One thread per pixel, the filter's 64 x 4 workgroup: a wave is one 64-pixel row segment, whose rays of one iteration leave neighbouring
// pixels and walk the same part of the BVH.  Iteration i's camera ray is a pure function of (i, pixel, traceDepth) -- generateRay seeds
// its generators with nothing else -- so the K rays here ARE the path kernels' camera rays of iterations iter_first .. iter_first + K - 1.
// The sums begin with the first hit sample (an assignment, not 0 + v: one sample's -0 survives, so aa = dof = 0, K = 1 is k_gbuffer's
// record) and add the later ones in iteration order; a miss adds nothing.  Thirteen accumulators, one float4 / int2 store per array.
// (4 waves per SIMD: 128 registers, what a whole intersectScene next to the sums needs -- tests/test_build_resources_guides.py)
__global__ __launch_bounds__(PT_BX * PT_BY, 4) void k_guides(const DScene sc, const DCamera cam, int traceDepth, int aa, int dof, int iter_first,
                                                             int count, float4 *__restrict__ nh, float4 *__restrict__ xt,
                                                             float4 *__restrict__ alb, int2 *__restrict__ ids) {
    const int x = blockIdx.x * PT_BX + threadIdx.x, y = blockIdx.y * PT_BY + threadIdx.y;
    if (x >= cam.resx || y >= cam.resy) return;
    const size_t i = (size_t)x + (size_t)y * cam.resx;
    vec3 sn = V3(0.f, 0.f, 0.f), sx = V3(0.f, 0.f, 0.f), sa = V3(0.f, 0.f, 0.f);
    float st = 0.f;
    int hits = 0, mat = 0, geom = 0;
#pragma unroll 1
    for (int k = 0; k < count; k++) {
        PathState ps;
        generateRay(cam, iter_first + k, traceDepth, aa != 0, dof != 0, x, y, ps);
        Ray r; r.o = ps.o; r.d = ps.d;
        Hit h;
        intersectScene(sc, r, h);
        if (!(h.t > 0.f)) continue;
        float a[3];
        write_albedo(sc, h, a);
        const vec3 p = add(r.o, scale(r.d, h.t));
        if (hits == 0) {
            sn = h.n; sx = p; st = h.t; sa = V3(a[0], a[1], a[2]);
            mat = h.mat; geom = h.geom;
        } else {
            sn = add(sn, h.n); sx = add(sx, p); st = st + h.t; sa = add(sa, V3(a[0], a[1], a[2]));
        }
        hits++;
    }
    if (hits > 0) {
        const float fh = (float)hits, fk = (float)count;
        nh[i] = make_float4(sn.x / fh, sn.y / fh, sn.z / fh, 1.f);
        xt[i] = make_float4(sx.x / fh, sx.y / fh, sx.z / fh, st / fh);
        alb[i] = make_float4(sa.x / fk, sa.y / fk, sa.z / fk, fh / fk);      // (.w = the coverage: no filter kernel reads it)
        ids[i] = make_int2(mat, geom);
    } else {
        nh[i] = xt[i] = alb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        ids[i] = make_int2(0, 0);
    }
}

}  // namespace

hipError_t pt_guides_enqueue(hipStream_t st, const DScene &sc, const DCamera &cam, int traceDepth, int aa, int dof, int iter_first, int count,
                             float4 *nh, float4 *xt, float4 *alb, int2 *ids) {
    hipLaunchKernelGGL(k_guides, pt_pixel_grid(cam.resx, cam.resy), dim3(PT_BX, PT_BY), 0, st, sc, cam, traceDepth, aa, dof, iter_first, count,
                       nh, xt, alb, ids);
    return hipGetLastError();
}
