// pt_guides_follow.hip -- the denoiser's guides followed through mirrors and glass (ptx_set_guide_bounces; definition in
// include/mi355x_pathtracer.h and DESIGN.md 10 "Guides through mirrors and glass"): every guide ray -- the pixel-centre pinhole ray, or
// each of the K camera rays of the sampled guides -- is continued through perfectly specular surfaces by the path's own rule, and the
// surface seen at the end of the chain is recorded in place of the first hit.  A unit of its own, compiled once at the exact level
// with pt_guides.hip's flags; k_gbuffer (pt_engine.hip) and k_guides (pt_guides.hip) stay what bounces = 0 launches.  This unit
// exports the launcher ensure_gbuffer calls (pt_denoise.h).
#include "pt_kernels.h"
#include "pt_denoise.h"

namespace {

// The deterministic parts of scatterRayT (pt_device.h), statement for statement, for a material the chain follows (reflective, or
// else refractive): the reflective branch whole -- it draws nothing -- and the refractive branch with its random draw taken as "not
// reflected", i.e. refract() unless the branch's own total-internal-reflection test sends the ray to reflect().  ps.color is the
// throughput T.
PT_DEV void followSpecular(PathState &ps, vec3 intersect, vec3 n, const DMaterial &m) {
    if (m.hasReflective > 0) {
        vec3 reflectDir = reflect(ps.d, n);
        float spec = powf_own(fmax_glm(dot(neg(ps.d), reflectDir), 0.0f), m.exponent);
        ps.color = mul(ps.color, scale(V3(m.speccolor[0], m.speccolor[1], m.speccolor[2]), m.hasReflective * spec));
        ps.o = add(intersect, scale(n, 0.01f));
        ps.d = reflectDir;
    } else {
        float IoR1 = 1.0f;
        float IoR2 = m.ior;
        float cosTheta = dot(neg(ps.d), n);
        if (cosTheta < 0) {
            n = scale(n, -1.0f);
            IoR1 = IoR2;
            IoR2 = 1.0f;
            cosTheta = __builtin_fabsf(cosTheta);
        }
        float sinTheta = (float)__builtin_sqrt(1.0 - (double)(cosTheta * cosTheta));
        vec3 nd;
        if (IoR1 / IoR2 * sinTheta > 1.0f) nd = reflect(ps.d, n);
        else nd = refract(ps.d, n, IoR1 / IoR2);
        ps.d = nd;
        ps.color = mul(ps.color, V3(m.speccolor[0], m.speccolor[1], m.speccolor[2]));
        ps.o = add(intersect, scale(nd, 0.01f));
    }
}

// k_guides' frame -- one thread per pixel, the 64 x 4 workgroup, the K loop, the thirteen accumulators, one float4 / int2 store per
// array -- around a chain of at most bounces + 1 segments per sample.  The segment loop's bound is uniform and intersectScene has one
// call site, which the wave's lanes reach together in every round; a lane whose chain has ended is masked until the round in which no
// lane is live.  The record (hit, point, throughput on arrival) is overwritten by every hit, so a continued ray that misses leaves
// the record of the specular surface it left, and a first segment that misses leaves none.  t is summed in segment order, beginning
// with the first.  With aa = dof = 0, count = 1 this is the pixel-centre mode; a ray that is never followed multiplies its albedo by
// T = (1, 1, 1) and gets k_gbuffer's / k_guides' record bit for bit.
// (4 waves per SIMD, as k_guides: the chain state -- throughput, record, point, t -- next to its sums and a whole intersectScene still
//  fits 128 registers without scratch; tests/test_build_resources_guides_follow.py holds it there and reports the count)
__global__ __launch_bounds__(PT_BX * PT_BY, 4) void k_guides_follow(const DScene sc, const DCamera cam, int traceDepth, int aa, int dof,
                                                                    int iter_first, int count, int bounces, float4 *__restrict__ nh,
                                                                    float4 *__restrict__ xt, float4 *__restrict__ alb,
                                                                    int2 *__restrict__ ids) {
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
        Hit rec;
        rec.t = -1.f; rec.n = V3(0.f, 0.f, 0.f); rec.u = rec.v = 0.f; rec.geom = rec.mat = 0; rec.ncode = 0;
        vec3 rp = V3(0.f, 0.f, 0.f), rT = ps.color;
        float ts = 0.f;
        bool live = true;
#pragma unroll 1
        for (int seg = 0; seg <= bounces; seg++) {
            if (!__any(live)) break;
            if (live) {
                Ray r; r.o = ps.o; r.d = ps.d;
                Hit h;
                intersectScene(sc, r, h);
                live = h.t > 0.f;
                if (live) {
                    rp = add(r.o, scale(r.d, h.t));
                    ts = seg == 0 ? h.t : ts + h.t;
                    rec = h; rT = ps.color;
                    const DMaterial m = getMaterial(sc, h.mat);
                    live = seg < bounces && geomType(sc, h.geom) != G_OBJ && !(m.emittance > 0.0f) &&
                           (m.hasReflective > 0 || m.hasRefractive > 0);
                    if (live) followSpecular(ps, rp, h.n, m);
                }
            }
        }
        if (rec.t > 0.f) {
            float a[3];
            write_albedo(sc, rec, a);
            const vec3 ta = mul(rT, V3(a[0], a[1], a[2]));
            if (hits == 0) {
                sn = rec.n; sx = rp; st = ts; sa = ta;
                mat = rec.mat; geom = rec.geom;
            } else {
                sn = add(sn, rec.n); sx = add(sx, rp); st = st + ts; sa = add(sa, ta);
            }
            hits++;
        }
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

hipError_t pt_guides_follow_enqueue(hipStream_t st, const DScene &sc, const DCamera &cam, int traceDepth, int aa, int dof, int iter_first,
                                    int count, int bounces, float4 *nh, float4 *xt, float4 *alb, int2 *ids) {
    hipLaunchKernelGGL(k_guides_follow, pt_pixel_grid(cam.resx, cam.resy), dim3(PT_BX, PT_BY), 0, st, sc, cam, traceDepth, aa, dof, iter_first,
                       count, bounces, nh, xt, alb, ids);
    return hipGetLastError();
}
