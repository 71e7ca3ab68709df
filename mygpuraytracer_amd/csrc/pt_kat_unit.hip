// pt_kat_unit.hip -- known-answer kernels for two routines of pt_device.h, at the exact level: pt_rsqrt_unit (1 / sqrt of an operand
// next to 1) against pt_rsqrt_glm, and pt_div_pairs3 (two quotients per denominator, the cube's slab test) against the divisions.
// A unit of its own: pt_engine.hip and pt_kernels.hip hold exactly the kernels tests/test_build_resources.py lists.  The entry point
// (ptx_kat_unit_rsqrt) is pt_engine.hip's, which owns the tracer; this unit exports the launcher it calls.
#include "pt_device.h"

using namespace ptd;

namespace {

__device__ __forceinline__ bool same_bits(float p, float q) { return __float_as_uint(p) == __float_as_uint(q) || (p != p && q != q); }
__device__ __forceinline__ float hide(float x) { asm volatile("" : "+v"(x)); return x; }      // (the two sides must not be merged into one computation)
__device__ __forceinline__ uint64_t mix(uint64_t z) {                                        // splitmix64
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// out[0]: operands on which pt_rsqrt_unit and pt_rsqrt_glm differ, over ALL 2^32 bit patterns (so: everything within 4 W of 1.0f, every
// fall-through, more than 2^24 random patterns); out[1]: operands inside the window (2 W + 1, or the test is empty)
__global__ void k_kat_rsqrt_unit(unsigned long long *out) {
    unsigned long long bad = 0, inside = 0;
    const unsigned long long total = 1ull << 32, step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += step) {
        const float x = hide(__uint_as_float((uint32_t)k)), y = hide(x);
        bad += same_bits(pt_rsqrt_unit(x), pt_rsqrt_glm(y)) ? 0 : 1;
        inside += pt_in_unit_window((uint32_t)k) ? 1 : 0;
    }
    if (bad) atomicAdd(&out[0], bad);
    if (inside) atomicAdd(&out[1], inside);
}

// one set of three axes through pt_div_pairs3 and through six divisions; -> number of quotients that differ
__device__ __forceinline__ int pairs_differ(const float a1[3], const float a2[3], const float d[3], unsigned long long &core) {
    float x1[3], x2[3], xd[3], y1[3], y2[3], yd[3], t1[3], t2[3];
    bool in_range = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        x1[k] = hide(a1[k]); x2[k] = hide(a2[k]); xd[k] = hide(d[k]);
        y1[k] = hide(x1[k]); y2[k] = hide(x2[k]); yd[k] = hide(xd[k]);
        in_range = in_range && pt_div_pair_in_range(a1[k], a2[k], d[k]);
    }
    core += in_range ? 1 : 0;
    pt_div_pairs3(x1, x2, xd, t1, t2);
    int bad = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) bad += (same_bits(t1[k], y1[k] / yd[k]) ? 0 : 1) + (same_bits(t2[k], y2[k] / yd[k]) ? 0 : 1);
    return bad;
}

__constant__ uint32_t SPECIAL[] = {
    0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00001u, 0x7f800001u,      // zeros, infinities, NaNs (quiet, signalling)
    0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u, 0x7f7fffffu, 0xff7fffffu,      // subnormals, the smallest normal, the largest
    0x3f800000u, 0xbf800000u, 0x3f000000u, 0xbf000000u, 0x40400000u, 0x3eaaaaabu,                  // 1, 0.5, 3, 1/3
    0x2a800000u, 0x2a7fffffu, 0xaa800000u, 0xaa7fffffu, 0x54800000u, 0x54800001u, 0xd4800000u, 0xd4800001u,      // the guard's bounds 2^-42 and 2^42 and their neighbours
    0x0c000000u, 0x0b800000u, 0x7e800000u, 0x7f000000u};                                           // biased exponents 24 and 23; 2^126 and 2^127
constexpr int NSPECIAL = sizeof(SPECIAL) / sizeof(SPECIAL[0]);

// a float with biased exponent e, random mantissa and sign
__device__ __forceinline__ float with_exponent(uint32_t e, uint64_t r) { return __uint_as_float(((uint32_t)r & 0x807fffffu) | (e << 23)); }

// out[2]: quotients that differ; out[3]: sets that took the core (or the test is empty).  Three families, `family` picks one:
//  0  every pair of biased exponents for numerator and denominator (256 x 256), `reps` random mantissas each; the second numerator is the
//     first plus one (the slab's relation) or has a random exponent of its own; the other two axes are benign (so the core can run) or
//     a neighbouring case (so one axis out of range sends all three to the divisions)
//  1  every triple of the special values above on one axis, the other two benign; and the same value on all three axes
//  2  n random sets from the slab loop's range: numerators -0.5 - o and +0.5 - o with |o| < 63.5, 2^-40 <= |d| <= 1
__global__ void k_kat_div_pairs(unsigned long long *out, int family, unsigned long long n) {
    unsigned long long bad = 0, core = 0;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        float a1[3] = {1.0f, -3.0f, 0.25f}, a2[3] = {2.0f, -2.0f, 1.25f}, d[3] = {0.5f, -0.75f, 0.001f};
        const uint64_t r0 = mix(i * 4 + family), r1 = mix(r0), r2 = mix(r1);
        if (family == 0) {
            const uint32_t ea = (uint32_t)(i & 255), ed = (uint32_t)((i >> 8) & 255);
            const int axes = (i >> 16) & 1 ? 3 : 1;                                 // odd repetition: all three axes carry such a case
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (k >= axes) continue;
                const uint64_t r = k == 0 ? r0 : k == 1 ? r1 : r2;
                a1[k] = with_exponent(k == 0 ? ea : (ea + 7 * k) & 255, r);
                d[k] = with_exponent(k == 0 ? ed : (ed + 11 * k) & 255, r >> 24);
                a2[k] = (r >> 60) & 1 ? a1[k] + 1.0f : with_exponent((uint32_t)(r >> 48) & 255, r >> 20);
            }
        } else if (family == 1) {
            const int ia = (int)(i % NSPECIAL), ib = (int)(i / NSPECIAL % NSPECIAL), ic = (int)(i / (NSPECIAL * NSPECIAL) % NSPECIAL);
            const bool all_axes = i >= (unsigned long long)NSPECIAL * NSPECIAL * NSPECIAL;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (k > 0 && !all_axes) continue;
                a1[k] = __uint_as_float(SPECIAL[ia]); a2[k] = __uint_as_float(SPECIAL[ib]); d[k] = __uint_as_float(SPECIAL[ic]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint64_t r = k == 0 ? r0 : k == 1 ? r1 : r2;
                const float o = with_exponent(127 - 30 + (uint32_t)((r >> 32) % 36), r);                // 2^-30 <= |o| < 2^6
                const float o63 = __builtin_fabsf(o) < 63.5f ? o : 0.5f * o;
                a1[k] = -0.5f - o63; a2[k] = +0.5f - o63;
                d[k] = with_exponent(127 - 40 + (uint32_t)((r >> 40) % 40), r >> 8);                    // 2^-40 <= |d| < 1
                if (((r >> 56) & 63) == 0) d[k] = (r >> 62) & 1 ? 1.0f : -1.0f;
            }
        }
        bad += pairs_differ(a1, a2, d, core);
    }
    if (bad) atomicAdd(&out[2], bad);
    if (core) atomicAdd(&out[3], core);
}

}  // namespace

namespace ptd {
// out: four zeroed counters on the device (see the kernels); random_sets: family 2's n
void launch_kat_unit_rsqrt(int cus, hipStream_t stream, unsigned long long *out, int exponent_reps, unsigned long long random_sets) {
    const dim3 grid(cus * 8), block(256);
    hipLaunchKernelGGL(k_kat_rsqrt_unit, grid, block, 0, stream, out);
    hipLaunchKernelGGL(k_kat_div_pairs, grid, block, 0, stream, out, 0, 65536ull * (unsigned long long)exponent_reps);
    hipLaunchKernelGGL(k_kat_div_pairs, grid, block, 0, stream, out, 1, 2ull * NSPECIAL * NSPECIAL * NSPECIAL);
    hipLaunchKernelGGL(k_kat_div_pairs, grid, block, 0, stream, out, 2, random_sets);
}
}  // namespace ptd
