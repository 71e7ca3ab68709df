// unit_rsqrt_check.cpp -- stand-alone check of pt_device.h's pt_unit_rsqrt_bits / pt_in_unit_window (1 / sqrt of an operand next to 1,
// the second normalize of a unit vector).  tests/test_unit_rsqrt.py compiles this file (host pass) with -fsanitize=address,undefined and the
// library's own flags (-ffp-contract=off: sqrtf and the division below are the two correctly rounded operations) and runs it.
//  1. every binary32 of the window [1 - W ulps, 1 + W ulps]: the integer mapping against 1.0f / sqrtf(s); the operands are counted and the
//     count must be 2 W + 1.  The formula is also followed outwards until it first fails, to show how far from its limit the window lies.
//  2. the window's derivation, with a fixed seed: the largest |bits(dot(v, v)) - bits(1)| over v = normalize(u) -- 10^8 random u and the
//     adversarial ones (axis vectors, components of equal size, components 2^+-20 apart, all signs) -- with the dot product as the exact
//     level forms it and as the contracted level does (fused); it must equal PT_UNIT_DMAX, and PT_UNIT_W twice that.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pt_device.h"

using namespace ptd;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float from_bits(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
static const uint32_t ONE = 0x3f800000u;

static uint32_t ieee(uint32_t sbits) {
    volatile float s = from_bits(sbits);
    volatile float r = sqrtf(s);
    volatile float q = 1.0f / r;
    return bits(q);
}

// |bits(dot(v, v)) - bits(1)| for v = normalize(u), the larger of the separate and the fused dot product (the first normalize fused too)
static uint32_t distance_from_one(vec3 u) {
    uint32_t worst = 0;
    for (int fused = 0; fused < 2; fused++) {
        float s = fused ? fmaf(u.z, u.z, fmaf(u.y, u.y, u.x * u.x)) : dot(u, u);
        if (!(s > 0.f) || isinf(s)) return 0;                                      // (no direction: normalize gives NaN or zero)
        const vec3 v = scale(u, 1.0f / sqrtf(s));
        const float t = fused ? fmaf(v.z, v.z, fmaf(v.y, v.y, v.x * v.x)) : dot(v, v);
        const int32_t d = (int32_t)(bits(t) - ONE);
        const uint32_t a = (uint32_t)(d < 0 ? -d : d);
        if (a > worst) worst = a;
    }
    return worst;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {                                                             // xorshift64*
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545f4914f6cdd1dull) >> 32);
}
static float rnd_unit() { return (float)(rnd() >> 8) * (1.0f / 8388608.0f) - 1.0f; }   // [-1, 1)

int main(int argc, char **argv) {
    const long long nrandom = argc > 1 ? atoll(argv[1]) : 100000000ll;
    // ---- 1. the mapping on the whole window
    long long checked = 0, wrong = 0;
    for (uint32_t sb = ONE - PT_UNIT_W; sb <= ONE + PT_UNIT_W; sb++) {
        CHECK(pt_in_unit_window(sb));
        if (pt_unit_rsqrt_bits(sb) != ieee(sb)) { wrong++; printf("operand %08x: mapping %08x, 1/sqrt %08x\n", sb, pt_unit_rsqrt_bits(sb), ieee(sb)); }
        checked++;
    }
    CHECK(!pt_in_unit_window(ONE - PT_UNIT_W - 1) && !pt_in_unit_window(ONE + PT_UNIT_W + 1));
    CHECK(!pt_in_unit_window(0u) && !pt_in_unit_window(0x7f800000u) && !pt_in_unit_window(0x7fc00000u) && !pt_in_unit_window(0xbf800000u) && !pt_in_unit_window(0xffffffffu));
    printf("window: %lld operands checked, %lld differ\n", checked, wrong);
    CHECK(checked == 2ll * PT_UNIT_W + 1);
    CHECK(wrong == 0);
    uint32_t up = 0, down = 0;
    while (pt_unit_rsqrt_bits(ONE + up) == ieee(ONE + up)) up++;
    while (pt_unit_rsqrt_bits(ONE - down) == ieee(ONE - down)) down++;
    printf("the mapping holds from 1 - %u ulps to 1 + %u ulps\n", down - 1, up - 1);
    CHECK(down - 1 >= 8 * PT_UNIT_W && up - 1 >= 8 * PT_UNIT_W);
    // ---- 2. how far dot(v, v) of a normalized v lies from 1
    uint32_t worst_random = 0, worst_adv = 0;
    for (long long k = 0; k < nrandom; k++) {
        vec3 u = V3(rnd_unit(), rnd_unit(), rnd_unit());
        if ((k & 3) == 3) {                                                         // a quarter of them with components of very different size
            u.x = ldexpf(u.x, -(int)(rnd() % 24)); u.y = ldexpf(u.y, -(int)(rnd() % 24)); u.z = ldexpf(u.z, -(int)(rnd() % 24));
        }
        const uint32_t a = distance_from_one(u);
        if (a > worst_random) worst_random = a;
    }
    const float mags[] = {1.f, 0.5f, 3.f, 0.1f, 1e-3f, 7.25f, 1048576.f, 1.f / 1048576.f, 1.9999999f, 1.0000001f, 0.70710678f, 0.57735027f, 1e10f, 1e-10f};
    const int nm = (int)(sizeof mags / sizeof mags[0]);
    for (int i = 0; i < nm; i++)
        for (int j = 0; j < nm; j++)
            for (int k = 0; k < nm; k++)
                for (int sg = 0; sg < 8; sg++)
                    for (int zero = 0; zero < 8; zero++) {                          // zero: which components are dropped (axis vectors, planes)
                        if (zero == 7) continue;
                        vec3 u = V3(mags[i], mags[j], mags[k]);
                        if (sg & 1) u.x = -u.x;
                        if (sg & 2) u.y = -u.y;
                        if (sg & 4) u.z = -u.z;
                        if (zero & 1) u.x = 0.f;
                        if (zero & 2) u.y = 0.f;
                        if (zero & 4) u.z = 0.f;
                        const uint32_t a = distance_from_one(u);
                        if (a > worst_adv) worst_adv = a;
                    }
    const uint32_t worst = worst_random > worst_adv ? worst_random : worst_adv;
    printf("largest distance of dot(v, v) from 1: %u ulps over %lld random directions, %u over the adversarial ones; PT_UNIT_DMAX %u, PT_UNIT_W %u\n",
           worst_random, nrandom, worst_adv, PT_UNIT_DMAX, PT_UNIT_W);
    if (nrandom >= 100000000ll) CHECK(worst == PT_UNIT_DMAX);
    CHECK(worst <= PT_UNIT_DMAX);
    CHECK(PT_UNIT_W == 2 * PT_UNIT_DMAX);
    printf("unit_rsqrt_check: %d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
