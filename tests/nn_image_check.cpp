// nn_image_check.cpp -- csrc/pt_nn_image.h, the arithmetic of the network denoiser's image descriptors, and csrc/oidn_api.h's weight-name
// table, as a stand-alone program for AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_nn_image_cpu.py compiles and runs it;
// host only, no device, and no byte of an image is touched: the pointers are numbers).  Over a few thousand random descriptors: a
// descriptor built to be valid is accepted and its view addresses every channel inside its interval, the interval's ends are channel
// (0, 0, 0) and the byte after channel (W - 1, H - 1, 2), two intervals meet exactly when a brute-force walk of their ends says so, and
// each rule refuses the descriptor that breaks it alone.  At 16384 x 16384 with a 16-byte stride the products pass 2^32.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <random>
#include <string>

#include "pt_nn_image.h"
#include "oidn_api.h"

static long failures = 0, checked = 0;
#define CHECK(cond, what) do { checked++; if (!(cond)) { if (failures++ < 40) printf("FAIL %s (line %d)\n", what, __LINE__); } } while (0)

static bool refused(int w, int h, const ptx_nn_image &d, const char *rule) {
    PtNnImageView v;
    const std::string why = pt_nn_image_view(w, h, d, v);
    return why.find(rule) != std::string::npos;
}

int main() {
    std::mt19937_64 rng(12345);
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (int it = 0; it < 4000; it++) {
        const int w = (int)pick(1, it % 50 == 0 ? 16384 : 97), h = (int)pick(1, it % 50 == 1 ? 16384 : 61);
        ptx_nn_image d;
        d.format = (int)pick(1, 2);
        const size_t size = pt_nn_image_channel(d.format);
        d.ptr = (const void *)(uintptr_t)(pick(1, 1 << 20) * 16);
        d.byte_offset = pick(0, 64) * size;
        const size_t ps = (3 + pick(0, 5)) * size;
        d.pixel_stride = pick(0, 1) ? ps : (ps == 3 * size ? 0 : ps);
        const size_t rs = ((size_t)w + pick(0, 9)) * ps;
        d.row_stride = rs == (size_t)w * ps && pick(0, 1) ? 0 : rs;
        PtNnImageView v;
        const std::string why = pt_nn_image_view(w, h, d, v);
        CHECK(why.empty(), "a valid descriptor is accepted");
        CHECK(v.base == (uintptr_t)d.ptr + d.byte_offset && v.pixel_stride == ps && v.row_stride == rs, "the view's defaults");
        uintptr_t lo, hi;
        pt_nn_image_interval(v, w, h, lo, hi);
        CHECK(lo == v.at(0, 0, 0) && hi == v.at((size_t)w - 1, (size_t)h - 1, 2) + size, "the interval's ends");
        CHECK(hi - lo == ((size_t)h - 1) * rs + ((size_t)w - 1) * ps + 3 * size, "the interval's length");
        for (int k = 0; k < 8; k++) {
            const size_t x = pick(0, (uint64_t)w - 1), y = pick(0, (uint64_t)h - 1), c = pick(0, 2);
            const uintptr_t a = v.at(x, y, c);
            CHECK(a >= lo && a + size <= hi && a % size == 0, "a channel lies in the interval, aligned");
            CHECK(a == (uintptr_t)d.ptr + d.byte_offset + y * rs + x * ps + c * size, "the address");
        }
        // a second interval near the first: meet <=> some byte is in both
        const uintptr_t len = hi - lo, blo = lo - std::min<uintptr_t>(lo, pick(0, 2 * len)) + pick(0, 2 * len), bhi = blo + pick(1, len + 8);
        const bool brute = std::max(lo, blo) < std::min(hi, bhi);
        CHECK(pt_nn_intervals_meet(lo, hi, blo, bhi) == brute && pt_nn_intervals_meet(blo, bhi, lo, hi) == brute, "intervals meet");
        CHECK(!pt_nn_intervals_meet(lo, hi, hi, hi + 4) && !pt_nn_intervals_meet(lo - std::min<uintptr_t>(lo, 4), lo, lo, hi), "touching intervals do not meet");
        CHECK(pt_nn_intervals_meet(lo, hi, hi - 1, hi + 4), "one shared byte meets");
        // each rule alone
        ptx_nn_image b = d;
        b.format = (int)pick(3, 9);
        CHECK(refused(w, h, b, "unknown format"), "unknown format");
        b = d; b.pixel_stride = 3 * size - size;
        CHECK(refused(w, h, b, "below the pixel's size"), "pixel stride below the pixel");
        b = d; b.pixel_stride = ps; b.row_stride = (size_t)w * ps - size;
        CHECK(refused(w, h, b, "below width * pixel stride"), "row stride below the row");
        b = d; b.pixel_stride = ps; b.row_stride = rs + size;
        CHECK(refused(w, h, b, "not a multiple of the pixel stride"), "row stride no multiple of the pixel stride");
        b = d; b.byte_offset = d.byte_offset + 1;
        CHECK(refused(w, h, b, "ptr + byte_offset is not a multiple of the channel size"), "misaligned origin");
        b = d; b.pixel_stride = ps + 1; b.row_stride = ((size_t)w + 1) * (ps + 1);
        CHECK(refused(w, h, b, "the pixel stride is not a multiple of the channel size"), "misaligned pixel stride");
    }
    {   // the largest tiled frame of float4 / half4 pixels: 2^28 pixels of 16 bytes
        const int w = 16384, h = 16384;
        ptx_nn_image d = {(const void *)(uintptr_t)0x7f0000000000ull, PTX_NN_FORMAT_FLOAT3, 0, 16, 0};
        PtNnImageView v;
        CHECK(pt_nn_image_view(w, h, d, v).empty() && v.row_stride == (size_t)262144, "16384 x 16384 float4");
        uintptr_t lo, hi;
        pt_nn_image_interval(v, w, h, lo, hi);
        CHECK(hi - lo == 4294967296ull - 4 && hi - lo > 0xffffffffull - 8, "the interval passes 2^32 - 8");
        CHECK(v.at(16383, 16383, 2) - v.base == 4294967296ull - 16 + 8, "the last channel's offset");
        d.row_stride = (size_t)w * 16 + 16 * 1024;
        CHECK(pt_nn_image_view(w, h, d, v).empty(), "with a row pitch");
        pt_nn_image_interval(v, w, h, lo, hi);
        CHECK(hi - lo == 16383ull * (262144 + 16384) + 16383ull * 16 + 12, "its interval is above 2^32");
    }
    {   // the veneer's weight table (core/unet.cpp:290-336 restated)
        struct Case { bool c, a, n, hdr, srgb, clean; const char *name; int role; } cases[] = {
            {true, false, false, false, false, false, "rt_ldr", 0},      {true, false, false, true, false, false, "rt_hdr", 0},
            {true, true, false, false, false, false, "rt_ldr_alb", 0},   {true, true, false, true, false, false, "rt_hdr_alb", 0},
            {true, true, true, false, false, false, "rt_ldr_alb_nrm", 0}, {true, true, true, true, false, false, "rt_hdr_alb_nrm", 0},
            {true, true, true, false, false, true, "rt_ldr_calb_cnrm", 0}, {true, true, true, true, false, true, "rt_hdr_calb_cnrm", 0},
            {true, true, false, false, true, true, "rt_ldr_alb", 0},     {false, true, false, false, false, false, "rt_alb", 1},
            {false, true, false, false, true, false, "rt_alb", 1},       {false, false, true, false, false, false, "rt_nrm", 2},
            {true, false, true, false, false, false, nullptr, 0},        {false, true, true, false, false, false, nullptr, 0},
            {false, true, false, true, false, false, nullptr, 0},        {false, false, true, true, false, false, nullptr, 0},
            {false, false, true, false, true, false, nullptr, 0},        {false, false, false, false, false, false, nullptr, 0},
            {true, false, false, true, true, false, nullptr, 0}};
        for (const Case &k : cases) {
            int role = -1;
            const char *why = nullptr;
            const char *name = oidn::detail::weightsName(k.c, k.a, k.n, k.hdr, k.srgb, k.clean, &role, &why);
            CHECK((name == nullptr) == (k.name == nullptr) && (!name || !strcmp(name, k.name)), "the weight file's name");
            CHECK(name ? (why == nullptr && role == k.role) : (why != nullptr && strlen(why) > 10), "the role, or the reason");
        }
        int role;
        const char *why;
        oidn::detail::weightsName(true, false, true, false, false, false, &role, &why);
        CHECK(!strcmp(why, "unsupported combination of input features"), "colour + normal without albedo");
    }
    printf("nn_image_check: %ld failures in %ld checks\n", failures, checked);
    return failures ? 1 : 0;
}
