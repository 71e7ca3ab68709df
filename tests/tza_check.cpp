// tza_check.cpp -- csrc/pt_tza.h on hostile blobs, as a stand-alone program for AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_nn_cpu.py compiles and runs it; host only, no device).  A small valid network blob is built in code; it must be
// accepted.  Then: the blob truncated at every byte, a table offset beyond the end, a name length running past the end, dims whose
// product overflows 64 bits, a data offset + size that wraps around -- every one refused with a message, each blob in a heap
// allocation of exactly its size so that a read past its end is seen.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "pt_tza.h"

static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { failures++; printf("FAIL %s (line %d)\n", what, __LINE__); } } while (0)

struct Entry { std::string name; std::vector<uint32_t> dims; std::string layout; char type; uint64_t offset; };

template <class T> static void put(std::vector<uint8_t> &b, T v) { const uint8_t *p = reinterpret_cast<const uint8_t *>(&v); b.insert(b.end(), p, p + sizeof(T)); }

static std::vector<uint8_t> table_blob(std::vector<uint8_t> data, const std::vector<Entry> &entries, const uint16_t *name_len_override = nullptr) {
    std::vector<uint8_t> b;
    put<uint16_t>(b, 0x41D7); put<uint8_t>(b, 2); put<uint8_t>(b, 0); put<uint64_t>(b, 0);
    b.insert(b.end(), data.begin(), data.end());
    const uint64_t table = b.size();
    memcpy(&b[4], &table, 8);
    put<uint32_t>(b, (uint32_t)entries.size());
    for (const Entry &e : entries) {
        put<uint16_t>(b, name_len_override ? *name_len_override : (uint16_t)e.name.size());
        b.insert(b.end(), e.name.begin(), e.name.end());
        put<uint8_t>(b, (uint8_t)e.dims.size());
        for (uint32_t d : e.dims) put<uint32_t>(b, d);
        b.insert(b.end(), e.layout.begin(), e.layout.end());
        put<char>(b, e.type);
        put<uint64_t>(b, e.offset);
    }
    return b;
}

// the whole network with one channel everywhere but the 3 in and 3 out: 16 weights and 16 biases
static std::vector<uint8_t> valid_blob(char type) {
    static const char *names[16] = {"enc_conv0", "enc_conv1", "enc_conv2", "enc_conv3", "enc_conv4", "enc_conv5a", "enc_conv5b", "dec_conv4a",
                                    "dec_conv4b", "dec_conv3a", "dec_conv3b", "dec_conv2a", "dec_conv2b", "dec_conv1a", "dec_conv1b", "dec_conv0"};
    static const uint32_t cin[16] = {3, 1, 1, 1, 1, 1, 1, 2, 1, 2, 1, 2, 1, 4, 1, 1}, cout[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3};
    const size_t esize = type == 'f' ? 4 : 2;
    std::vector<uint8_t> data;
    std::vector<Entry> entries;
    for (int i = 0; i < 16; i++) {
        entries.push_back({std::string(names[i]) + ".weight", {cout[i], cin[i], 3, 3}, "oihw", type, 12 + data.size()});
        data.resize(data.size() + esize * cout[i] * cin[i] * 9, 0);
        entries.push_back({std::string(names[i]) + ".bias", {cout[i]}, "x", type, 12 + data.size()});
        data.resize(data.size() + esize * cout[i], 0);
    }
    return table_blob(data, entries);
}

// the plan of a copy of `b` in an allocation of exactly its size
static bool plan_of(const std::vector<uint8_t> &b, std::string &err, size_t bytes) {
    std::unique_ptr<uint8_t[]> heap(new uint8_t[bytes ? bytes : 1]);
    memcpy(heap.get(), b.data(), bytes);
    PtNnPlan plan;
    return pt_nn_plan(heap.get(), bytes, plan, err);
}

int main() {
    std::string err;
    for (const char type : {'f', 'h'}) {
        const std::vector<uint8_t> ok = valid_blob(type);
        CHECK(plan_of(ok, err, ok.size()), "the valid blob is accepted");
        int refused = 0;
        for (size_t n = 0; n < ok.size(); n++) {
            err.clear();
            if (!plan_of(ok, err, n) && !err.empty()) refused++;
        }
        CHECK(refused == (int)ok.size(), "truncated at every byte: refused with a message");
        printf("type %c: %zu bytes, %d truncations refused\n", type, ok.size(), refused);
    }
    const std::vector<uint8_t> ok = valid_blob('f');
    {   // a table offset beyond the end, and one that wraps a pointer
        for (const uint64_t off : {(uint64_t)ok.size() + 1, (uint64_t)1 << 40, ~(uint64_t)0, ~(uint64_t)0 - 3}) {
            std::vector<uint8_t> b = ok;
            memcpy(&b[4], &off, 8);
            CHECK(!plan_of(b, err, b.size()) && err.find("table") != std::string::npos, "table offset beyond the end");
        }
    }
    {   // a name length running past the end
        const uint16_t len = 60000;
        const std::vector<uint8_t> b = table_blob(std::vector<uint8_t>(36, 0), {{"enc_conv0.weight", {1, 1, 3, 3}, "oihw", 'f', 12}}, &len);
        CHECK(!plan_of(b, err, b.size()) && err.find("name") != std::string::npos, "name length past the end");
    }
    {   // dims whose product overflows 64 bits (and one whose byte size does)
        const std::vector<uint8_t> b = table_blob({}, {{"enc_conv0.weight", {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, "oihw", 'f', 12}});
        CHECK(!plan_of(b, err, b.size()) && err.find("enc_conv0.weight") != std::string::npos && err.find("overflow") != std::string::npos, "dims overflow");
        const std::vector<uint8_t> c = table_blob({}, {{"enc_conv0.bias", {0x80000000u, 0x80000000u}, "xx", 'f', 12}});
        CHECK(!plan_of(c, err, c.size()), "layout xx");
        const std::vector<uint8_t> d = table_blob({}, {{"enc_conv0.weight", {0x80000000u, 0x80000000u, 2, 2}, "oihw", 'f', 12}});
        CHECK(!plan_of(d, err, d.size()) && err.find("enc_conv0.weight") != std::string::npos, "byte size overflow");
        const std::vector<uint8_t> z = table_blob({}, {{"enc_conv0.weight", {1, 0, 3, 3}, "oihw", 'f', 12}});
        CHECK(!plan_of(z, err, z.size()) && err.find("is 0") != std::string::npos, "a dimension of 0");
    }
    {   // data offset + size wrapping around
        for (const uint64_t off : {~(uint64_t)0, ~(uint64_t)0 - 35, ~(uint64_t)0 - 36, (uint64_t)1 << 63}) {
            const std::vector<uint8_t> b = table_blob(std::vector<uint8_t>(36, 0), {{"enc_conv0.weight", {1, 1, 3, 3}, "oihw", 'f', off}});
            CHECK(!plan_of(b, err, b.size()) && err.find("enc_conv0.weight") != std::string::npos && err.find("past") != std::string::npos, "offset + size wraps");
        }
    }
    {   // bad magic, version, layout, type
        std::vector<uint8_t> b = ok; b[0] ^= 1;
        CHECK(!plan_of(b, err, b.size()), "magic");
        b = ok; b[2] = 1;
        CHECK(!plan_of(b, err, b.size()) && err.find("version") != std::string::npos, "version");
        const std::vector<uint8_t> t = table_blob(std::vector<uint8_t>(36, 0), {{"enc_conv0.weight", {1, 1, 3, 3}, "oihw", 'b', 12}});
        CHECK(!plan_of(t, err, t.size()) && err.find("data type") != std::string::npos, "type b");
    }
    // the exact conversion of every half: sign * m * 2^-24 below the normals, sign * (1024 + m) * 2^(e - 25) among them
    for (uint32_t h = 0; h < 65536; h++) {
        const float f = PtTzaTensor::half_bits_to_float((uint16_t)h);
        const int e = (h >> 10) & 31, m = h & 1023;
        const float sign = (h & 0x8000) ? -1.f : 1.f;
        bool good;
        if (e == 31) good = m ? f != f : (std::isinf(f) && (f < 0) == (sign < 0));
        else good = f == sign * ldexpf((float)(e ? 1024 + m : m), e ? e - 25 : -24) && std::signbit(f) == (sign < 0);
        if (!good) { failures++; printf("FAIL half %04x\n", h); break; }
    }
    printf("tza_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
