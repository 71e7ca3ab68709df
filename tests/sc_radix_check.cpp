// sc_radix_check.cpp -- StreamCompaction::Records::radixSortByKey (mygpuraytracer_amd/csrc/stream_compaction_api.h) as a caller with
// kernels of their own would use it: device arrays of structs of their own, int, unsigned and float keys read out of the records or
// from an array of their own, against std::stable_sort on the host with the header's key map restated.  Built with hipcc and run by
// the GPU tier (tests/test_gpu_sc_radix.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mygpuraytracer_amd/csrc/stream_compaction_api.h"

struct Hit { float t; int pixel; float n[3]; };               // 20 bytes: the dword path
struct Seg { float o[4], d[4]; unsigned morton; int id, pad[2]; };      // 48 bytes: the 16-byte path

#define HIP_OK(expr) do { if ((expr) != hipSuccess) { printf("%s failed\n", #expr); return 1; } } while (0)

static unsigned bits_of(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static unsigned map_int(int k) { return (unsigned)k ^ 0x80000000u; }
static unsigned map_float(float f) { const unsigned b = bits_of(f); return (b >> 31) ? ~b : b | 0x80000000u; }

// the stable order of n rows by the field [begin, end) of u[], complemented first if descending
static std::vector<int> order_of(const std::vector<unsigned> &u, bool descending, int begin, int end) {
    std::vector<int> order(u.size());
    for (size_t i = 0; i < u.size(); i++) order[i] = (int)i;
    const uint64_t mask = (1ull << (end - begin)) - 1;
    auto field = [&](int i) { return ((uint64_t)(descending ? ~u[i] : u[i]) >> begin) & mask; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return field(a) < field(b); });
    return order;
}

template <typename T>
static int rows_differ(const std::vector<T> &got, const std::vector<T> &in, const std::vector<int> &order) {
    int bad = 0;
    for (size_t i = 0; i < got.size(); i++) bad += memcmp(&got[i], &in[order[i]], sizeof(T)) != 0;
    return bad;
}

int main() {
    using namespace StreamCompaction;
    const int T = sc_records_tile_elements();
    int bad = 0;
    for (int n : {1, 65, T - 1, T, T + 1, 3 * T + 17}) {
        std::vector<Hit> hits(n), hits_got(n);
        std::vector<Seg> segs(n), segs_got(n);
        std::vector<int> perm_got(n);
        std::vector<unsigned> u(n);
        unsigned s = 4242u + (unsigned)n;
        for (int i = 0; i < n; i++) {
            s = s * 1664525u + 1013904223u;
            const float t = (s & 7u) == 0 ? -0.f : (s & 7u) == 1 ? 0.f : ((int)(s >> 8) - (1 << 23)) * 0.37f;
            hits[i] = Hit{t, (int)(s * 2654435761u), {1.f, 2.f, (float)(s & 255)}};
            segs[i] = Seg{{(float)i, 0.f, 1.f, 2.f}, {3.f, 4.f, 5.f, 6.f}, s ^ (s >> 7), i, {0, 0}};
        }
        Hit *d_hits, *d_hits_out;
        Seg *d_segs, *d_segs_out;
        int *d_perm;
        float *d_t_out;
        HIP_OK(hipMalloc(&d_hits, sizeof(Hit) * n)); HIP_OK(hipMalloc(&d_hits_out, sizeof(Hit) * n));
        HIP_OK(hipMalloc(&d_segs, sizeof(Seg) * n)); HIP_OK(hipMalloc(&d_segs_out, sizeof(Seg) * n));
        HIP_OK(hipMalloc(&d_perm, sizeof(int) * n)); HIP_OK(hipMalloc(&d_t_out, sizeof(float) * n));
        HIP_OK(hipMemcpy(d_hits, hits.data(), sizeof(Hit) * n, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_segs, segs.data(), sizeof(Seg) * n, hipMemcpyHostToDevice));

        // int keys inside the first array, two arrays, all bits, ascending: frame order restored by pixel index
        Records::radixSortByKey(n, 0, 0, 32, &d_hits->pixel, (int)sizeof(Hit), d_hits_out, d_hits, d_segs_out, d_segs);
        HIP_OK(hipMemcpy(hits_got.data(), d_hits_out, sizeof(Hit) * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(segs_got.data(), d_segs_out, sizeof(Seg) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) u[i] = map_int(hits[i].pixel);
        std::vector<int> order = order_of(u, false, 0, 32);
        bad += rows_differ(hits_got, hits, order) + rows_differ(segs_got, segs, order);

        // unsigned keys inside the second kind of record, one array, bits [10, 30) of a Morton code, descending, with the permutation
        Records::radixSortByKey(n, 1, 10, 30, &d_segs->morton, (int)sizeof(Seg), d_segs_out, d_segs, d_perm);
        HIP_OK(hipMemcpy(segs_got.data(), d_segs_out, sizeof(Seg) * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(perm_got.data(), d_perm, sizeof(int) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) u[i] = segs[i].morton;
        order = order_of(u, true, 10, 30);
        bad += rows_differ(segs_got, segs, order) + (memcmp(perm_got.data(), order.data(), sizeof(int) * n) != 0);

        // float keys (hit distance, front to back, -0 before +0), the segments alongside, the sorted keys returned
        Records::radixSortByKey(n, 0, 0, 32, &d_hits->t, (int)sizeof(Hit), d_hits_out, d_hits, d_segs_out, d_segs, d_perm, d_t_out);
        HIP_OK(hipMemcpy(hits_got.data(), d_hits_out, sizeof(Hit) * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(segs_got.data(), d_segs_out, sizeof(Seg) * n, hipMemcpyDeviceToHost));
        std::vector<float> t_got(n);
        HIP_OK(hipMemcpy(t_got.data(), d_t_out, sizeof(float) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) u[i] = map_float(hits[i].t);
        order = order_of(u, false, 0, 32);
        bad += rows_differ(hits_got, hits, order) + rows_differ(segs_got, segs, order);
        for (int i = 0; i < n; i++) bad += bits_of(t_got[i]) != bits_of(hits[order[i]].t);
        for (int i = 0; i + 1 < n; i++) bad += t_got[i] > t_got[i + 1];
        (void)hipFree(d_hits); (void)hipFree(d_hits_out); (void)hipFree(d_segs); (void)hipFree(d_segs_out); (void)hipFree(d_perm); (void)hipFree(d_t_out);
    }
    Records::release();
    printf("all: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
