// sc_records_check.cpp -- StreamCompaction::Records (mygpuraytracer_amd/csrc/stream_compaction_api.h) as a caller with kernels of their
// own would use it: device arrays of a struct of their own, the key and the flag read out of the records, against std::stable_sort /
// std::stable_partition on the host.  Built with hipcc and run by the GPU tier (tests/test_gpu_sc_records.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mygpuraytracer_amd/csrc/stream_compaction_api.h"

struct Hit { float t; int material; float n[3]; };            // 20 bytes: the dword path
struct Seg { float o[4], d[4]; int pixel, live, pad[2]; };    // 48 bytes: the 16-byte path

#define HIP_OK(expr) do { if ((expr) != hipSuccess) { printf("%s failed\n", #expr); return 1; } } while (0)

int main() {
    using namespace StreamCompaction;
    const int T = sc_records_tile_elements(), materials = 7;
    int bad = 0;
    for (int n : {1, 65, T - 1, T, T + 1, 3 * T + 5}) {
        std::vector<Hit> hits(n), hits_got(n);
        std::vector<Seg> segs(n), segs_got(n);
        unsigned s = 99u + (unsigned)n;
        for (int i = 0; i < n; i++) {
            s = s * 1664525u + 1013904223u;
            hits[i] = Hit{(float)i, (int)((s >> 20) % materials), {1.f, 2.f, (float)(s & 255)}};
            segs[i] = Seg{{(float)i, 0.f, 1.f, 2.f}, {3.f, 4.f, 5.f, 6.f}, i, (s >> 28) < 7 ? (int)(s >> 28) + 1 : 0, {0, 0}};
        }
        Hit *d_hits, *d_hits_out;
        Seg *d_segs, *d_segs_out;
        HIP_OK(hipMalloc(&d_hits, sizeof(Hit) * n)); HIP_OK(hipMalloc(&d_hits_out, sizeof(Hit) * n));
        HIP_OK(hipMalloc(&d_segs, sizeof(Seg) * n)); HIP_OK(hipMalloc(&d_segs_out, sizeof(Seg) * n));
        HIP_OK(hipMemcpy(d_hits, hits.data(), sizeof(Hit) * n, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_segs, segs.data(), sizeof(Seg) * n, hipMemcpyHostToDevice));

        // thrust::sort_by_key(hits, hits + n, segs, sortByMaterial()): material descending, stable, the segments permuted alike
        Records::sortByKey(n, materials, 1, &d_hits->material, (int)sizeof(Hit), d_hits_out, d_hits, d_segs_out, d_segs);
        HIP_OK(hipMemcpy(hits_got.data(), d_hits_out, sizeof(Hit) * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(segs_got.data(), d_segs_out, sizeof(Seg) * n, hipMemcpyDeviceToHost));
        std::vector<int> order(n);
        for (int i = 0; i < n; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hits[a].material > hits[b].material; });
        for (int i = 0; i < n; i++)
            bad += memcmp(&hits_got[i], &hits[order[i]], sizeof(Hit)) != 0 || memcmp(&segs_got[i], &segs[order[i]], sizeof(Seg)) != 0;
        // one array alone, ascending
        Records::sortByKey(n, materials, 0, &d_hits->material, (int)sizeof(Hit), d_hits_out, d_hits);
        HIP_OK(hipMemcpy(hits_got.data(), d_hits_out, sizeof(Hit) * n, hipMemcpyDeviceToHost));
        std::vector<Hit> hits_want = hits;
        std::stable_sort(hits_want.begin(), hits_want.end(), [](const Hit &a, const Hit &b) { return a.material < b.material; });
        bad += memcmp(hits_got.data(), hits_want.data(), sizeof(Hit) * n) != 0;

        // thrust::stable_partition(segs, segs + n, isTerminate())
        std::vector<Seg> want = segs;
        const int live_want = (int)(std::stable_partition(want.begin(), want.end(), [](const Seg &p) { return p.live != 0; }) - want.begin());
        const int live = Records::stablePartition(n, d_segs_out, d_segs, &d_segs->live, (int)sizeof(Seg));
        HIP_OK(hipMemcpy(segs_got.data(), d_segs_out, sizeof(Seg) * n, hipMemcpyDeviceToHost));
        bad += live != live_want || memcmp(segs_got.data(), want.data(), sizeof(Seg) * n) != 0;
        // the kept ones alone: what lies behind them stays
        HIP_OK(hipMemset(d_segs_out, 0x5a, sizeof(Seg) * n));
        const int kept = Records::compact(n, d_segs_out, d_segs, &d_segs->live, (int)sizeof(Seg));
        HIP_OK(hipMemcpy(segs_got.data(), d_segs_out, sizeof(Seg) * n, hipMemcpyDeviceToHost));
        bad += kept != live_want || memcmp(segs_got.data(), want.data(), sizeof(Seg) * kept) != 0;
        const unsigned char *tail = reinterpret_cast<const unsigned char *>(segs_got.data() + kept);
        for (size_t i = 0; i < sizeof(Seg) * (size_t)(n - kept); i++) bad += tail[i] != 0x5a;
        (void)hipFree(d_hits); (void)hipFree(d_hits_out); (void)hipFree(d_segs); (void)hipFree(d_segs_out);
    }
    Records::release();
    Records::release();                                        // (nothing left to free: harmless)
    printf("all: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
