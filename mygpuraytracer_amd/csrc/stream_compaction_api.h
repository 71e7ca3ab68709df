// stream_compaction_api.h -- C++ veneer with the reference's own names over the C ABI of the scan / compaction library
// (include/mi355x_stream_compaction.h).  Header-only.
//
// A user of the reference's stream_compaction/ library replaces
//     #include <stream_compaction/cpu.h> <stream_compaction/naive.h> <stream_compaction/efficient.h> <stream_compaction/thrust.h>
// by this header and links libmi355x_pathtracer.so; calls such as
//     StreamCompaction::Efficient::scan(n, odata, idata);                                  // efficient.h:9
//     int kept = StreamCompaction::Efficient::compact(n, odata, idata);                    // efficient.h:11
//     float ms = StreamCompaction::Efficient::timer().getGpuElapsedTimeForPreviousOperation();
//     StreamCompaction::CPU::compactWithoutScan(n, odata, idata);                          // cpu.h:11
// compile and mean what they meant: host pointers in and out, exclusive prefix sums, non-zero elements kept in order, one
// timer per namespace holding the time of that namespace's previous operation (common.h:48-132).  A failing GPU call
// prints and exits like checkCUDAError (common.h:17-20, common.cu:3-17); use the C ABI for return codes.
// Common::kernMapToBoolean / kernScatter (common.h:38-41) are __global__ kernels in the reference, launched by its own
// compaction with <<<grid, block>>>; here they are ordinary functions on device pointers that enqueue the whole array on a
// stream (default: the null stream), because this header must also compile in translation units without HIP:
//     StreamCompaction::Common::kernMapToBoolean(n, dev_bools, dev_idata);              // was <<<blocks, 128>>>(n, ...)
// StreamCompaction::Records is what the reference's path tracer asks of thrust per bounce (src/pathtrace.cu:518,541), on DEVICE pointers:
//     Records::sortByKey(num_paths, nmaterials, 1, &dev_isects->materialId, sizeof(ShadeableIntersection), out_isects, dev_isects,
//                        out_paths, dev_paths);                                           // was thrust::sort_by_key(.., sortByMaterial())
//     int live = Records::stablePartition(num_paths, out_paths, dev_paths, &dev_paths->remainingBounces, sizeof(PathSegment));
// and, for keys of any value (int, unsigned or float; pixel index, Morton code, hit distance), thrust::sort_by_key proper:
//     Records::radixSortByKey(num_paths, 0, 0, 32, &dev_paths->pixelIndex, sizeof(PathSegment), out_paths, dev_paths);
// It allocates its workspace with hipMalloc, so it exists only in translation units compiled for HIP (hipcc, or
// -D__HIP_PLATFORM_AMD__ with the HIP headers on the include path).
// Not carried over: startGpuTimer/endGpuTimer and their CPU twins (the library times its operations itself).
#pragma once
#include <cstdio>
#include <cstdlib>
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
#include <hip/hip_runtime_api.h>
#include <type_traits>
#endif

#include "../../include/mi355x_pathtracer.h"
#include "../../include/mi355x_stream_compaction.h"

inline int ilog2(int x) { return sc_ilog2(x); }              // common.h:21-27
inline int ilog2ceil(int x) { return sc_ilog2ceil(x); }      // common.h:29-31

namespace StreamCompaction {
namespace Common {

class PerformanceTimer {                                     // common.h:48-132, the two getters
public:
    float getCpuElapsedTimeForPreviousOperation() { return cpu_ms_; }
    float getGpuElapsedTimeForPreviousOperation() { return gpu_ms_; }
    PerformanceTimer() = default;
    PerformanceTimer(const PerformanceTimer &) = delete;
    PerformanceTimer &operator=(const PerformanceTimer &) = delete;
    void mi355x_set(float cpu_ms, float gpu_ms) { if (cpu_ms >= 0.f) cpu_ms_ = cpu_ms; if (gpu_ms >= 0.f) gpu_ms_ = gpu_ms; }
private:
    float cpu_ms_ = 0.f, gpu_ms_ = 0.f;
};

inline void mi355x_check(int rc, const char *what) {
    if (rc == 0) return;
    fprintf(stderr, "mi355x stream compaction error (%s): %s\n", what, ptx_last_error());
    exit(EXIT_FAILURE);
}

// common.h:38-41, common.cu:25-49 -- device pointers; the launch configuration is the library's business
inline void kernMapToBoolean(int n, int *bools, const int *idata, void *stream = nullptr) {
    mi355x_check(sc_map_to_boolean_device(n, bools, idata, stream), "Common::kernMapToBoolean");
}
inline void kernScatter(int n, int *odata, const int *idata, const int *bools, const int *indices, void *stream = nullptr) {
    mi355x_check(sc_scatter_device(n, odata, idata, bools, indices, stream), "Common::kernScatter");
}

}  // namespace Common

namespace CPU {                                              // cpu.h:5-15
inline Common::PerformanceTimer &timer() { static Common::PerformanceTimer t; return t; }
inline void scan(int n, int *odata, const int *idata) { sc_cpu_scan(n, odata, idata); timer().mi355x_set(sc_last_cpu_ms(), -1.f); }
inline int compactWithoutScan(int n, int *odata, const int *idata) {
    const int k = sc_cpu_compact_without_scan(n, odata, idata);
    timer().mi355x_set(sc_last_cpu_ms(), -1.f);
    return k;
}
inline int compactWithScan(int n, int *odata, const int *idata) {
    const int k = sc_cpu_compact_with_scan(n, odata, idata);
    timer().mi355x_set(sc_last_cpu_ms(), -1.f);
    return k;
}
}  // namespace CPU

namespace Naive {                                            // naive.h:5-9
inline Common::PerformanceTimer &timer() { static Common::PerformanceTimer t; return t; }
inline void scan(int n, int *odata, const int *idata) {
    Common::mi355x_check(sc_naive_scan(n, odata, idata), "Naive::scan");
    timer().mi355x_set(-1.f, sc_last_gpu_ms());
}
}  // namespace Naive

namespace Efficient {                                        // efficient.h:5-13
inline Common::PerformanceTimer &timer() { static Common::PerformanceTimer t; return t; }
inline void scan(int n, int *odata, const int *idata) {
    Common::mi355x_check(sc_efficient_scan(n, odata, idata), "Efficient::scan");
    timer().mi355x_set(-1.f, sc_last_gpu_ms());
}
inline int compact(int n, int *odata, const int *idata) {
    const int k = sc_efficient_compact(n, odata, idata);
    Common::mi355x_check(k < 0 ? 1 : 0, "Efficient::compact");
    timer().mi355x_set(-1.f, sc_last_gpu_ms());
    return k;
}
}  // namespace Efficient

namespace Thrust {                                           // thrust.h:5-9
inline Common::PerformanceTimer &timer() { static Common::PerformanceTimer t; return t; }
inline void scan(int n, int *odata, const int *idata) {
    Common::mi355x_check(sc_thrust_scan(n, odata, idata), "Thrust::scan");
    timer().mi355x_set(-1.f, sc_last_gpu_ms());
}
}  // namespace Thrust

#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
namespace Records {                                          // thrust::sort_by_key / stable_partition of src/pathtrace.cu:418-428,518,541
// the workspace every call borrows: grown on demand (after a device synchronisation: an earlier call may still be using the old
// one), freed by release()
inline void *mi355x_workspace(unsigned long long bytes, bool free_it = false) {
    static void *ws = nullptr;
    static unsigned long long have = 0;
    if (free_it || bytes > have) {
        if (ws) { (void)hipDeviceSynchronize(); (void)hipFree(ws); }
        ws = nullptr; have = 0;
        if (!free_it) {
            if (hipMalloc(&ws, bytes) != hipSuccess) { fprintf(stderr, "mi355x stream compaction error (Records): hipMalloc of %llu bytes failed\n", bytes); exit(EXIT_FAILURE); }
            have = bytes;
        }
    }
    return ws;
}
inline void release() { mi355x_workspace(0, true); }

// the workspace of one call, with 8 bytes behind it for the count that stablePartition / compact read back
inline void *mi355x_borrow(int n, int nkeys, int **count) {
    const unsigned long long need = sc_records_workspace_bytes(n, nkeys);
    char *ws = static_cast<char *>(mi355x_workspace(need + 8));
    *count = reinterpret_cast<int *>(ws + need);
    return ws;
}

template <typename T>
inline void sortByKey(int n, int nkeys, int descending, const int *firstKey, int keyStride, T *outA, const T *inA, void *stream = nullptr) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "records are trivially copyable, a multiple of 4 bytes");
    int *count;
    void *ws = mi355x_borrow(n, nkeys, &count);
    Common::mi355x_check(sc_sort_records_by_key_device(n, nkeys, descending, firstKey, keyStride, outA, inA, (int)sizeof(T), nullptr, nullptr, 0,
                                                       nullptr, nullptr, ws, stream), "Records::sortByKey");
}
template <typename T, typename U>
inline void sortByKey(int n, int nkeys, int descending, const int *firstKey, int keyStride, T *outA, const T *inA, U *outB, const U *inB,
                      void *stream = nullptr) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "records are trivially copyable, a multiple of 4 bytes");
    static_assert(std::is_trivially_copyable<U>::value && sizeof(U) % 4 == 0, "records are trivially copyable, a multiple of 4 bytes");
    int *count;
    void *ws = mi355x_borrow(n, nkeys, &count);
    Common::mi355x_check(sc_sort_records_by_key_device(n, nkeys, descending, firstKey, keyStride, outA, inA, (int)sizeof(T), outB, inB, (int)sizeof(U),
                                                       nullptr, nullptr, ws, stream), "Records::sortByKey");
}

// thrust::sort_by_key for keys of any value: K = int, unsigned or float, bits [beginBit, endBit) of the key's order-preserving map
// (include/mi355x_stream_compaction.h), ascending or descending, stable.  perm (source index per output row) and keysOut (the keys in
// output order) are optional device arrays of n.
template <typename K> struct mi355x_key_type;
template <> struct mi355x_key_type<int> { static constexpr int value = SC_KEY_INT32; };
template <> struct mi355x_key_type<unsigned> { static constexpr int value = SC_KEY_UINT32; };
template <> struct mi355x_key_type<float> { static constexpr int value = SC_KEY_FLOAT32; };

template <typename K, typename T>
inline void radixSortByKey(int n, int descending, int beginBit, int endBit, const K *firstKey, int keyStride, T *outA, const T *inA,
                           int *perm = nullptr, K *keysOut = nullptr, void *stream = nullptr) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "records are trivially copyable, a multiple of 4 bytes");
    void *ws = mi355x_workspace(sc_radix_workspace_bytes(n));
    Common::mi355x_check(sc_radix_sort_records_device(n, mi355x_key_type<K>::value, descending, beginBit, endBit, firstKey, keyStride, outA, inA, (int)sizeof(T),
                                                      nullptr, nullptr, 0, perm, keysOut, ws, stream), "Records::radixSortByKey");
}
template <typename K, typename T, typename U>
inline void radixSortByKey(int n, int descending, int beginBit, int endBit, const K *firstKey, int keyStride, T *outA, const T *inA, U *outB, const U *inB,
                           int *perm = nullptr, K *keysOut = nullptr, void *stream = nullptr) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "records are trivially copyable, a multiple of 4 bytes");
    static_assert(std::is_trivially_copyable<U>::value && sizeof(U) % 4 == 0, "records are trivially copyable, a multiple of 4 bytes");
    void *ws = mi355x_workspace(sc_radix_workspace_bytes(n));
    Common::mi355x_check(sc_radix_sort_records_device(n, mi355x_key_type<K>::value, descending, beginBit, endBit, firstKey, keyStride, outA, inA, (int)sizeof(T),
                                                      outB, inB, (int)sizeof(U), perm, keysOut, ws, stream), "Records::radixSortByKey");
}

template <typename T>
inline int mi355x_split(bool keptOnly, int n, T *out, const T *in, const int *firstFlag, int flagStride, void *stream) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "records are trivially copyable, a multiple of 4 bytes");
    int *count, kept = 0;
    void *ws = mi355x_borrow(n, 2, &count);
    Common::mi355x_check((keptOnly ? sc_compact_records_device : sc_partition_records_device)(n, (int)sizeof(T), out, in, firstFlag, flagStride, count, ws, stream),
                         keptOnly ? "Records::compact" : "Records::stablePartition");
    // one synchronising read, as thrust's return value is
    if (hipMemcpyAsync(&kept, count, sizeof(int), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)) != hipSuccess ||
        hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) {
        fprintf(stderr, "mi355x stream compaction error (Records): reading the count failed\n");
        exit(EXIT_FAILURE);
    }
    return kept;
}
// flag != 0 first, then flag == 0, both in order; returns the partition point
template <typename T>
inline int stablePartition(int n, T *out, const T *in, const int *firstFlag, int flagStride, void *stream = nullptr) {
    return mi355x_split(false, n, out, in, firstFlag, flagStride, stream);
}
// the kept records only; returns their number
template <typename T>
inline int compact(int n, T *out, const T *in, const int *firstFlag, int flagStride, void *stream = nullptr) {
    return mi355x_split(true, n, out, in, firstFlag, flagStride, stream);
}
}  // namespace Records
#endif
}  // namespace StreamCompaction
