/* mi355x_stream_compaction.h -- C ABI of the scan / stream-compaction library (part of libmi355x_pathtracer.so).
 *
 * Drop-in for the reference's stream_compaction/ library (file:line relative to the reference root):
 *
 *   StreamCompaction::CPU::scan                 stream_compaction/cpu.cu:20      sc_cpu_scan
 *   StreamCompaction::CPU::compactWithoutScan   stream_compaction/cpu.cu:39      sc_cpu_compact_without_scan
 *   StreamCompaction::CPU::compactWithScan      stream_compaction/cpu.cu:58      sc_cpu_compact_with_scan
 *   StreamCompaction::Naive::scan               stream_compaction/naive.cu:34    sc_naive_scan
 *   StreamCompaction::Efficient::scan           stream_compaction/efficient.cu:36 sc_efficient_scan
 *   StreamCompaction::Efficient::compact        stream_compaction/efficient.cu:79 sc_efficient_compact
 *   StreamCompaction::Thrust::scan              stream_compaction/thrust.cu:20   sc_thrust_scan
 *   StreamCompaction::Common::kernMapToBoolean  stream_compaction/common.cu:25   sc_map_to_boolean_device
 *   StreamCompaction::Common::kernScatter       stream_compaction/common.cu:40   sc_scatter_device
 *   <ns>::timer().getGpu/CpuElapsedTimeForPreviousOperation  common.h:48-132     sc_last_gpu_ms / sc_last_cpu_ms
 *   thrust::sort_by_key(.., sortByMaterial())   src/pathtrace.cu:418-422,518     sc_sort_records_by_key_device
 *   thrust::stable_partition(.., isTerminate()) src/pathtrace.cu:424-428,541     sc_partition_records_device
 *   (the kept half of that partition alone)                                      sc_compact_records_device
 *   thrust::sort_by_key(keys, keys + n, values)  with keys of any value          sc_radix_sort_records_device
 *
 * Same argument meaning as the reference: n elements, host pointers in and out (the GPU variants allocate and
 * copy internally, exactly like the reference's), exclusive prefix sum, compaction keeps non-zero elements in
 * order and returns their count.  The three GPU scan entry points are one implementation here (a single-pass chained
 * scan with decoupled look-back written for wave64; the reference's O(log n)-launch Naive and Blelloch variants are
 * teaching steps, not something to preserve) and give identical results.  The *_device forms take device
 * pointers and a hipStream_t and do no allocation or copy: that is what a production caller wants.
 * GPU entry points return 0 on success, non-zero (PTX_ERR_*) on failure with the message in ptx_last_error().
 */
#ifndef MI355X_STREAM_COMPACTION_H
#define MI355X_STREAM_COMPACTION_H

#ifdef __cplusplus
extern "C" {
#endif

void sc_cpu_scan(int n, int *odata, const int *idata);
int sc_cpu_compact_without_scan(int n, int *odata, const int *idata);
int sc_cpu_compact_with_scan(int n, int *odata, const int *idata);

int sc_naive_scan(int n, int *odata, const int *idata);
int sc_efficient_scan(int n, int *odata, const int *idata);
int sc_thrust_scan(int n, int *odata, const int *idata);
/* returns the number of elements kept, or -1 on failure */
int sc_efficient_compact(int n, int *odata, const int *idata);

/* device-pointer forms; workspace: sc_scan_workspace_bytes(n) bytes of device memory, 8-byte aligned, contents arbitrary;
 * the scan may run in place (d_odata == d_idata), the compaction may not */
unsigned long long sc_scan_workspace_bytes(int n);
int sc_scan_device(int n, int *d_odata, const int *d_idata, void *d_workspace, void *stream);
int sc_compact_device(int n, int *d_odata, const int *d_idata, int *d_count, void *d_workspace, void *stream);

/* the two building-block kernels of the reference's own compaction (common.h:38-41), on device arrays of n ints:
 * bools[i] = idata[i] != 0 ? 1 : 0;   and   bools[i] == 1  =>  odata[indices[i]] = idata[i].   Enqueued on `stream`, no sync. */
int sc_map_to_boolean_device(int n, int *d_bools, const int *d_idata, void *stream);
int sc_scatter_device(int n, int *d_odata, const int *d_idata, const int *d_bools, const int *d_indices, void *stream);

/* ---- records: what the reference's per-bounce loop asks of thrust, on records instead of ints ------------------------------
 * A stable counting sort of n records by a small integer key.  The key of element i is the int at d_keys + i * key_stride_bytes,
 * so it can be read straight out of a record array (materialId inside ShadeableIntersection: d_keys = records + 16, stride 32).
 * A key outside [0, nkeys) is CLAMPED into the range before it is used (a negative one counts as 0, a large one as nkeys - 1): a
 * bad key gives a defined order and never an address.  descending != 0 maps key k to nkeys - 1 - k; equal keys keep input order
 * either way.  Up to two record arrays are permuted alike (b: NULL, NULL, 0 = one array); d_perm, if given, receives the source
 * index of every output slot, d_key_totals the number of elements per (mapped) key.
 * Limits: 1 <= nkeys <= 256; record_bytes a multiple of 4 in 4..256; key / flag stride a multiple of 4, >= 4; all pointers 4-byte
 * aligned (records whose size is a multiple of 16 move as 16-byte accesses when both their pointers are 16-byte aligned); every
 * output differs from, and does not overlap, every input and the keys: there is no in-place form.  Anything else returns
 * PTX_ERR_INVALID with the offending value in ptx_last_error() and enqueues nothing; these checks come before the device check
 * (PTX_ERR_NODEVICE).  Workspace: sc_records_workspace_bytes(n, nkeys) bytes of device memory, 8-byte aligned, contents arbitrary,
 * reusable by later calls of any size it is large enough for (the size grows with n and with nkeys) and by sc_scan_device /
 * sc_compact_device.  No allocation, no host synchronisation, no copy: three kernels and one memset on `stream`.  The result is
 * the same on every run.  n == 0 writes zero totals / *d_count = 0 and nothing else. */
int sc_records_tile_elements(void);                                    /* elements one workgroup ranks (tests sit on its edges) */
unsigned long long sc_records_workspace_bytes(int n, int nkeys);       /* 0 for arguments outside the limits */

/* thrust::sort_by_key(dev_intersections, dev_intersections + num_paths, dev_paths, sortByMaterial())  src/pathtrace.cu:418-422,518:
 * nkeys = number of materials, descending = 1 */
int sc_sort_records_by_key_device(int n, int nkeys, int descending,
        const void *d_keys, int key_stride_bytes,
        void *d_out_a, const void *d_in_a, int record_bytes_a,
        void *d_out_b, const void *d_in_b, int record_bytes_b,
        int *d_perm, int *d_key_totals,
        void *d_workspace, void *stream);

/* thrust::stable_partition(dev_paths, dev_paths + num_paths, isTerminate())  src/pathtrace.cu:424-428,541: the records whose flag
 * (the int at d_flags + i * flag_stride_bytes; remainingBounces: d_flags = paths + 40, stride 44) is != 0 first, then those with
 * flag == 0, both in input order; *d_count = the partition point */
int sc_partition_records_device(int n, int record_bytes, void *d_out, const void *d_in,
        const void *d_flags, int flag_stride_bytes, int *d_count, void *d_workspace, void *stream);

/* the kept records only: nothing is written at or after d_out + count * record_bytes */
int sc_compact_records_device(int n, int record_bytes, void *d_out, const void *d_in,
        const void *d_flags, int flag_stride_bytes, int *d_count, void *d_workspace, void *stream);

/* host-pointer forms of the three (allocate, copy and synchronise internally, like sc_efficient_compact); keys / flags: n ints.
 * perm and key_totals may be NULL; count may not.  sc_compact_records writes *count records to out. */
int sc_sort_records_by_key(int n, int nkeys, int descending, const int *keys,
        void *out_a, const void *in_a, int record_bytes_a, void *out_b, const void *in_b, int record_bytes_b,
        int *perm, int *key_totals);
int sc_partition_records(int n, int record_bytes, void *out, const void *in, const int *flags, int *count);
int sc_compact_records(int n, int record_bytes, void *out, const void *in, const int *flags, int *count);

/* ---- records by full 32-bit keys: thrust::sort_by_key for keys of ANY value ---------------------------------------------------
 * A stable least-significant-digit radix sort of n records, 8 bits per pass.  The 32 key bits of element i are read at
 * d_keys + i * key_stride_bytes (a field of a record serves, as above) and mapped to an unsigned u whose order is the key type's:
 *     SC_KEY_INT32    u = bits ^ 0x80000000
 *     SC_KEY_UINT32   u = bits
 *     SC_KEY_FLOAT32  u = (bits >> 31) ? ~bits : bits | 0x80000000
 * and, with descending != 0, complemented afterwards.  sc_radix_map_key is that map (host code, no device).  The float order is total:
 * negative NaNs < -inf < ... < -0 < +0 < ... < +inf < positive NaNs, NaNs by payload -- a NaN key gives a defined order and never an
 * address.  The result is the stable sort by the field (u >> begin_bit) & (2^(end_bit - begin_bit) - 1), 0 <= begin_bit <= end_bit <= 32:
 * equal fields keep input order, ascending or descending; begin_bit == end_bit copies the input.  ceil((end_bit - begin_bit) / 8)
 * passes move (u, source index) pairs inside the workspace; the records themselves move once, in a gather behind the last pass.
 * d_perm[p], if given, receives the source index of output row p; d_keys_out[p], if given, the caller's original 32 key bits of
 * that row (what thrust::sort_by_key leaves in the key array).
 * Limits, refusals and side effects are sc_sort_records_by_key_device's: record_bytes a multiple of 4 in 4..256, stride a multiple of
 * 4 and >= 4, 4-byte aligned pointers (16-byte moves where the size and both pointers allow), no output equal to or overlapping an
 * input, the keys or another output; anything else returns PTX_ERR_INVALID with the offending value in ptx_last_error(), enqueues
 * nothing and is checked before the device (PTX_ERR_NODEVICE).  Workspace: sc_radix_workspace_bytes(n) bytes of device memory (about
 * 16 n), 8-byte aligned, contents arbitrary, reusable by any later call of the library it is large enough for.  No allocation, no
 * host synchronisation, no copy; the same bytes on every run; n == 0 writes nothing. */
enum { SC_KEY_INT32 = 0, SC_KEY_UINT32 = 1, SC_KEY_FLOAT32 = 2 };

unsigned long long sc_radix_workspace_bytes(int n);                    /* 0 for n < 0 */
unsigned int sc_radix_map_key(int key_type, int descending, unsigned int bits);

int sc_radix_sort_records_device(int n, int key_type, int descending, int begin_bit, int end_bit,
        const void *d_keys, int key_stride_bytes,
        void *d_out_a, const void *d_in_a, int record_bytes_a,
        void *d_out_b, const void *d_in_b, int record_bytes_b,         /* NULL, NULL, 0 = one array */
        int *d_perm, void *d_keys_out,                                  /* both optional */
        void *d_workspace, void *stream);

/* host pointers (keys: n 32-bit words); allocates, copies, synchronises and sets sc_last_gpu_ms; perm and keys_out may be NULL */
int sc_radix_sort_records(int n, int key_type, int descending, int begin_bit, int end_bit, const void *keys,
        void *out_a, const void *in_a, int record_bytes_a, void *out_b, const void *in_b, int record_bytes_b,
        int *perm, void *keys_out);

float sc_last_gpu_ms(void);      /* device time of the kernels of the previous GPU call (hipEvent), ms */
float sc_last_cpu_ms(void);      /* wall time of the previous sc_cpu_* call, ms */

int sc_ilog2(int x);             /* common.h:21-27 */
int sc_ilog2ceil(int x);         /* common.h:29-31 */

#ifdef __cplusplus
}
#endif
#endif
