// sketch_find.hip -- the way back from a sketch to the sequences: which k-mers of a buffer hash into a query sketch, and where.
//
// GPU counterpart of the reference's `sourmash sig kmers` loop (src/sourmash/sig/__main__.py:1087-1310: per record a sketch, an
// intersection and then a Python membership test per k-mer) for a whole buffer at once:
//   directory  the query's sorted hashes get a bucket directory over the top bits of the hash space (find_core.hpp), one lane per
//              bucket boundary;
//   find       the per-record kernel's walk (records_kernel.hpp) with a sink that filters where the staged pairs leave LDS
//              (find_kernel.hpp): only (hash, position) pairs whose hash is in the query reach HBM.  Membership is not in the
//              walk: there one lane of a wave keeps a hash now and then, and its dependent loads -- directory, then q -- would
//              hold up the other 63 lanes' arithmetic; at the flush all 256 lanes look up one staged pair each.
//   assign     one lane per matched pair: the record of the position and the rule that no k-mer spans two records
//              (records_core.hpp: rec_assign).  A pair the rule drops gets position UINT64_MAX.
//   sort       by position, the hash as payload (device_sort.hip: sort_pairs); the dropped pairs sort last.
//   offsets    one lane per record: the first row at or behind the record's start; n_out = rows below UINT64_MAX.
//   text       one lane per (row, byte): the k-mer as it stands in the buffer, upper-cased.
// Rows are therefore ordered by record, then position.  Nothing here reads a count back: the caller passes the number of pairs
// and reads the number of rows when it synchronises.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_api.hpp"
#include "find_core.hpp"
#include "find_kernel.hpp"
#include "records_core.hpp"

namespace smg {

namespace {

constexpr int FD_THREADS = 256;

unsigned fd_grid(uint64_t n) { return (unsigned)((n + FD_THREADS - 1) / FD_THREADS); }

// dir[b] for b = 0 .. nb
__global__ __launch_bounds__(FD_THREADS) void find_dir_kernel(const uint64_t* __restrict__ q, uint64_t n, uint32_t shift, uint64_t nb,
                                                              uint32_t* __restrict__ dir) {
    const uint64_t b = (uint64_t)blockIdx.x * FD_THREADS + threadIdx.x;
    if (b > nb) return;
    dir[b] = find_dir_entry(q, n, shift, b);
}

// pos[i] stays where the k-mer lies inside a record, and becomes UINT64_MAX where rec_assign drops it
__global__ __launch_bounds__(FD_THREADS) void find_assign_kernel(uint64_t* __restrict__ pos, uint64_t n, const uint64_t* __restrict__ starts,
                                                                 uint64_t n_records, uint32_t k) {
    const uint64_t i = (uint64_t)blockIdx.x * FD_THREADS + threadIdx.x;
    if (i >= n) return;
    uint64_t r = 0;
    if (!rec_assign(starts, n_records, pos[i], k, &r)) pos[i] = ~0ull;
}

// first index of the ascending pos[0, n) that is >= v
__device__ __forceinline__ uint64_t fd_lower_bound(const uint64_t* pos, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (pos[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// offsets[r] = first row at or behind starts[r], for r = 0 .. n_records, never above n_out; *n_out = rows below UINT64_MAX
__global__ __launch_bounds__(FD_THREADS) void find_offsets_kernel(const uint64_t* __restrict__ pos, uint64_t n, const uint64_t* __restrict__ starts,
                                                                  uint64_t n_records, uint64_t* __restrict__ offsets, uint64_t* __restrict__ n_out) {
    const uint64_t r = (uint64_t)blockIdx.x * FD_THREADS + threadIdx.x;
    if (r > n_records) return;
    const uint64_t rows = fd_lower_bound(pos, n, ~0ull);
    if (r == 0) *n_out = rows;
    const uint64_t at = fd_lower_bound(pos, n, starts[r]);
    offsets[r] = at < rows ? at : rows;
}

// kmers[row * k + j] = upper(seq[pos[row] + j]) for the rows below *n_rows
__global__ __launch_bounds__(FD_THREADS) void find_text_kernel(const uint8_t* __restrict__ seq, uint64_t len, const uint64_t* __restrict__ pos,
                                                               const uint64_t* __restrict__ n_rows, uint64_t n, uint32_t k,
                                                               uint8_t* __restrict__ kmers) {
    const uint64_t i = (uint64_t)blockIdx.x * FD_THREADS + threadIdx.x;
    const uint64_t rows = *n_rows < n ? *n_rows : n;
    if (i >= rows * k) return;
    const uint64_t row = i / k, j = i - row * k;
    const uint64_t at = pos[row] + j;
    kmers[i] = at < len ? (uint8_t)(seq[at] & 0xdfu) : (uint8_t)0;      // the bytes of a reported k-mer are all in ACGTacgt
}

}  // namespace

hipError_t find_dir_launch(const uint64_t* d_q, uint64_t n, uint32_t shift, uint64_t n_buckets, uint32_t* d_dir, hipStream_t stream) {
    if (n > FIND_MAX_QUERY || n_buckets > FIND_MAX_BUCKETS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(find_dir_kernel, dim3(fd_grid(n_buckets + 1)), dim3(FD_THREADS), 0, stream, d_q, n, shift, n_buckets, d_dir);
    return hipGetLastError();
}

hipError_t find_pairs_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, uint64_t seed, const FindQuery& query, uint64_t* d_hash,
                             uint64_t* d_pos, unsigned long long* d_count, uint64_t cap, uint32_t grid, hipStream_t stream) {
    if (k == 0 || k > (uint32_t)SK_FAST_MAX_K || query.max_hash == 0 || grid > (1u << 20)) return hipErrorInvalidValue;
    if (len < k) return hipSuccess;
    return launcher<FindLaunch>(k)(d_seq, len, seed, query, d_hash, d_pos, d_count, cap, grid, stream);
}

size_t find_rows_temp_bytes(uint64_t n_pairs) { return al256(sort_pairs_temp_bytes(n_pairs ? n_pairs : 1)) + 256; }

hipError_t find_rows_launch(const uint8_t* d_seq, uint64_t len, uint64_t* d_pair_hash, uint64_t* d_pair_pos, uint64_t n_pairs,
                            const uint64_t* d_starts, uint64_t n_records, uint32_t k, uint64_t* d_positions, uint64_t* d_hashes,
                            uint8_t* d_kmers, uint64_t* d_offsets, uint64_t* d_n_out, void* d_temp, size_t temp_bytes, hipStream_t stream) {
    if (n_pairs == 0 || n_records == 0) {
        hipError_t e = hipMemsetAsync(d_offsets, 0, (n_records + 1) * 8, stream);
        return e != hipSuccess ? e : hipMemsetAsync(d_n_out, 0, 8, stream);
    }
    if (n_pairs > 0xffffffffull || n_records > 0xffffffffull) return hipErrorInvalidValue;
    if (temp_bytes < find_rows_temp_bytes(n_pairs)) return hipErrorInvalidValue;
    hipError_t e;
    hipLaunchKernelGGL(find_assign_kernel, dim3(fd_grid(n_pairs)), dim3(FD_THREADS), 0, stream, d_pair_pos, n_pairs, d_starts, n_records, k);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = sort_pairs(d_pair_pos, d_positions, d_pair_hash, d_hashes, n_pairs, 64, d_temp, temp_bytes, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(find_offsets_kernel, dim3(fd_grid(n_records + 1)), dim3(FD_THREADS), 0, stream, (const uint64_t*)d_positions, n_pairs,
                       d_starts, n_records, d_offsets, d_n_out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (d_kmers) {
        hipLaunchKernelGGL(find_text_kernel, dim3(fd_grid(n_pairs * k)), dim3(FD_THREADS), 0, stream, d_seq, len, (const uint64_t*)d_positions,
                           (const uint64_t*)d_n_out, n_pairs, k, d_kmers);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace smg
