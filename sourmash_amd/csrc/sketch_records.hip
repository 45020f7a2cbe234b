// sketch_records.hip -- every record of a buffer into its own sketch in one pass: sequence in HBM -> one CSR row per record.
//
// GPU counterpart of the reference's singleton loop (src/sourmash/command_sketch.py:712-739: one signature per record, one
// add_sequence each) for a whole buffer at once, without a launch, a sort or a host object per record:
//   pairs     the sketch kernel's walk with a (hash, position) sink (records_kernel.hpp): every kept hash together with the
//             start of its k-mer in the caller's buffer.  The hot kernel knows nothing about records.
//   assign    one lane per pair: the record of the position (binary search in the caller's ascending starts) and the rule
//             that no k-mer spans two records (records_core.hpp: rec_assign; rec_assign_ends for records with explicit ends,
//             which the residue passes of protein_records.hip use).  A pair the rule drops gets key 0, which no kept
//             pair has (hashes are >= 1).
//   sort      by (record, hash).  Packed form: the record number in the key bits above the hash, the library's 64-bit sort +
//             run-length encode (device_sort.hip: sort_unique); wide form, when record and hash bits exceed 64: two stable radix
//             passes over (hash, record) pairs -- hash, then record -- and a run-length encode over the pair.  The run lengths
//             are the abundances.
//   finish    the dropped pairs' run (key 0 sorts first) is skipped, hashes / abundances go to the caller's arrays;
//   offsets   one lane per record: a binary search for the record's first entry.
// Nothing here reads a count back: the caller passes the number of pairs (an upper bound of every later size) and reads the
// number of entries when it synchronises.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_api.hpp"
#include "records_core.hpp"
#include "records_kernel.hpp"

namespace smg {

namespace {

constexpr int RC_THREADS = 256;

unsigned rc_grid(uint64_t n) { return (unsigned)((n + RC_THREADS - 1) / RC_THREADS); }

// *bad |= 1: starts not ascending; |= 2: starts[n_records] > len
__global__ __launch_bounds__(RC_THREADS) void rec_check_starts_kernel(const uint64_t* __restrict__ starts, uint64_t n_records, uint64_t len,
                                                                      unsigned long long* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i < n_records && starts[i] > starts[i + 1]) atomicOr(bad, 1ull);
    if (i == n_records && starts[i] > len) atomicOr(bad, 2ull);
}

// *bad |= 4: an end outside [starts[r], starts[r + 1]]
__global__ __launch_bounds__(RC_THREADS) void rec_check_ends_kernel(const uint64_t* __restrict__ starts, const uint64_t* __restrict__ ends,
                                                                    uint64_t n_records, unsigned long long* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i < n_records && !rec_ends_valid(starts, ends, i)) atomicOr(bad, 4ull);
}

// a file's records (fastx.hip keeps the first byte of every header line in front of the next record's bytes): ends[r] =
// starts[r + 1] - 1 for every record but the last
__global__ __launch_bounds__(RC_THREADS) void rec_file_ends_kernel(const uint64_t* __restrict__ starts, uint64_t n_records, uint64_t* __restrict__ ends) {
    const uint64_t r = (uint64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (r >= n_records) return;
    const uint64_t s = starts[r], e = starts[r + 1];
    ends[r] = r + 1 < n_records && e > s ? e - 1 : e;
}

// the rule of the DNA records (rec_assign) or, ENDS, the one with explicit ends (rec_assign_ends; ends may be null)
template <bool ENDS>
__device__ __forceinline__ bool rec_assign_by(const uint64_t* starts, const uint64_t* ends, uint64_t n_records, uint64_t pos, uint32_t k, uint64_t* rec) {
    if constexpr (ENDS) return rec_assign_ends(starts, ends, n_records, pos, k, rec);
    else return rec_assign(starts, n_records, pos, k, rec);
}

// packed: pos[i] becomes the key (record << hbits) | hash, or 0 for a dropped pair
template <bool ENDS>
__global__ __launch_bounds__(RC_THREADS) void rec_assign_packed_kernel(const uint64_t* __restrict__ hash, uint64_t* __restrict__ pos, uint64_t n,
                                                                       const uint64_t* __restrict__ starts, const uint64_t* __restrict__ ends,
                                                                       uint64_t n_records, uint32_t k, int hbits) {
    const uint64_t i = (uint64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= n) return;
    uint64_t r = 0;
    const bool keep = rec_assign_by<ENDS>(starts, ends, n_records, pos[i], k, &r);
    pos[i] = keep ? ((hbits < 64 ? r << hbits : 0ull) | hash[i]) : 0ull;
}
// wide: pos[i] becomes the record number; a dropped pair becomes (record 0, hash 0)
template <bool ENDS>
__global__ __launch_bounds__(RC_THREADS) void rec_assign_wide_kernel(uint64_t* __restrict__ hash, uint64_t* __restrict__ pos, uint64_t n,
                                                                     const uint64_t* __restrict__ starts, const uint64_t* __restrict__ ends,
                                                                     uint64_t n_records, uint32_t k) {
    const uint64_t i = (uint64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= n) return;
    uint64_t r = 0;
    const bool keep = rec_assign_by<ENDS>(starts, ends, n_records, pos[i], k, &r);
    pos[i] = keep ? r : 0ull;
    if (!keep) hash[i] = 0ull;
}

// The sorted distinct entries: packed, u_key[i]; wide, (u_rec[i], u_hash[i]).  `first` says whether entry 0 is the dropped
// pairs' run.
struct RecRuns {
    const uint64_t* u_key;
    const uint64_t* u_rec;
    const uint64_t* u_hash;
    const uint64_t* counts;
    const uint64_t* n_runs;
    int hbits;                 // packed only
    bool packed;
    __device__ __forceinline__ uint64_t skip() const {
        if (*n_runs == 0) return 0;
        return packed ? (u_key[0] == 0 ? 1 : 0) : ((u_rec[0] == 0 && u_hash[0] == 0) ? 1 : 0);
    }
    __device__ __forceinline__ uint64_t rec(uint64_t i) const { return packed ? (hbits < 64 ? u_key[i] >> hbits : 0ull) : u_rec[i]; }
    __device__ __forceinline__ uint64_t hash(uint64_t i) const {
        return packed ? (hbits < 64 ? u_key[i] & (((uint64_t)1 << hbits) - 1) : u_key[i]) : u_hash[i];
    }
};

__global__ __launch_bounds__(RC_THREADS) void rec_finish_kernel(RecRuns runs, uint64_t* __restrict__ out_hashes, uint64_t* __restrict__ out_abunds,
                                                                uint64_t* __restrict__ n_out) {
    const uint64_t skip = runs.skip(), n = *runs.n_runs - skip;
    const uint64_t i = (uint64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i == 0) *n_out = n;
    if (i >= n) return;
    out_hashes[i] = runs.hash(i + skip);
    if (out_abunds) out_abunds[i] = runs.counts[i + skip];
}

// offsets[r] = first entry whose record is >= r, for r = 0 .. n_records
__global__ __launch_bounds__(RC_THREADS) void rec_offsets_kernel(RecRuns runs, uint64_t n_records, uint64_t* __restrict__ offsets) {
    const uint64_t r = (uint64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (r > n_records) return;
    const uint64_t skip = runs.skip(), n = *runs.n_runs - skip;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (runs.rec(mid + skip) < r) lo = mid + 1; else hi = mid;
    }
    offsets[r] = lo;
}

}  // namespace

hipError_t records_pairs_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, uint64_t seed, uint64_t thr, uint64_t* d_hash,
                                uint64_t* d_pos, unsigned long long* d_count, uint64_t cap, hipStream_t stream) {
    if (k == 0 || k > (uint32_t)SK_FAST_MAX_K) return hipErrorInvalidValue;
    if (len < k) return hipSuccess;
    return launcher<RecordsLaunch>(k)(d_seq, len, seed, thr, d_hash, d_pos, d_count, cap, stream);
}

hipError_t records_check_starts_launch(const uint64_t* d_starts, uint64_t n_records, uint64_t len, unsigned long long* d_bad,
                                       hipStream_t stream) {
    hipLaunchKernelGGL(rec_check_starts_kernel, dim3(rc_grid(n_records + 1)), dim3(RC_THREADS), 0, stream, d_starts, n_records, len, d_bad);
    return hipGetLastError();
}

// temp layout: [n_runs: 256 bytes][A: n u64][B: n u64][the packed sort's own temp | C: n u64, the pair primitives' temp]
size_t records_csr_temp_bytes(uint64_t n_pairs) {
    const uint64_t n = n_pairs ? n_pairs : 1;
    const size_t packed = sort_unique_temp_bytes(n);
    const size_t wide = al256(n * 8) + al256(sort_pairs_temp_bytes(n) > rle_pairs_temp_bytes(n) ? sort_pairs_temp_bytes(n) : rle_pairs_temp_bytes(n));
    return 256 + 2 * al256(n * 8) + (packed > wide ? packed : wide) + 256;
}

hipError_t records_check_ends_launch(const uint64_t* d_starts, const uint64_t* d_ends, uint64_t n_records, unsigned long long* d_bad,
                                     hipStream_t stream) {
    if (n_records == 0) return hipSuccess;
    hipLaunchKernelGGL(rec_check_ends_kernel, dim3(rc_grid(n_records)), dim3(RC_THREADS), 0, stream, d_starts, d_ends, n_records, d_bad);
    return hipGetLastError();
}

hipError_t records_file_ends_launch(const uint64_t* d_starts, uint64_t n_records, uint64_t* d_ends, hipStream_t stream) {
    if (n_records == 0) return hipSuccess;
    hipLaunchKernelGGL(rec_file_ends_kernel, dim3(rc_grid(n_records)), dim3(RC_THREADS), 0, stream, d_starts, n_records, d_ends);
    return hipGetLastError();
}

namespace {

// ENDS: assign by rec_assign_ends with d_ends (may be null); else by rec_assign
template <bool ENDS>
hipError_t records_csr_run(uint64_t* d_pair_hash, uint64_t* d_pair_pos, uint64_t n_pairs, const uint64_t* d_starts, const uint64_t* d_ends,
                           uint64_t n_records, uint32_t k, uint64_t max_hash, uint64_t* d_hashes, uint64_t* d_abunds, uint64_t* d_offsets,
                           uint64_t* d_n_out, void* d_temp, size_t temp_bytes, hipStream_t stream) {
    if (n_pairs == 0 || n_records == 0) {
        hipError_t e = hipMemsetAsync(d_offsets, 0, (n_records + 1) * 8, stream);
        return e != hipSuccess ? e : hipMemsetAsync(d_n_out, 0, 8, stream);
    }
    if (n_pairs > 0xffffffffull || n_records > 0xffffffffull) return hipErrorInvalidValue;
    if (temp_bytes < records_csr_temp_bytes(n_pairs)) return hipErrorInvalidValue;
    const uint64_t n = n_pairs;
    char* base = (char*)d_temp;
    uint64_t* d_n_runs = (uint64_t*)base;
    uint64_t* A = (uint64_t*)(base + 256);
    uint64_t* B = (uint64_t*)(base + 256 + al256(n * 8));
    char* rest = base + 256 + 2 * al256(n * 8);
    const size_t rest_bytes = temp_bytes - (256 + 2 * al256(n * 8));
    const int hbits = rec_hash_bits(max_hash);
    RecRuns runs{};
    runs.n_runs = d_n_runs;
    runs.hbits = hbits;
    runs.packed = rec_packed(n_records, max_hash);
    hipError_t e;
    if (runs.packed) {
        hipLaunchKernelGGL((rec_assign_packed_kernel<ENDS>), dim3(rc_grid(n)), dim3(RC_THREADS), 0, stream, (const uint64_t*)d_pair_hash, d_pair_pos,
                           n, d_starts, d_ends, n_records, k, hbits);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        const int bits = rec_bits(n_records - 1) + hbits;
        if ((e = sort_unique(d_pair_pos, n, A, B, d_n_runs, rest, rest_bytes, bits, stream)) != hipSuccess) return e;
        runs.u_key = A;
        runs.counts = B;
    } else {
        hipLaunchKernelGGL((rec_assign_wide_kernel<ENDS>), dim3(rc_grid(n)), dim3(RC_THREADS), 0, stream, d_pair_hash, d_pair_pos, n, d_starts, d_ends,
                           n_records, k);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        uint64_t* C = (uint64_t*)rest;
        void* prim = rest + al256(n * 8);
        const size_t prim_bytes = rest_bytes - al256(n * 8);
        // stable passes: by hash, then by record
        if ((e = sort_pairs(d_pair_hash, A, d_pair_pos, B, n, hbits, prim, prim_bytes, stream)) != hipSuccess) return e;
        const int rbits = rec_bits(n_records - 1) > 0 ? rec_bits(n_records - 1) : 1;
        if ((e = sort_pairs(B, d_pair_pos, A, d_pair_hash, n, rbits, prim, prim_bytes, stream)) != hipSuccess) return e;
        if ((e = rle_pairs(d_pair_pos, d_pair_hash, n, A, B, C, d_n_runs, prim, prim_bytes, stream)) != hipSuccess) return e;
        runs.u_rec = A;
        runs.u_hash = B;
        runs.counts = C;
    }
    hipLaunchKernelGGL(rec_finish_kernel, dim3(rc_grid(n)), dim3(RC_THREADS), 0, stream, runs, d_hashes, d_abunds, d_n_out);
    hipLaunchKernelGGL(rec_offsets_kernel, dim3(rc_grid(n_records + 1)), dim3(RC_THREADS), 0, stream, runs, n_records, d_offsets);
    return hipGetLastError();
}

}  // namespace

hipError_t records_csr_launch(uint64_t* d_pair_hash, uint64_t* d_pair_pos, uint64_t n_pairs, const uint64_t* d_starts, uint64_t n_records,
                              uint32_t k, uint64_t max_hash, uint64_t* d_hashes, uint64_t* d_abunds, uint64_t* d_offsets, uint64_t* d_n_out,
                              void* d_temp, size_t temp_bytes, hipStream_t stream) {
    return records_csr_run<false>(d_pair_hash, d_pair_pos, n_pairs, d_starts, nullptr, n_records, k, max_hash, d_hashes, d_abunds, d_offsets, d_n_out,
                                  d_temp, temp_bytes, stream);
}

hipError_t records_csr_ends_launch(uint64_t* d_pair_hash, uint64_t* d_pair_pos, uint64_t n_pairs, const uint64_t* d_starts, const uint64_t* d_ends,
                                   uint64_t n_records, uint32_t k, uint64_t max_hash, uint64_t* d_hashes, uint64_t* d_abunds, uint64_t* d_offsets,
                                   uint64_t* d_n_out, void* d_temp, size_t temp_bytes, hipStream_t stream) {
    return records_csr_run<true>(d_pair_hash, d_pair_pos, n_pairs, d_starts, d_ends, n_records, k, max_hash, d_hashes, d_abunds, d_offsets, d_n_out,
                                 d_temp, temp_bytes, stream);
}

}  // namespace smg
