// protein_records.hip -- the residue side of per-record sketching (sketch_records.hip holds the rest): protein / dayhoff / hp
// sketches of every record of a buffer in one pass, for protein input and for DNA input translated in six frames.
//
// GPU counterpart of the reference's singleton loop over a proteome or over reads (src/sourmash/command_sketch.py:712-739 with
// add_protein / add_sequence on a protein sketch: src/core/src/signature.rs:257-261, 307-393), without a launch, a sort or a
// read-back per record:
//   translate  (DNA input) translate_records_kernel: every record's six frames into a block of its own of one residue buffer
//              (translate_records_core.hpp); the block starts are an exclusive scan of the block sizes.  Protein input goes
//              through residues_kernel (protein.hip) as a whole: positions in the residue buffer are positions in the input.
//   pairs      window_pairs_kernel<NB>: the round loop of the residue window kernels (residue_kernel.hpp; residue_core.hpp holds
//              the lane) with a (hash, window start) sink.  The kernel knows nothing about records.
//   the rest   records_csr_ends_launch (sketch_records.hip): assign by the rule with explicit ends (records_core.hpp), sort by
//              (record, hash), offsets.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>
#include "device_api.hpp"
#include "murmur3.hpp"
#include "residues.hpp"
#include "residue_core.hpp"
#include "residue_kernel.hpp"
#include "records_core.hpp"
#include "translate_records_core.hpp"

namespace smg {

namespace {

// LDS staging entries for kept (hash, start) pairs: 2 x 8 KiB, the 16 KiB of window_fast_kernel's 2,048 hashes.  A round of a
// workgroup covers 2,048 window starts; at scaled = 200 it keeps about ten of them.
constexpr int RWP_OUT_CAP = 1024;

// residue_kernel.hpp's rounds with a (hash, window start) sink.  n: residue_n(n_host, d_n); the buffer is read as aligned 8-byte
// words up to ceil(n / 8).  SEP: 0xFF bytes separate (the translated buffer); protein input has no separators -- the records'
// ends do that work -- and a 0xFF byte in it is hashed as the reference hashes it.
template <int NB, bool SEP>
__global__ __launch_bounds__(RW_BLOCK) void window_pairs_kernel(const uint64_t* __restrict__ aa64, uint64_t n_host, const uint64_t* __restrict__ d_n,
                                                                ResidueTail t, uint64_t seed, uint64_t thr, uint64_t* __restrict__ out_hash,
                                                                uint64_t* __restrict__ out_pos, unsigned long long* __restrict__ out_count,
                                                                uint64_t cap) {
    __shared__ uint64_t s_hash[RWP_OUT_CAP];
    __shared__ uint64_t s_pos[RWP_OUT_CAP];
    __shared__ unsigned int s_cnt;
    __shared__ unsigned long long s_base;
    const LdsSink<RWP_OUT_CAP, RW_BLOCK, 2> sink{{s_hash, s_pos}, &s_cnt, &s_base, {out_hash, out_pos}, out_count, cap};
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    residue_rounds_kept<NB, SEP>(aa64, residue_n(n_host, d_n), t, seed, thr, sink);
}

template <int NB>
hipError_t window_pairs_launch(const uint8_t* d_aa, uint64_t n_bound, const uint64_t* d_n, uint32_t k, uint64_t seed, uint64_t thr,
                               uint64_t* d_hash, uint64_t* d_pos, unsigned long long* d_count, uint64_t cap, hipStream_t stream) {
    // (d_n: the translated buffer -- a size on the device, separators)
    const auto kernel = d_n ? window_pairs_kernel<NB, true> : window_pairs_kernel<NB, false>;
    hipLaunchKernelGGL(kernel, dim3(residue_grid(n_bound, k)), dim3(RW_BLOCK), 0, stream, (const uint64_t*)d_aa, n_bound, d_n, residue_tail(k), seed,
                       thr, d_hash, d_pos, d_count, cap);
    return hipGetLastError();
}

// sizes[r] = bytes of record r's block for r < n_records, sizes[n_records] = 0: the scan's input
__global__ __launch_bounds__(256) void block_sizes_kernel(const uint64_t* __restrict__ starts, const uint64_t* __restrict__ ends, uint64_t n_records,
                                                          uint64_t* __restrict__ sizes) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n_records) sizes[r] = translated_block_bytes(rec_len(starts, ends, r));
    else if (r == n_records) sizes[r] = 0;
}

// one aligned output word per lane (translate_records_core.hpp); aa has room for whole words
__global__ __launch_bounds__(256) void translate_records_kernel(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ starts,
                                                                const uint64_t* __restrict__ ends, const uint64_t* __restrict__ block_starts,
                                                                uint64_t n_records, uint32_t hf, uint64_t* __restrict__ aa64) {
    __shared__ uint8_t code_f[256], code_r[256], codon[216];
    fill_translate_tables(code_f, code_r, codon, hf);
    const TranslateTables T{code_f, code_r, codon};
    const uint64_t n_words = (block_starts[n_records] + 7) / 8;
    for (uint64_t G = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; G < n_words; G += (uint64_t)gridDim.x * blockDim.x)
        aa64[G] = translate_records_word(seq, starts, ends, block_starts, n_records, T, G);
}

size_t scan_temp_bytes(uint64_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)(n ? n : 1), rocprim::plus<uint64_t>(),
                                  (hipStream_t)0);
    return bytes;
}

}  // namespace

hipError_t residue_pairs_launch(const uint8_t* d_aa, uint64_t n_bound, const uint64_t* d_n, uint32_t k, uint64_t seed, uint64_t thr,
                                uint64_t* d_hash, uint64_t* d_pos, unsigned long long* d_count, uint64_t cap, hipStream_t stream) {
    if (k == 0 || k / 16 > (uint32_t)RW_MAX_NB || ((uintptr_t)d_aa & 7) != 0) return hipErrorInvalidValue;
    if (n_bound < k) return hipSuccess;
    switch (k / 16) {
    case 0: return window_pairs_launch<0>(d_aa, n_bound, d_n, k, seed, thr, d_hash, d_pos, d_count, cap, stream);
    case 1: return window_pairs_launch<1>(d_aa, n_bound, d_n, k, seed, thr, d_hash, d_pos, d_count, cap, stream);
    case 2: return window_pairs_launch<2>(d_aa, n_bound, d_n, k, seed, thr, d_hash, d_pos, d_count, cap, stream);
    case 3: return window_pairs_launch<3>(d_aa, n_bound, d_n, k, seed, thr, d_hash, d_pos, d_count, cap, stream);
    default: return window_pairs_launch<4>(d_aa, n_bound, d_n, k, seed, thr, d_hash, d_pos, d_count, cap, stream);
    }
}

uint64_t translated_records_bytes_bound(uint64_t len, uint64_t n_records) { return translated_records_bound(len, n_records); }

// temp layout: [block sizes: n_records + 1 u64][the scan's own temp]
size_t translate_records_temp_bytes(uint64_t n_records) { return al256((n_records + 1) * 8) + scan_temp_bytes(n_records + 1); }

hipError_t translate_records_launch(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, const uint64_t* d_ends, uint64_t n_records,
                                    uint32_t hash_function, uint64_t* d_block_starts, uint8_t* d_aa, void* d_temp, size_t temp_bytes,
                                    hipStream_t stream) {
    if (((uintptr_t)d_aa & 7) != 0 || temp_bytes < translate_records_temp_bytes(n_records)) return hipErrorInvalidValue;
    uint64_t* d_sizes = (uint64_t*)d_temp;
    hipLaunchKernelGGL(block_sizes_kernel, dim3(grid_for(n_records + 1, 256, 8192)), dim3(256), 0, stream, d_starts, d_ends, n_records, d_sizes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = temp_bytes - al256((n_records + 1) * 8);
    e = rocprim::exclusive_scan((char*)d_temp + al256((n_records + 1) * 8), bytes, d_sizes, d_block_starts, (uint64_t)0, (size_t)(n_records + 1),
                                rocprim::plus<uint64_t>(), stream);
    if (e != hipSuccess) return e;
    if (n_records == 0) return hipSuccess;
    const uint64_t words_bound = (translated_records_bound(len, n_records) + 7) / 8;
    hipLaunchKernelGGL(translate_records_kernel, dim3(grid_for(words_bound, 256, 8192)), dim3(256), 0, stream, d_seq, d_starts, d_ends,
                       (const uint64_t*)d_block_starts, n_records, hash_function, reinterpret_cast<uint64_t*>(d_aa));
    return hipGetLastError();
}

}  // namespace smg
