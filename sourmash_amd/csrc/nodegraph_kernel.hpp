// nodegraph_kernel.hpp -- the Nodegraph (Bloom filter) kernels: the k-mer kernel (the sketch kernel's tile staging with a two-bit
// rolling walk in place of MurmurHash3), the hash-array kernel and the read-only matches kernel, all over one bit sink.  See
// nodegraph.hip for the design notes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_api.hpp"
#include "kmer_core.hpp"
#include "nodegraph_core.hpp"

namespace smg {

constexpr int NG_BLOCK = 256;                 // 4 waves, one per SIMD (the sketch kernel's workgroup)
constexpr int NG_RUN = 16;                    // k-mer start positions per lane and tile
constexpr int NG_TILE = NG_BLOCK * NG_RUN;    // start positions per tile
constexpr int NG_HALO = 32;                   // bytes past the tile a lane may read: k - 1 <= 31
constexpr int NG_IN_CHUNKS = (NG_TILE + NG_HALO) / 16;
constexpr uint64_t NG_LDS_MAX_WORDS = 16384;  // the LDS form holds every table of the graph: up to 64 KiB of words

// Set bit (h mod size) of every table.  LDS: in the workgroup's copy s_w (LDS atomic OR, no return); otherwise in the device
// words behind a read filter (bits only ever turn on, so a bit already visible as set needs no atomic), counting the table-0
// bits this lane turned from 0 to 1 in *nocc (from the old word the atomic returns).
template <bool LDS>
__device__ __forceinline__ void ng_set(uint64_t h, const NgTable* __restrict__ tabs, uint32_t n_tables, uint32_t* s_w,
                                       uint32_t* words, uint32_t& nocc) {
    for (uint32_t t = 0; t < n_tables; ++t) {
        const NgTable T = tabs[t];
        const uint64_t b = ng_mod(h, T.size, T.magic);
        const uint64_t w = T.off + (b >> 5);
        const uint32_t bit = 1u << (uint32_t)(b & 31);
        if constexpr (LDS) {
            atomicOr(&s_w[w], bit);
        } else {
            if (!(words[w] & bit)) {
                const uint32_t old = atomicOr(&words[w], bit);
                if (t == 0 && !(old & bit)) ++nocc;
            }
        }
    }
}

// Fold a workgroup's LDS copy into the device words: an atomic only where the copy holds a bit the device word does not show;
// table-0 bits that the atomic turned on are counted.
__device__ __forceinline__ void ng_fold_lds(const uint32_t* s_w, uint32_t n_words, uint64_t t0_words, uint32_t* words,
                                            uint32_t& nocc) {
    for (uint32_t i = threadIdx.x; i < n_words; i += blockDim.x) {
        const uint32_t v = s_w[i];
        if (v & ~words[i]) {
            const uint32_t old = atomicOr(&words[i], v);
            if (i < t0_words) nocc += (uint32_t)__popc(v & ~old);
        }
    }
}

// one atomic per wave for the table-0 bits its lanes turned on (every lane of the wave must be here)
__device__ __forceinline__ void ng_add_occupied(uint32_t nocc, unsigned long long* occ) {
    unsigned long long s = nocc;
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(occ, s);
}

// Every k-mer of seq[0, len) whose k bytes are all in ACGTacgt (case folded) sets its bits: h = min(forward, reverse) two-bit
// words.  Tiles of NG_TILE start positions are staged in LDS as the sketch kernel stages them (16-byte chunks, the tile's
// k - 1 byte halo included; bytes past len read as 0, which is no base); lane l walks the NG_RUN + k - 1 bytes of its
// positions with a forward word, a reverse word and a count of valid bases.  seq is 16-byte aligned; its first `skip` bytes
// precede the caller's buffer and are masked to 0.
template <bool LDS>
__global__ __launch_bounds__(NG_BLOCK) void ng_dna_kernel(const uint8_t* __restrict__ seq, uint64_t len, uint32_t k,
                                                          const NgTable* __restrict__ tabs, uint32_t n_tables, uint32_t* words,
                                                          uint32_t n_words, uint64_t t0_words, unsigned long long* occ,
                                                          uint64_t n_tiles, uint32_t skip) {
    __shared__ __attribute__((aligned(16))) uint32_t s_in[NG_IN_CHUNKS * 4];
    extern __shared__ uint32_t s_w[];

    const int tid = threadIdx.x;
    if constexpr (LDS)
        for (uint32_t i = tid; i < n_words; i += NG_BLOCK) s_w[i] = 0;
    const uint64_t kmask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    const uint32_t rshift = 2 * (k - 1);
    const uint32_t nbytes = NG_RUN + k - 1;
    const uint32_t ndw = (nbytes + 3) / 4;
    uint32_t nocc = 0;

    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t base = tile * (uint64_t)NG_TILE;
        __syncthreads();
        stage_tile<NG_IN_CHUNKS, false, NG_BLOCK>(seq, base, len, skip, s_in, nullptr, nullptr);
        __syncthreads();
        const uint32_t* lane = &s_in[tid * (NG_RUN / 4)];
        uint64_t fw = 0, rv = 0;
        uint32_t nv = 0;
        for (uint32_t j = 0; j < ndw; ++j) {
            const uint32_t d = lane[j];
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                if (4 * j + b < nbytes) {
                    bool ok;
                    const uint32_t code = ng_code((d >> (8 * b)) & 0xffu, &ok);
                    fw = ((fw << 2) | code) & kmask;
                    rv = (rv >> 2) | ((uint64_t)(code ^ 1u) << rshift);
                    nv = ok ? nv + 1 : 0;
                    if (nv >= k) ng_set<LDS>(fw < rv ? fw : rv, tabs, n_tables, s_w, words, nocc);
                }
            }
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        ng_fold_lds(s_w, n_words, t0_words, words, nocc);
    }
    ng_add_occupied(nocc, occ);
}

// every hash of hashes[0, n) sets its bits (the same two forms)
template <bool LDS>
__global__ __launch_bounds__(NG_BLOCK) void ng_hashes_kernel(const uint64_t* __restrict__ hashes, uint64_t n,
                                                             const NgTable* __restrict__ tabs, uint32_t n_tables, uint32_t* words,
                                                             uint32_t n_words, uint64_t t0_words, unsigned long long* occ) {
    extern __shared__ uint32_t s_w[];
    if constexpr (LDS) {
        for (uint32_t i = threadIdx.x; i < n_words; i += NG_BLOCK) s_w[i] = 0;
        __syncthreads();
    }
    uint32_t nocc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * NG_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NG_BLOCK)
        ng_set<LDS>(hashes[i], tabs, n_tables, s_w, words, nocc);
    if constexpr (LDS) {
        __syncthreads();
        ng_fold_lds(s_w, n_words, t0_words, words, nocc);
    }
    ng_add_occupied(nocc, occ);
}

// out[r] = how many hashes of CSR row r have their bit set in every table (read-only).  One wave per row.
__global__ __launch_bounds__(NG_BLOCK) void ng_matches_kernel(const uint64_t* __restrict__ hashes,
                                                              const uint64_t* __restrict__ offsets, uint64_t n_rows,
                                                              const NgTable* __restrict__ tabs, uint32_t n_tables,
                                                              const uint32_t* __restrict__ words, uint64_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_waves = (uint64_t)gridDim.x * (NG_BLOCK / 64);
    for (uint64_t r = ((uint64_t)blockIdx.x * NG_BLOCK + threadIdx.x) >> 6; r < n_rows; r += n_waves) {
        const uint64_t lo = offsets[r], hi = offsets[r + 1];
        unsigned long long cnt = 0;
        for (uint64_t i = lo + lane; i < hi; i += 64) {
            const uint64_t h = hashes[i];
            uint32_t all = 1;
            for (uint32_t t = 0; t < n_tables && all; ++t) {
                const NgTable T = tabs[t];
                const uint64_t b = ng_mod(h, T.size, T.magic);
                all = (words[T.off + (b >> 5)] >> (uint32_t)(b & 31)) & 1u;
            }
            cnt += all;
        }
        for (int d = 32; d; d >>= 1) cnt += __shfl_xor(cnt, d);
        if (lane == 0) out[r] = cnt;
    }
}

}  // namespace smg
