// hll_kernel.hpp -- the HyperLogLog register kernel for k = 1 .. SK_FAST_MAX_K (template) and its launch table, shared by the
// parts of hll_dense.hip.  See hll.hip for the design notes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "kmer_core.hpp"
#include "sketch_kernel.hpp"

namespace smg {

constexpr int HLL_LDS_MAX_P = 14;          // one u32 per register in LDS up to 2^14 registers (64 KiB)
constexpr uint64_t HLL_SEED = 42;          // sketch/hyperloglog/mod.rs: the seed of every HLL

// rank of a hash: leading zeros of its upper 64 - p bits, plus one (1 .. 65 - p); its register: the low p bits
__device__ __forceinline__ uint32_t hll_rank(uint64_t h, uint32_t p) {
    const uint64_t v = h >> p;
    return (v ? (uint32_t)__clzll((long long)v) : 64u) + 1u - p;
}

// Fold a workgroup's LDS register file into the device registers: read first, atomicMax only where the value is larger
// (after warm-up nearly every register of a workgroup is at or below the device's).
__device__ __forceinline__ void hll_fold_lds(const uint32_t* s_reg, uint32_t n_regs, uint32_t* regs) {
    for (uint32_t i = threadIdx.x; i < n_regs; i += blockDim.x) {
        const uint32_t v = s_reg[i];
        if (v > regs[i]) atomicMax(&regs[i], v);
    }
}

// The sketch kernel's staging and per-lane walk (sketch_kernel.hpp) with a register sink: every canonical k-mer hash h != 0
// of seq updates register h & (2^p - 1) to max(reg, rank(h)).  LDS == true: the workgroup's registers live in dynamic LDS (one
// u32 each, native ds_max_u32) and are folded into `regs` at the end; LDS == false (p > HLL_LDS_MAX_P): straight to `regs`
// behind a read filter.
// The instantiations that keep the plain 64-bit constant multiply (murmur3.hpp, mul_c64<C, PLAIN>): the limb form would cost each
// of them a wave per SIMD (profiles/mul_c64_kernel_resources.txt).
constexpr bool hll_plain_mul(int k, bool lds) { return k == 28 || k == 60 || (k == 57 && lds); }

template <int K, int P, bool LDS>
__global__ __launch_bounds__(SK_BLOCK) void hll_dna_kernel(const uint8_t* __restrict__ seq, uint64_t len, uint32_t p,
                                                           uint32_t* regs, uint64_t n_tiles, uint32_t skip) {
    using T = TileGeom<K, P, SK_BLOCK>;
    constexpr int TILE = T::TILE, LANE_RD = T::LANE_RD, IN_CHUNKS = T::IN_CHUNKS;
    static_assert(P == 16, "lane runs of 16 positions");

    __shared__ __attribute__((aligned(16))) uint32_t s_in[IN_CHUNKS * 4];
    extern __shared__ uint32_t s_reg[];

    const int tid = threadIdx.x;
    const uint32_t n_regs = 1u << p;
    const uint64_t mask = (uint64_t)n_regs - 1;
    if constexpr (LDS)
        for (uint32_t i = tid; i < n_regs; i += SK_BLOCK) s_reg[i] = 0;

    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t base = tile * (uint64_t)TILE;
        __syncthreads();
        // stage_tile<IN_CHUNKS, false> (kmer_core.hpp), kept inline: through the function, in either shape of its loader, <19, 16, true>
        // goes from 80 to 86 VGPRs, <20, 16, false> from 80 to 84, <28, 16, true> from 96 to 98 -- a wave per SIMD each.
        for (int c = tid; c < IN_CHUNKS; c += SK_BLOCK) {
            const uint64_t off = base + (uint64_t)c * 16;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (off + 16 <= len) {
                v = *reinterpret_cast<const uint4*>(seq + off);
            } else if (off < len) {
                uint32_t w[4] = {0, 0, 0, 0};
                for (uint64_t b = off; b < len; ++b) w[(b - off) >> 2] |= (uint32_t)seq[b] << (8 * ((b - off) & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            if (off == 0 && skip) {                      // blank the alignment prefix
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
                for (uint32_t b = 0; b < skip; ++b) w[b >> 2] &= ~(0xffu << (8 * (b & 3)));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4*>(&s_in[c * 4]) = v;
        }
        __syncthreads();
        uint32_t raw[LANE_RD];
        read_window<LANE_RD, P>(s_in, tid, raw);
        process_lane<K, P, false, hll_plain_mul(K, LDS)>(raw, HLL_SEED, ~0ull, [&](int, uint64_t h) {
            const uint32_t idx = (uint32_t)(h & mask);
            const uint32_t r = hll_rank(h, p);
            if constexpr (LDS) {
                if (s_reg[idx] < r) atomicMax(&s_reg[idx], r);
            } else {
                if (regs[idx] < r) atomicMax(&regs[idx], r);
            }
        });
    }
    if constexpr (LDS) {
        __syncthreads();
        hll_fold_lds(s_reg, n_regs, regs);
    }
}

// The launchers of hll_dna_kernel<K, 16, LDS>, one per ksize: six parts in hll_dense.hip (tile_launch.hpp)
struct HllLaunch {
    using fn = hipError_t (*)(const uint8_t*, uint64_t, uint32_t, uint32_t*, hipStream_t);
    static constexpr int KMAX = SK_FAST_MAX_K;
    template <int K>
    static hipError_t launch(const uint8_t* d_seq, uint64_t len, uint32_t p, uint32_t* d_regs, hipStream_t stream) {
        const TileSpan t = align_to_tiles(d_seq, len, (uint64_t)SK_BLOCK * 16);
        if (t.n_tiles == 0) return hipSuccess;
        const bool lds = p <= (uint32_t)HLL_LDS_MAX_P;
        const unsigned grid = lds_grid(t.n_tiles, lds);      // the fold is 2^p register checks per workgroup
        if (lds) {
            const size_t shm = (size_t)4 << p;
            const hipError_t allowed = allow_dynamic_lds<&hll_dna_kernel<K, 16, true>>(shm, (size_t)4 << HLL_LDS_MAX_P);
            if (allowed != hipSuccess) return allowed;
            hipLaunchKernelGGL((hll_dna_kernel<K, 16, true>), dim3(grid), dim3(SK_BLOCK), shm, stream, t.seq, t.len, p, d_regs,
                               t.n_tiles, t.skip);
        } else {
            hipLaunchKernelGGL((hll_dna_kernel<K, 16, false>), dim3(grid), dim3(SK_BLOCK), 0, stream, t.seq, t.len, p, d_regs,
                               t.n_tiles, t.skip);
        }
        return hipGetLastError();
    }
};

}  // namespace smg
