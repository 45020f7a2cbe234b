// records_kernel.hpp -- the walk of the DNA (hash, position) kernels, the kernel behind per-record sketches for k = 1 ..
// SK_FAST_MAX_K (template) and its launch table, shared by the parts of sketch_records_k.hip.  See sketch_records.hip for the
// design notes.  find_kernel.hpp has the second kernel over the same walk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "kmer_core.hpp"
#include "sketch_kernel.hpp"

namespace smg {

constexpr int REC_OUT_CAP = SK_OUT_CAP / 2;   // LDS staging entries: 1,024 (hash, position) pairs, the sketch kernel's 16 KiB

// The sketch kernel's staging and per-lane walk (sketch_kernel.hpp: process_lane_staged where sk_staged(K), the same choice of
// multiply, the same tiles) with a pair sink: every kept hash (1 <= h <= thr) is appended to the sink together with the position
// of its k-mer's first byte in the caller's buffer.  The sink is flushed at REC_OUT_CAP / 2 pairs between tiles and at 1 behind
// the last.  seq is 16-byte aligned, its first `skip` bytes precede the caller's buffer (len includes them).  The kernel
// declares the LDS: s_in and s_comp as TileGeom<K, P, SK_BLOCK> sizes them (s_comp is read where sk_staged(K) only), and the
// sink's own counter s_cnt, which is zeroed here in front of the first barrier.
template <int K, int P, class Sink>
__device__ __forceinline__ void pair_walk(const uint8_t* __restrict__ seq, uint64_t len, uint64_t seed, uint64_t thr, uint64_t n_tiles,
                                          uint32_t skip, const Sink& sink, uint32_t* s_in, uint32_t* s_comp, unsigned int* s_dirty,
                                          unsigned int* s_cnt) {
    using T = TileGeom<K, P, SK_BLOCK>;
    constexpr int TILE = T::TILE, LANE_RD = T::LANE_RD, IN_CHUNKS = T::IN_CHUNKS;
    constexpr bool STAGED = sk_staged(K);
    static_assert(P == 16, "lane runs of 16 positions");

    const int tid = threadIdx.x;
    if (tid == 0) *s_cnt = 0;

    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t base = tile * (uint64_t)TILE;
        if constexpr (STAGED) {
            if (tid == 0) *s_dirty = 0;
        }
        __syncthreads();
        stage_tile<IN_CHUNKS, STAGED, SK_BLOCK>(seq, base, len, skip, s_in, s_comp, s_dirty);
        __syncthreads();
        uint32_t raw[LANE_RD];
        read_window<LANE_RD, P>(s_in, tid, raw);
        auto emit = [&](int o, uint64_t h) {
            // the position is made here, from the lane number behind a barrier the optimiser does not look through: otherwise the 16
            // positions of a lane are computed in front of the walk and stay live through it (20 VGPRs, a wave per SIMD at k = 31
            // and 51: profiles/singleton_kernel_resources.txt).  Valid k-mers never start in the prefix, so pos >= 0.
            const uint64_t pos = base + (uint64_t)(opaque(threadIdx.x) * P + (uint32_t)o) - skip;
            sink.append(h, pos);
        };
        if constexpr (STAGED) {
            uint32_t comp[LANE_RD];
            read_window<LANE_RD, P>(s_comp, tid, comp);
            const bool dirty = __builtin_amdgcn_readfirstlane(*s_dirty) != 0;
            process_lane_staged<K, P, true, sk_plain_mul(K, false)>(raw, comp, dirty, seed, thr, emit);
        } else {
            process_lane<K, P, true, sk_plain_mul(K, false)>(raw, seed, thr, emit);
        }
        __syncthreads();
        sink.flush(REC_OUT_CAP / 2);
    }
    __syncthreads();
    sink.flush(1);
}

// pair_walk with LdsSink: the pairs go to out_hash / out_pos.  Unordered; *out_count keeps counting past out_cap, entries past
// it are dropped.
template <int K, int P>
__global__ __launch_bounds__(SK_BLOCK) void records_dna_kernel(
    const uint8_t* __restrict__ seq, uint64_t len, uint64_t seed, uint64_t thr,
    uint64_t* __restrict__ out_hash, uint64_t* __restrict__ out_pos, unsigned long long* __restrict__ out_count, uint64_t out_cap,
    uint64_t n_tiles, uint32_t skip) {
    constexpr int IN_CHUNKS = TileGeom<K, P, SK_BLOCK>::IN_CHUNKS;
    __shared__ __attribute__((aligned(16))) uint32_t s_in[IN_CHUNKS * 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_comp[sk_staged(K) ? IN_CHUNKS * 4 : 4];
    __shared__ unsigned int s_dirty;
    __shared__ uint64_t s_hash[REC_OUT_CAP];
    __shared__ uint64_t s_pos[REC_OUT_CAP];
    __shared__ unsigned int s_cnt;
    __shared__ unsigned long long s_base;
    const LdsSink<REC_OUT_CAP, SK_BLOCK, 2> sink{{s_hash, s_pos}, &s_cnt, &s_base, {out_hash, out_pos}, out_count, out_cap};
    pair_walk<K, P>(seq, len, seed, thr, n_tiles, skip, sink, s_in, s_comp, &s_dirty, &s_cnt);
}

// What the launchers of the two pair kernels share: the tiles of the buffer, nothing to do for none, the grid (0: the sketch
// kernel's choice; otherwise exactly that many workgroups, a test's way to many tiles per workgroup on a small input).
// launch(grid, span) starts the kernel.
template <class F>
inline hipError_t launch_pair_kernel(const uint8_t* d_seq, uint64_t len, uint32_t grid, F&& launch) {
    const TileSpan t = align_to_tiles(d_seq, len, (uint64_t)SK_BLOCK * 16);
    if (t.n_tiles == 0) return hipSuccess;
    launch(dim3(grid ? grid : sk_grid(t.n_tiles)), t);
    return hipGetLastError();
}

// The launchers of records_dna_kernel<K, 16>, one per ksize: six parts in sketch_records_k.hip (tile_launch.hpp)
struct RecordsLaunch {
    using fn = hipError_t (*)(const uint8_t*, uint64_t, uint64_t, uint64_t, uint64_t*, uint64_t*, unsigned long long*, uint64_t, hipStream_t);
    static constexpr int KMAX = SK_FAST_MAX_K;
    template <int K>
    static hipError_t launch(const uint8_t* d_seq, uint64_t len, uint64_t seed, uint64_t thr, uint64_t* d_hash, uint64_t* d_pos,
                             unsigned long long* d_count, uint64_t cap, hipStream_t stream) {
        return launch_pair_kernel(d_seq, len, 0, [&](dim3 grid, const TileSpan& t) {
            hipLaunchKernelGGL((records_dna_kernel<K, 16>), grid, dim3(SK_BLOCK), 0, stream, t.seq, t.len, seed, thr, d_hash, d_pos,
                               d_count, cap, t.n_tiles, t.skip);
        });
    }
};

}  // namespace smg
