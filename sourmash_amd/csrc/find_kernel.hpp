// find_kernel.hpp -- the kernel that finds a query sketch's k-mers in a buffer for k = 1 .. SK_FAST_MAX_K (template) and its launch
// table, shared by the parts of sketch_find_k.hip.  See sketch_find.hip for the design notes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "find_core.hpp"
#include "kmer_core.hpp"
#include "records_kernel.hpp"
#include "sketch_kernel.hpp"

namespace smg {

// LdsSink's staging of (hash, position) pairs (kmer_core.hpp) with a filter where the pairs leave LDS: only members of the query
// reach HBM.  The walk's append is LdsSink's -- a slot from the LDS counter, two LDS stores -- so the membership test, with its
// dependent reads of the directory and of q, is not in the per-lane walk, where one lane of a wave keeps a hash once in a while
// and the other 63 would wait for its loads; it is paid at flush time, by all BLOCK lanes at once, one staged pair each.
// *out_count keeps counting past out_cap, entries past it are dropped.  The kernel declares the LDS; pair_walk zeroes *s_cnt in
// front of its first barrier.
template <int CAP, int BLOCK>
struct FilterSink {
    uint64_t* s_hash;
    uint64_t* s_pos;
    unsigned int* s_cnt;
    FindQuery query;
    uint64_t* out_hash;
    uint64_t* out_pos;
    unsigned long long* out_count;
    uint64_t out_cap;

    __device__ __forceinline__ bool member(uint64_t h) const { return find_member(query.q, query.dir, query.shift, query.max_hash, h); }

    __device__ __forceinline__ void append(uint64_t h, uint64_t pos) const {
        const unsigned int idx = atomicAdd(s_cnt, 1u);
        if (idx < (unsigned)CAP) {
            s_hash[idx] = h;
            s_pos[idx] = pos;
        } else if (member(h)) {   // staging is full (e.g. scaled == 1: a tile keeps 4,096 pairs): test here, straight to HBM
            const unsigned long long g = atomicAdd(out_count, 1ull);
            if (g < out_cap) {
                out_hash[g] = h;
                out_pos[g] = pos;
            }
        }
    }

    // Filter the staged pairs and write the members out if at least `at_least` pairs are staged: CAP / 2 between tiles, 1 at the
    // end.  Called by every thread of the workgroup, behind a barrier.  Every lane takes the pairs tid, tid + BLOCK, ..; the
    // members of a wave's 64 pairs get their places with one ballot and one atomic of the wave's first member lane.
    // The lane number comes from behind opaque(), as the position in the kernel's emit does: what the optimiser can make of
    // threadIdx.x in front of the tile loop -- the lane's LDS addresses here -- it keeps in registers through the walk, and eight
    // more VGPRs there cost a wave per SIMD at nine ksizes (profiles/find_kernel_resources.txt).
    __device__ __forceinline__ void flush(unsigned int at_least) const {
        const unsigned int cnt = *s_cnt;                      // workgroup-uniform
        if (cnt < at_least) return;
        const unsigned int n = cnt < (unsigned)CAP ? cnt : (unsigned)CAP;
        const unsigned int tid = opaque(threadIdx.x);
        for (unsigned int i0 = 0; i0 < n; i0 += BLOCK) {
            const unsigned int i = i0 + tid;
            uint64_t h = 0, pos = 0;
            bool m = false;
            if (i < n) {
                h = s_hash[i];
                pos = s_pos[i];
                m = member(h);
            }
            const unsigned long long mask = __ballot(m);
            if (mask == 0) continue;                          // wave-uniform
            // members of the wave in front of this lane
            const unsigned int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            unsigned long long b = 0;
            if (m && rank == 0) b = atomicAdd(out_count, (unsigned long long)__popcll(mask));
            const int leader = __ffsll(mask) - 1;             // the first member lane, wave-uniform
            b = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), leader) << 32) |
                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, leader);
            if (m) {
                const unsigned long long g = b + rank;
                if (g < out_cap) {
                    out_hash[g] = h;
                    out_pos[g] = pos;
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) *s_cnt = 0;
    }
};

// pair_walk (records_kernel.hpp) with the filtering sink: every k-mer of seq whose canonical hash h, 1 <= h <= query.max_hash, is
// a member of the query is appended to out_hash together with the position of its first byte in the caller's buffer, in out_pos.
// Unordered; *out_count keeps counting past out_cap.  seq is 16-byte aligned, its first `skip` bytes precede the caller's buffer
// (len includes them).
template <int K, int P>
__global__ __launch_bounds__(SK_BLOCK) void find_dna_kernel(
    const uint8_t* __restrict__ seq, uint64_t len, uint64_t seed, FindQuery query,
    uint64_t* __restrict__ out_hash, uint64_t* __restrict__ out_pos, unsigned long long* __restrict__ out_count, uint64_t out_cap,
    uint64_t n_tiles, uint32_t skip) {
    constexpr int IN_CHUNKS = TileGeom<K, P, SK_BLOCK>::IN_CHUNKS;
    __shared__ __attribute__((aligned(16))) uint32_t s_in[IN_CHUNKS * 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_comp[sk_staged(K) ? IN_CHUNKS * 4 : 4];
    __shared__ unsigned int s_dirty;
    __shared__ uint64_t s_hash[REC_OUT_CAP];
    __shared__ uint64_t s_pos[REC_OUT_CAP];
    __shared__ unsigned int s_cnt;
    const FilterSink<REC_OUT_CAP, SK_BLOCK> sink{s_hash, s_pos, &s_cnt, query, out_hash, out_pos, out_count, out_cap};
    pair_walk<K, P>(seq, len, seed, query.max_hash, n_tiles, skip, sink, s_in, s_comp, &s_dirty, &s_cnt);
}

// The launchers of find_dna_kernel<K, 16>, one per ksize: six parts in sketch_find_k.hip (tile_launch.hpp).  grid: as in
// launch_pair_kernel.
struct FindLaunch {
    using fn = hipError_t (*)(const uint8_t*, uint64_t, uint64_t, FindQuery, uint64_t*, uint64_t*, unsigned long long*, uint64_t, uint32_t,
                              hipStream_t);
    static constexpr int KMAX = SK_FAST_MAX_K;
    template <int K>
    static hipError_t launch(const uint8_t* d_seq, uint64_t len, uint64_t seed, FindQuery query, uint64_t* d_hash, uint64_t* d_pos,
                             unsigned long long* d_count, uint64_t cap, uint32_t grid, hipStream_t stream) {
        return launch_pair_kernel(d_seq, len, grid, [&](dim3 g, const TileSpan& t) {
            hipLaunchKernelGGL((find_dna_kernel<K, 16>), g, dim3(SK_BLOCK), 0, stream, t.seq, t.len, seed, query, d_hash, d_pos, d_count,
                               cap, t.n_tiles, t.skip);
        });
    }
};

}  // namespace smg
