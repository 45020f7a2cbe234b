// records_kernel.hpp -- the (hash, position) kernel behind per-record sketches for k = 1 .. SK_FAST_MAX_K (template) and its
// launch table, shared by the parts of sketch_records_k.hip.  See sketch_records.hip for the design notes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "kmer_core.hpp"
#include "sketch_kernel.hpp"

namespace smg {

constexpr int REC_OUT_CAP = SK_OUT_CAP / 2;   // LDS staging entries: 1,024 (hash, position) pairs, the sketch kernel's 16 KiB

// The sketch kernel's staging and per-lane walk (sketch_kernel.hpp: process_lane_staged where sk_staged(K), the same choice of
// multiply, the same tiles) with a pair sink: every kept hash (1 <= h <= thr) is appended to out_hash together with the position
// of its k-mer's first byte in the caller's buffer, in out_pos.  Unordered; *out_count keeps counting past out_cap, entries past
// it are dropped.  seq is 16-byte aligned, its first `skip` bytes precede the caller's buffer (len includes them).
template <int K, int P>
__global__ __launch_bounds__(SK_BLOCK) void records_dna_kernel(
    const uint8_t* __restrict__ seq, uint64_t len, uint64_t seed, uint64_t thr,
    uint64_t* __restrict__ out_hash, uint64_t* __restrict__ out_pos, unsigned long long* __restrict__ out_count, uint64_t out_cap,
    uint64_t n_tiles, uint32_t skip) {
    using T = TileGeom<K, P, SK_BLOCK>;
    constexpr int TILE = T::TILE, LANE_RD = T::LANE_RD, IN_CHUNKS = T::IN_CHUNKS;
    constexpr bool STAGED = sk_staged(K);
    static_assert(P == 16, "lane runs of 16 positions");

    __shared__ __attribute__((aligned(16))) uint32_t s_in[IN_CHUNKS * 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_comp[STAGED ? IN_CHUNKS * 4 : 4];
    __shared__ unsigned int s_dirty;
    __shared__ uint64_t s_hash[REC_OUT_CAP];
    __shared__ uint64_t s_pos[REC_OUT_CAP];
    __shared__ unsigned int s_cnt;
    __shared__ unsigned long long s_base;

    const int tid = threadIdx.x;
    if (tid == 0) s_cnt = 0;

    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t base = tile * (uint64_t)TILE;
        if constexpr (STAGED) {
            if (tid == 0) s_dirty = 0;
        }
        __syncthreads();
        for (int c = tid; c < IN_CHUNKS; c += SK_BLOCK) {
            const uint64_t off = base + (uint64_t)c * 16;
            uint32_t w[4];
            load_chunk(seq, off, len, skip, w);
            if constexpr (STAGED) {
                uint32_t cw[4];
                if (stage_chunk(w, cw)) s_dirty = 1;
                *reinterpret_cast<uint4*>(&s_comp[c * 4]) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
            }
            *reinterpret_cast<uint4*>(&s_in[c * 4]) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        __syncthreads();
        uint32_t raw[LANE_RD];
        const uint4* wp = reinterpret_cast<const uint4*>(&s_in[tid * (P / 4)]);
#pragma unroll
        for (int i = 0; i < LANE_RD / 4; ++i) {
            const uint4 v = wp[i];
            raw[4 * i] = v.x; raw[4 * i + 1] = v.y; raw[4 * i + 2] = v.z; raw[4 * i + 3] = v.w;
        }
        auto emit = [&](int o, uint64_t h) {
            const unsigned int idx = atomicAdd(&s_cnt, 1u);
            // the position is made here, from the lane number behind a barrier the optimiser does not look through: otherwise the 16
            // positions of a lane are computed in front of the walk and stay live through it (20 VGPRs, a wave per SIMD at k = 31
            // and 51: profiles/singleton_kernel_resources.txt).  Valid k-mers never start in the prefix, so pos >= 0.
            const uint64_t pos = base + (uint64_t)(opaque(threadIdx.x) * P + (uint32_t)o) - skip;
            if (idx < (unsigned)REC_OUT_CAP) {
                s_hash[idx] = h;
                s_pos[idx] = pos;
            } else {  // dense output (scaled == 1 emits at every position): spill straight to HBM
                const unsigned long long g = atomicAdd(out_count, 1ull);
                if (g < out_cap) { out_hash[g] = h; out_pos[g] = pos; }
            }
        };
        if constexpr (STAGED) {
            uint32_t comp[LANE_RD];
            const uint4* cp = reinterpret_cast<const uint4*>(&s_comp[tid * (P / 4)]);
#pragma unroll
            for (int i = 0; i < LANE_RD / 4; ++i) {
                const uint4 v = cp[i];
                comp[4 * i] = v.x; comp[4 * i + 1] = v.y; comp[4 * i + 2] = v.z; comp[4 * i + 3] = v.w;
            }
            const bool dirty = __builtin_amdgcn_readfirstlane(s_dirty) != 0;
            process_lane_staged<K, P, true, sk_plain_mul(K, false)>(raw, comp, dirty, seed, thr, emit);
        } else {
            process_lane<K, P, true, sk_plain_mul(K, false)>(raw, seed, thr, emit);
        }
        // ---- flush the LDS buffer when it is at least half full: one global atomic per flush ----
        __syncthreads();
        const unsigned int cnt = s_cnt;
        if (cnt >= (unsigned)REC_OUT_CAP / 2) {
            const unsigned int n = cnt < (unsigned)REC_OUT_CAP ? cnt : (unsigned)REC_OUT_CAP;
            if (tid == 0) s_base = atomicAdd(out_count, (unsigned long long)n);
            __syncthreads();
            const unsigned long long b = s_base;
            for (unsigned int i = tid; i < n; i += SK_BLOCK)
                if (b + i < out_cap) { out_hash[b + i] = s_hash[i]; out_pos[b + i] = s_pos[i]; }
            __syncthreads();
            if (tid == 0) s_cnt = 0;
        }
    }
    __syncthreads();
    const unsigned int cnt = s_cnt;
    if (cnt) {
        const unsigned int n = cnt < (unsigned)REC_OUT_CAP ? cnt : (unsigned)REC_OUT_CAP;
        if (tid == 0) s_base = atomicAdd(out_count, (unsigned long long)n);
        __syncthreads();
        const unsigned long long b = s_base;
        for (unsigned int i = tid; i < n; i += SK_BLOCK)
            if (b + i < out_cap) { out_hash[b + i] = s_hash[i]; out_pos[b + i] = s_pos[i]; }
    }
}

typedef hipError_t (*records_launch_fn)(const uint8_t*, uint64_t, uint64_t, uint64_t, uint64_t*, uint64_t*, unsigned long long*, uint64_t,
                                        hipStream_t);

template <int K>
static hipError_t launch_records_k(const uint8_t* d_seq, uint64_t len, uint64_t seed, uint64_t thr, uint64_t* d_hash, uint64_t* d_pos,
                                   unsigned long long* d_count, uint64_t cap, hipStream_t stream) {
    constexpr uint64_t TILE = (uint64_t)SK_BLOCK * 16;
    const uint32_t skip = (uint32_t)((uintptr_t)d_seq & 15);
    d_seq -= skip;
    len += skip;
    const uint64_t n_tiles = (len + TILE - 1) / TILE;
    if (n_tiles == 0) return hipSuccess;
    const uint64_t max_blocks = 256ull * 8;                // the sketch kernel's grid rule
    const unsigned grid = (unsigned)(n_tiles < max_blocks ? n_tiles : max_blocks);
    hipLaunchKernelGGL((records_dna_kernel<K, 16>), dim3(grid), dim3(SK_BLOCK), 0, stream, d_seq, len, seed, thr, d_hash, d_pos,
                       d_count, cap, n_tiles, skip);
    return hipGetLastError();
}
template <int K0, int... KS>
static records_launch_fn records_launcher_from(uint32_t k, std::integer_sequence<int, KS...>) {
    static const records_launch_fn table[] = {&launch_records_k<K0 + KS + 1>...};
    return table[k - K0 - 1];
}
// sketch_records_k.hip, compiled as six parts of up to 16 ksizes each: k = 1 .. 16, ..., 81 .. 88
records_launch_fn records_launcher_0(uint32_t k);
records_launch_fn records_launcher_1(uint32_t k);
records_launch_fn records_launcher_2(uint32_t k);
records_launch_fn records_launcher_3(uint32_t k);
records_launch_fn records_launcher_4(uint32_t k);
records_launch_fn records_launcher_5(uint32_t k);
inline records_launch_fn records_launcher(uint32_t k) {
    switch ((k - 1u) / 16u) {
    case 0: return records_launcher_0(k);
    case 1: return records_launcher_1(k);
    case 2: return records_launcher_2(k);
    case 3: return records_launcher_3(k);
    case 4: return records_launcher_4(k);
    default: return records_launcher_5(k);
    }
}

}  // namespace smg
