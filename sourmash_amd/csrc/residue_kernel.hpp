// residue_kernel.hpp -- what the two residue window kernels share (window_fast_kernel in protein.hip, window_pairs_kernel in
// protein_records.hip): the size convention, the lanes and the grid, and the round loop over residue_windows_lane
// (residue_core.hpp) with LdsSink (kmer_core.hpp) behind it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_api.hpp"
#include "kmer_core.hpp"
#include "residue_core.hpp"

namespace smg {

constexpr int RW_BLOCK = 256;

// n, the bytes of the residue buffer: the host's value, or *d_n when d_n is given (a size that is known on the device only; the
// host's value is then an upper bound, for the grid)
__device__ __forceinline__ uint64_t residue_n(uint64_t n_host, const uint64_t* d_n) { return d_n ? *d_n : n_host; }

// lanes that own at least one window start of aa[0, n)
SMG_HD uint64_t residue_lanes(uint64_t n, uint32_t k) { return n >= (uint64_t)k ? (n - k + 1 + RW_P - 1) / RW_P : 0; }

inline unsigned residue_grid(uint64_t n_bound, uint32_t k) { return grid_for(residue_lanes(n_bound, k), RW_BLOCK, 256 * 8); }

// Rounds of gridDim.x * RW_BLOCK lanes over the windows of aa[0, n): emit(window start, hash) as residue_windows_lane<NB, SEP>
// calls it, then round_end() by every thread of the workgroup (the trip count is uniform, so it may hold barriers).
template <int NB, bool SEP, class Emit, class RoundEnd>
__device__ __forceinline__ void residue_rounds(const uint64_t* __restrict__ aa64, uint64_t n, const ResidueTail& t, uint64_t seed, Emit&& emit,
                                               RoundEnd&& round_end) {
    const uint64_t n_lanes = residue_lanes(n, t.k);
    const uint64_t rounds = (n_lanes + (uint64_t)gridDim.x * RW_BLOCK - 1) / ((uint64_t)gridDim.x * RW_BLOCK);
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t g = (r * gridDim.x + blockIdx.x) * RW_BLOCK + threadIdx.x;
        if (g < n_lanes) residue_windows_lane<NB, SEP>(aa64, n, g, t, seed, emit);
        round_end();
    }
}

// The rounds with every kept hash (1 <= h <= thr) appended to the sink -- alone (NV = 1) or with its window start (NV = 2) --
// and the sink flushed at CAP / 2 entries between rounds and at 1 behind the last.  The kernel has zeroed the sink's counter in
// front of a barrier.  A round ends with two barriers: one between its appends and the flush's read of the counter, and one
// behind the flush, since LdsSink::flush resets the counter after its own last barrier and the next round appends at once.
template <int NB, bool SEP, int CAP, int NV>
__device__ __forceinline__ void residue_rounds_kept(const uint64_t* __restrict__ aa64, uint64_t n, const ResidueTail& t, uint64_t seed, uint64_t thr,
                                                    const LdsSink<CAP, RW_BLOCK, NV>& sink) {
    residue_rounds<NB, SEP>(
        aa64, n, t, seed,
        [&](uint64_t start, uint64_t h) {
            if ((h - 1) < thr) {
                if constexpr (NV == 1) sink.append(h);
                else sink.append(h, start);
            }
        },
        [&] {
            __syncthreads();
            sink.flush(CAP / 2);
            __syncthreads();
        });
    sink.flush(1);
}

}  // namespace smg
