// slice_walk.hpp -- several short slices of an array walked by the 64 lanes of a wave as ONE list (device only; the arithmetic is
// slice_walk_core.hpp).  A wave per row would leave most lanes idle on rows of a few dozen elements; here lane l < EPW holds slice l
// as (absolute index of its first element, length), a prefix sum over those lanes places the slices one after the other, and every
// lane of a step takes one flattened position: its slice from the wave-uniform slice ends, the element's index from three shuffles.
// Users: the gather index build (gather_build.hip), the rounds' apply (gather.hip), the dictionary index (dictindex.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "slice_walk_core.hpp"

namespace smg {

// inclusive sum over the first WIDTH lanes of a wave (64: the whole wave); lanes from WIDTH on hold sums nobody reads
template <int WIDTH>
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, int lane) {
    static_assert(WIDTH >= 1 && WIDTH <= 64 && (WIDTH & (WIDTH - 1)) == 0, "");
#pragma unroll
    for (int d = 1; d < WIDTH; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

template <int EPW>
struct SliceGroup {
    uint32_t total;                 // elements of all slices together
    uint32_t incl, excl;            // lane l < EPW: end / start of slice l in the flattened list
    uint32_t lo_lo, lo_hi;          // lane l < EPW: absolute index of the slice's first element
    uint32_t bound[EPW - 1];        // wave-uniform: end of slices 0 .. EPW - 2

    // lane l < EPW brings slice l = [lo, lo + n), the other lanes n = 0; every lane of the wave calls it
    __device__ __forceinline__ void build(uint64_t lo, uint32_t n, int lane) {
        incl = wave_incl_sum<EPW>(n, lane);
        total = __shfl(incl, EPW - 1);
#pragma unroll
        for (int k = 0; k < EPW - 1; ++k) bound[k] = __shfl(incl, k);
        excl = incl - n;
        lo_lo = (uint32_t)lo;
        lo_hi = (uint32_t)(lo >> 32);
    }
    // flattened position t -> slice h and the element's absolute index (meaningful for t < total).  The shuffles read lanes
    // 0 .. EPW - 1: all lanes call it together, so a loop over t needs a wave-uniform trip count.
    __device__ __forceinline__ uint64_t at(uint32_t t, int& h) const {
        h = slice_of<EPW>(t, bound);
        const uint64_t start = ((uint64_t)(uint32_t)__shfl((int)lo_hi, h) << 32) | (uint32_t)__shfl((int)lo_lo, h);
        return start + (t - (uint32_t)__shfl((int)excl, h));
    }
    // lane l < EPW: how many lanes of `ballot`, taken over the step of 64 positions from t0, belong to slice l
    __device__ __forceinline__ uint32_t hits_of_step(unsigned long long ballot, uint32_t t0) const {
        return (uint32_t)__popcll(ballot & slice_step_mask(excl, incl, t0));
    }
};

}  // namespace smg
