// slice_walk_core.hpp -- the arithmetic of the flattened slice walk (slice_walk.hpp adds the wave's shuffles) over values already in
// registers, shared by the host and the device: plain C++ on the host (tests/native/slice_walk_emul.cpp compiles it with g++).
// EPW slices of lengths n[0 .. EPW) are walked as ONE list: slice l occupies the flattened positions [excl[l], incl[l]), incl the
// inclusive prefix sum of n and excl = incl - n; bound[k] = incl[k] for k < EPW - 1 is what every lane needs of it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SMG_UNROLL _Pragma("unroll")
#else
#define SMG_UNROLL
#endif
#ifndef SMG_HD
#if defined(__HIPCC__)
#define SMG_HD __host__ __device__ __forceinline__
#else
#define SMG_HD inline
#endif
#endif

namespace smg {

// flattened position t -> its slice: the number of slice ends it has passed.  Empty slices are stepped over (their end equals their
// start); a position at or past the total lands in the last slice.
template <int EPW>
SMG_HD int slice_of(uint32_t t, const uint32_t (&bound)[EPW - 1]) {
    int h = 0;
    SMG_UNROLL
    for (int k = 0; k < EPW - 1; ++k) h += t >= bound[k];
    return h;
}

// The step of 64 lanes that starts at flattened position t0: bit i set when lane i (position t0 + i) belongs to the slice
// [excl, incl), a contiguous run of lanes.  (A shift by 64 is not defined: runs that reach the step's end are taken apart.)
SMG_HD unsigned long long slice_step_mask(uint32_t excl, uint32_t incl, uint32_t t0) {
    const uint32_t a = excl > t0 ? (excl - t0 < 64u ? excl - t0 : 64u) : 0u;
    const uint32_t e = incl > t0 ? (incl - t0 < 64u ? incl - t0 : 64u) : 0u;
    const unsigned long long upto_e = e >= 64u ? ~0ull : ((1ull << e) - 1ull);
    const unsigned long long upto_a = a >= 64u ? ~0ull : ((1ull << a) - 1ull);
    return upto_e & ~upto_a;
}

}  // namespace smg
