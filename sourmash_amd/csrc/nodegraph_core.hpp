// nodegraph_core.hpp -- the two pieces of the Nodegraph (Bloom filter) arithmetic shared by the host container
// (nodegraph_host.hpp) and the GPU kernels (nodegraph_kernel.hpp): khmer's two-bit base codes and the reduction
// h mod size without a divide.  Plain C++ on the host (tests/native/nodegraph_mod_emul.cpp compiles it with g++).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef SMG_HD
#if defined(__HIPCC__)
#define SMG_HD __host__ __device__ __forceinline__
#else
#define SMG_HD inline
#endif
#endif

namespace smg {

constexpr uint32_t NG_MAX_K = 32;   // the longest k-mer of the bulk paths (khmer's limit: its two-bit word fills a u64)

// high 64 bits of a * b
SMG_HD uint64_t ng_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// The reciprocal of a table size d >= 1: m = floor((2^64 - 1) / d), computed once per table on the host.
inline uint64_t ng_magic(uint64_t d) { return d ? UINT64_MAX / d : 0; }

// h mod d for every u64 h and every 1 <= d < 2^63, with m = ng_magic(d).  The estimate q = mulhi(h, m) never exceeds
// floor(h / d) and falls short of it by at most 2 (h * m / 2^64 > h / d - h (d + 1) / (d 2^64) > h / d - 2 + 1/d), so
// r = h - q d (no wrap: q d <= h) needs at most two corrections.
SMG_HD uint64_t ng_mod(uint64_t h, uint64_t d, uint64_t m) {
    uint64_t r = h - ng_mulhi(h, m) * d;
    if (r >= d) r -= d;
    if (r >= d) r -= d;
    return r;
}

// khmer's two-bit code of a base, case folded (A 0, T 1, C 2, G 3; the complement's code is code ^ 1).  *ok = false for a
// byte outside ACGTacgt.  The bulk paths fold case; the single-k-mer host path (nodegraph_host.hpp) is strict, as khmer is.
SMG_HD uint32_t ng_code(uint32_t c, bool* ok) {
    const uint32_t up = c & 0xdfu;
    const uint32_t u = up - 0x41u;                          // 'A' -> 0, 'C' -> 2, 'G' -> 6, 'T' -> 19
    *ok = u < 20u && ((0x80045u >> u) & 1u);
    const uint32_t x = (up >> 1) & 3u;                      // A 0, C 1, G 3, T 2 (bits 1-2 of the ASCII code)
    return ((x & 1u) << 1) | (x >> 1);                      // swap the two bits: A 0, C 2, G 3, T 1
}

}  // namespace smg
