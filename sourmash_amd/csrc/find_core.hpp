// find_core.hpp -- membership in a query sketch, the one rule of k-mer finding (sketch_find.hip, find_kernel.hpp) that the host
// and the device share.  Plain C++ on the host (tests/native/find_core_emul.cpp compiles it with g++).
//
// The query is its sorted distinct hashes q[0 .. n) (1 <= q[i] <= max_hash) and a bucket directory dir[0 .. nb + 1) over the top
// bits of the hash space: bucket b holds the hashes with q[i] >> shift == b, dir[b] is the first index with q[i] >> shift >= b
// and dir[nb] == n.  With about one bucket per hash a uniformly spread query has at most one hash per bucket on average and a
// probe is one directory read and one or two reads of q; a clustered query -- thousands of hashes in one bucket -- costs the
// logarithm of the bucket, never its length.
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

constexpr uint64_t FIND_MAX_BUCKETS = (uint64_t)1 << 24;   // 64 MiB of directory at the most
constexpr uint64_t FIND_MAX_QUERY = 0xfffffffeull;         // the directory holds 32-bit indices

// buckets of the directory for this shift: every hash 0 .. max_hash has one
SMG_HD uint64_t find_dir_buckets(uint64_t max_hash, uint32_t shift) { return (max_hash >> shift) + 1; }

// The shift of a query of n hashes: the largest one that leaves at least n buckets -- so the bucket count is the smallest value
// >= n the shifts offer, below 2 n -- and never more than FIND_MAX_BUCKETS of them.  n == 0 counts as 1.
SMG_HD uint32_t find_dir_shift(uint64_t n, uint64_t max_hash) {
    if (n == 0) n = 1;
    uint32_t shift = 0;
    while (shift < 63 && find_dir_buckets(max_hash, shift + 1) >= n) ++shift;
    while (shift < 63 && find_dir_buckets(max_hash, shift) > FIND_MAX_BUCKETS) ++shift;
    return shift;
}

// dir[b] for one bucket boundary b in 0 .. nb: the first index i with q[i] >> shift >= b (n where there is none)
SMG_HD uint32_t find_dir_entry(const uint64_t* q, uint64_t n, uint32_t shift, uint64_t b) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((q[mid] >> shift) < b) lo = mid + 1; else hi = mid;
    }
    return (uint32_t)lo;
}

// Whether h is one of q: never for h == 0 or h > max_hash, which are not looked up at all (no bucket is theirs).
SMG_HD bool find_member(const uint64_t* q, const uint32_t* dir, uint32_t shift, uint64_t max_hash, uint64_t h) {
    if (h - 1 >= max_hash) return false;
    const uint64_t b = h >> shift;
    uint32_t lo = dir[b], hi = dir[b + 1];
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint64_t v = q[mid];
        if (v == h) return true;
        if (v < h) lo = mid + 1; else hi = mid;
    }
    return false;
}

// the query as the kernels take it: q and dir on the device, the sketch's max_hash, the directory's shift
struct FindQuery {
    const uint64_t* q;
    const uint32_t* dir;
    uint64_t max_hash;
    uint32_t shift;
};

}  // namespace smg
