// many_core.hpp -- the rules of the many-queries-against-a-collection pass (overlap_many.hip) that can be stated without a GPU:
// which part of a posting list belongs to a block of queries, where a row ends at the common scaled, the integer filter a search
// threshold turns into, and the key the hits are ordered by.  Compiled for the device by overlap_many.hip and for the host by
// capi_many.cpp and tests/native/many_core_emul.cpp.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MANY_HD __host__ __device__ inline
#else
#define MANY_HD inline
#endif

namespace smg {

constexpr uint32_t MANY_BLOCK = 256;            // lanes of a workgroup of many_overlap_kernel
// Counters a workgroup keeps in LDS (one u32 per query of the block): 16 KiB, so that the eight workgroups of 256 lanes a CU can
// hold (32 waves) keep 128 KiB of its 160 KiB and LDS never costs the kernel a wave.
constexpr uint32_t MANY_Q_BLOCK = 4096;
constexpr uint32_t MANY_Q_BLOCK_MAX = 8192;     // the most a caller may ask for (32 KiB: within the dynamic LDS a launch gets unasked)

// Both sets are taken at the coarser scaled (minhash.rs:539-548): only hashes <= min(max_hash_q, max_hash_db) count.
MANY_HD uint64_t many_cutoff(uint64_t max_hash_q, uint64_t max_hash_db) { return max_hash_q < max_hash_db ? max_hash_q : max_hash_db; }

// hashes of the ascending row[0, n) that are <= cutoff: where the row ends at the common scaled
MANY_HD uint64_t many_cut_len(const uint64_t* row, uint64_t n, uint64_t cutoff) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (row[mid] <= cutoff) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The postings post[*a, *b) of one hash hold ascending query numbers: narrow the range to the queries of [q_lo, q_hi).
MANY_HD void many_post_range(const uint32_t* post, uint32_t* a, uint32_t* b, uint32_t q_lo, uint32_t q_hi) {
    uint32_t lo = *a, hi = *b;
    if (lo >= hi) { *b = lo; return; }
    if (post[lo] >= q_lo && post[hi - 1] < q_hi) return;                // the whole list (always, when one block holds every query)
    uint32_t l = lo, h = hi;
    while (l < h) {                                                      // first posting >= q_lo
        const uint32_t mid = l + ((h - l) >> 1);
        if (post[mid] < q_lo) l = mid + 1; else h = mid;
    }
    *a = l;
    h = hi;
    while (l < h) {                                                      // first posting >= q_hi
        const uint32_t mid = l + ((h - l) >> 1);
        if (post[mid] < q_hi) l = mid + 1; else h = mid;
    }
    *b = l;
}

// The parameters two sets must share, checked in the reference's order (check_compatible, minhash.rs:886-912): ksize, hash function,
// max_hash only when a side is a num sketch, then seed; num sets are refused behind that, as prefetch refuses them.  -> 0, or the
// reference's error code (include/sourmash_amd.h: SOURMASH_ERROR_CODE_MISMATCH_*).
struct ManyParams {
    uint32_t ksize, hash_function;
    uint64_t seed, max_hash, num;
};
MANY_HD uint32_t many_compat_code(const ManyParams& a, const ManyParams& b) {
    if (a.ksize != b.ksize) return 101;                                  // MISMATCH_K_SIZES
    if (a.hash_function != b.hash_function) return 102;                  // MISMATCH_DNA_PROT
    if ((a.num || b.num) && a.max_hash != b.max_hash) return 103;        // MISMATCH_SCALED
    if (a.seed != b.seed) return 104;                                    // MISMATCH_SEED
    if (a.num || b.num || !a.max_hash || !b.max_hash) return 107;        // MISMATCH_NUM: the pass takes scaled sketches
    return 0;
}

// hits leave ordered by (query, row)
MANY_HD uint64_t many_key(uint32_t query, uint32_t row) { return ((uint64_t)query << 32) | row; }
MANY_HD uint32_t many_key_query(uint64_t key) { return (uint32_t)(key >> 32); }
MANY_HD uint32_t many_key_row(uint64_t key) { return (uint32_t)key; }

// The device's filter for a search at `threshold` over a query of n_q hashes: a count below the returned value cannot pass the
// float test of the scoring (index.py: score_hits), whatever the row.  Conservative: the bound is rounded down and lowered by
// one more, so that no rounding of the float score can lose a hit; the exact test stays the host's.  Never 0 (a pair sharing
// nothing is never a hit).
//   mode 0 Jaccard:          c / (n_q + n_r - c) >= t  implies  c >= t n_q / (1 + t)    (n_r >= c)
//   mode 1 containment:      c / n_q >= t              implies  c >= t n_q
//   mode 2 max containment:  c / min(n_q, n_r) >= t    says nothing without n_r: 1
enum ManyMode : uint32_t { MANY_JACCARD = 0, MANY_CONTAINMENT = 1, MANY_MAX_CONTAINMENT = 2 };
MANY_HD uint32_t many_need(uint32_t mode, double threshold, uint64_t n_q) {
    if (mode == MANY_MAX_CONTAINMENT || !(threshold > 0.0)) return 1;   // (NaN lands here too)
    double bound = threshold * (double)n_q;
    if (mode == MANY_JACCARD) bound /= 1.0 + threshold;
    bound = floor(bound) - 1.0;
    if (!(bound > 1.0)) return 1;
    return bound >= 4294967295.0 ? 0xffffffffu : (uint32_t)bound;
}

}  // namespace smg
