// gather_many_core.hpp -- the rules of gather for many small queries at once (gather_many.hip) that can be stated without a GPU:
// the caps of the LDS form and which queries it takes, where a hash stands in a query, the key a round's arg-max reduces, the
// test-and-clear of the uncovered bitmap, the key the inverted lists are sorted by and where a position's list starts, and the
// ranges of queries a call is cut into.  Compiled for the device by gather_many.hip and for the host by capi_gather_many.cpp and
// tests/native/gather_many_core_emul.cpp.
#pragma once
#include <stdint.h>
#include "many_core.hpp"

#ifdef __HIPCC__
#define GM_UNROLL _Pragma("unroll")
#else
#define GM_UNROLL
#endif

namespace smg {

constexpr uint32_t GM_BLOCK = 256;                   // lanes of a workgroup of gm_rounds_kernel and gm_fill_kernel
// What a workgroup keeps in LDS for its query: one bit per query hash (uncovered or not) and one u32 counter per candidate row.
// The defaults: 16 KiB of bitmap + 32 KiB of counters; with the static words of the reduction that stays under GM_LDS_LIMIT, so
// two workgroups fit a CU's 160 KiB even at the caps.  A launch asks only for what its largest query needs.
constexpr uint32_t GM_MAX_QUERY_HASHES = 131072;
constexpr uint32_t GM_MAX_CANDIDATES = 8192;
constexpr uint32_t GM_LDS_LIMIT = 64 * 1024;         // static + dynamic LDS of gm_rounds_kernel, at the most
constexpr uint32_t GM_LDS_STATIC = 64;               // room kept for the kernel's static words (4 u64 of the reduction, the ticket)
constexpr uint32_t GM_NONE = 0xffffffffu;
constexpr uint64_t GM_BATCH_COMMON = 1ull << 25;     // forward-CSR entries of one batch (the sort space is 36 bytes an entry)
constexpr uint64_t GM_INDEX_LIMIT = 0xffffffffull;   // entries a batch may never reach: every index is u32

MANY_HD uint32_t gm_bitmap_words(uint32_t query_hashes) { return (query_hashes + 31u) / 32u; }
// dynamic LDS of a workgroup whose queries have at most query_hashes hashes and candidates candidates
MANY_HD uint64_t gm_lds_bytes(uint32_t query_hashes, uint32_t candidates) {
    return 4ull * gm_bitmap_words(query_hashes) + 4ull * candidates;
}
MANY_HD bool gm_caps_fit(uint32_t max_query_hashes, uint32_t max_candidates) {
    return gm_lds_bytes(max_query_hashes, max_candidates) + GM_LDS_STATIC <= GM_LDS_LIMIT;
}
// 0: the query runs in the LDS form; 1: it is left to the one-query path
MANY_HD uint32_t gm_status(uint64_t query_hashes, uint64_t candidates, uint32_t max_query_hashes, uint32_t max_candidates) {
    return query_hashes > max_query_hashes || candidates > max_candidates ? 1u : 0u;
}

// pos[k] = position of v[k] in the ascending Q[0, n), or GM_NONE, for U values at once.  A binary search whose number of steps
// depends on n alone, so that the U searches of a lane go in step: each step is U independent loads, not one (the fill walks a
// row of thousands of hashes and waits for nothing but these loads).
constexpr int GM_FILL_UNROLL = 8;                    // hashes a lane of gm_fill_kernel looks up side by side
template <int U>
MANY_HD void gm_find_group(const uint64_t* Q, uint32_t n, const uint64_t (&v)[U], uint32_t (&pos)[U]) {
    if (n == 0) {
        GM_UNROLL for (int k = 0; k < U; ++k) pos[k] = GM_NONE;
        return;
    }
    uint32_t base[U];
    GM_UNROLL for (int k = 0; k < U; ++k) base[k] = 0;
    for (uint32_t len = n; len > 1;) {                // the first entry >= v[k] lies in [base[k], base[k] + len]
        const uint32_t half = len >> 1;
        GM_UNROLL for (int k = 0; k < U; ++k) base[k] = Q[base[k] + half - 1] < v[k] ? base[k] + half : base[k];
        len -= half;
    }
    GM_UNROLL for (int k = 0; k < U; ++k) {
        const uint32_t at = base[k] + (Q[base[k]] < v[k] ? 1u : 0u);
        pos[k] = at < n && Q[at] == v[k] ? at : GM_NONE;
    }
}
// position of h in the ascending Q[0, n), or GM_NONE
MANY_HD uint32_t gm_find(const uint64_t* Q, uint32_t n, uint64_t h) {
    const uint64_t v[1] = {h};
    uint32_t pos[1];
    gm_find_group<1>(Q, n, v, pos);
    return pos[0];
}

// first of the ascending 32-bit values v[0, n) that is >= x (the first hit of a query among the hits ordered by query)
MANY_HD uint64_t gm_lower_bound32(const uint32_t* v, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The arg-max of a round reduces one key per candidate: the larger count wins, among equal counts the LOWER candidate (candidates
// stand in row order, so that is the lowest row).  A key whose count is 0 never wins against one that has a count.
MANY_HD uint64_t gm_pick_key(uint32_t count, uint32_t candidate) { return ((uint64_t)count << 32) | (uint32_t)~candidate; }
MANY_HD uint32_t gm_key_count(uint64_t key) { return (uint32_t)(key >> 32); }
MANY_HD uint32_t gm_key_candidate(uint64_t key) { return ~(uint32_t)key; }
// the loop ends when the best counter is 0 or below the threshold in hashes (search.py:15-37)
MANY_HD bool gm_stop(uint64_t best_key, uint64_t threshold_hashes) {
    const uint32_t c = gm_key_count(best_key);
    return c == 0 || (uint64_t)c < threshold_hashes;
}

// the uncovered set of a query of n hashes: bit p of word p / 32
MANY_HD uint32_t gm_bitmap_init_word(uint32_t word, uint32_t n) {
    const uint32_t lo = word * 32u;
    if (lo >= n) return 0u;
    return n - lo >= 32u ? 0xffffffffu : (1u << (n - lo)) - 1u;
}
MANY_HD uint32_t gm_bit(uint32_t pos) { return 1u << (pos & 31u); }
// (the device clears with an LDS atomicAnd and tests the value it returns; this is the same step on plain memory)
MANY_HD bool gm_test_and_clear(uint32_t* bitmap, uint32_t pos) {
    const uint32_t bit = gm_bit(pos), old = bitmap[pos >> 5];
    bitmap[pos >> 5] = old & ~bit;
    return (old & bit) != 0;
}

// The inverted lists are ONE stable sort of (key, candidate) pairs: key = the position of the query's first hash among the hashes
// of all queries of the call + the hash's position in its query.  The pairs of a query then stand together, in position order, and
// within a position in candidate order; the list of a position starts at the first pair with its key.
MANY_HD uint64_t gm_inv_key(uint64_t query_base, uint32_t pos) { return query_base + pos; }
MANY_HD uint32_t gm_inv_start(const uint64_t* keys, uint32_t lo, uint32_t hi, uint64_t key) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// significant bits of the largest key of a call whose queries hold q_span hashes in all (at least 1)
MANY_HD int gm_key_bits(uint64_t q_span) {
    int bits = 1;
    while (bits < 64 && (q_span >> bits) != 0) ++bits;
    return bits;
}

// Batches: queries are taken in contiguous ranges whose forward-CSR entries (the sum of `common` over the hits of the queries that
// run in the LDS form) stay under the budget; a range always takes at least one query.  -> the end of the range that starts at
// q_lo.  weight[q] = entries of query q (0 for a query left to the one-query path); a query of GM_INDEX_LIMIT entries or more
// never enters a range with another (the caller leaves it to the one-query path).
MANY_HD uint64_t gm_batch_end(const uint64_t* weight, uint64_t m, uint64_t q_lo, uint64_t budget) {
    uint64_t sum = 0, q = q_lo;
    while (q < m) {
        const uint64_t w = weight[q];
        if (q > q_lo && (sum + w >= budget || sum + w >= GM_INDEX_LIMIT)) break;
        sum += w;
        ++q;
    }
    return q;
}

}  // namespace smg
