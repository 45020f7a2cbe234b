// gather_rows_core.hpp -- the rules of the pass that turns the picks of gather into the integers of its result rows
// (gather_rows.hip) that can be stated without a GPU: who owns a query hash, the key the (pick, abundance) pairs are sorted by,
// which query or pick a position of a flat array belongs to, and how the workspace is cut.  Compiled for the device by
// gather_rows.hip and for the host by capi_gather_rows.cpp and tests/native/gather_rows_core_emul.cpp.
//
// The picks of query q are pick_rows[pick_offsets[q], pick_offsets[q + 1]) in rank order.  The OWNER of a query hash is the lowest
// rank among the query's picks whose row holds it, or none: the reference removes the whole match from the query every round
// (search.py:915-919), so "remaining query ∩ match" of a round is exactly the hashes the round's pick owns.
#pragma once
#include <stdint.h>
#include "gather_many_core.hpp"

namespace smg {

constexpr uint32_t GR_BLOCK = 256;                   // lanes of a workgroup of gr_owner_kernel and gr_tally_kernel
constexpr uint64_t GR_ALIGN = 256;                   // granule of the workspace

// ---- the owner: a u32 per query hash, preset to GM_NONE, lowered to the rank of every pick that holds the hash
MANY_HD uint32_t gr_owner_merge(uint32_t owner, uint32_t rank) { return rank < owner ? rank : owner; }   // (atomicMin on the device)
MANY_HD bool gr_owned(uint32_t owner) { return owner != GM_NONE; }

// ---- the segment a position of a flat array belongs to: the last s of [0, m) with offsets[s] <= i, for offsets[0] <= i <
// offsets[m] and ascending offsets (empty segments are stepped over).  Whatever the offsets hold, the answer lies in [0, m).
MANY_HD uint32_t gr_segment_of(const uint64_t* offsets, uint64_t m, uint64_t i) {
    uint64_t lo = 0, hi = m;                          // the first s of (0, m] with offsets[s] > i lies in (lo, hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return (uint32_t)lo;
}

// ---- the pairs: one per owned hash, key = (pick among all picks of the call, position of the hash in its query), value = the
// abundance.  Sorted by the key they stand pick by pick, within a pick in ascending hash order -- whatever order they were emitted
// in and whether or not the sort is stable.
MANY_HD uint64_t gr_pair_key(uint32_t pick, uint32_t pos) { return ((uint64_t)pick << 32) | pos; }
MANY_HD uint32_t gr_key_pick(uint64_t key) { return (uint32_t)(key >> 32); }
MANY_HD uint32_t gr_key_pos(uint64_t key) { return (uint32_t)key; }
// significant bits of the largest key of a call with n_picks picks
MANY_HD int gr_key_bits(uint64_t n_picks) { return 32 + gm_key_bits(n_picks ? n_picks : 1); }

// ---- what a call refuses: every index is u32, and GM_NONE is no rank
MANY_HD bool gr_sizes_fit(uint64_t m, uint64_t q_total, uint64_t n_rows, uint64_t n_picks) {
    return m < GM_INDEX_LIMIT && q_total < GM_INDEX_LIMIT && n_rows < GM_INDEX_LIMIT && n_picks < GM_INDEX_LIMIT;
}
// bits of the trouble word the kernels raise
constexpr uint32_t GR_BAD_QUERY_OFFSETS = 1, GR_BAD_PICK_OFFSETS = 2, GR_BAD_PICK_ROW = 4, GR_BAD_ROW_OFFSETS = 8;

// ---- the workspace, cut in granules: the hashes <= cutoff of every query, the scalars (tickets, trouble, pairs emitted), the
// widened unique counts and the scan's scratch, then the pairs before and (the keys) after the sort and the sort's scratch.
// scan_bytes / sort_bytes are what the device library asks for n_picks + 1 and q_total elements.
MANY_HD uint64_t gr_al(uint64_t bytes) { return (bytes + GR_ALIGN - 1) / GR_ALIGN * GR_ALIGN; }
struct GrLayout {
    uint64_t qn, scal, wide, scan, keys_a, vals_a, keys_b, sort, end;
};
MANY_HD GrLayout gr_layout(uint64_t m, uint64_t q_total, uint64_t n_picks, uint64_t scan_bytes, uint64_t sort_bytes) {
    GrLayout L;
    uint64_t at = 0;
    L.qn = at; at += gr_al((m + 1) * 4);
    L.scal = at; at += gr_al(256);
    L.wide = at; at += gr_al((n_picks + 2) * 8);
    L.scan = at; at += gr_al(scan_bytes);
    L.keys_a = at; at += gr_al((q_total + 1) * 8);
    L.vals_a = at; at += gr_al((q_total + 1) * 8);
    L.keys_b = at; at += gr_al((q_total + 1) * 8);
    L.sort = at; at += gr_al(sort_bytes);
    L.end = at + GR_ALIGN;
    return L;
}

}  // namespace smg
