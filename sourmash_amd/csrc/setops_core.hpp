// setops_core.hpp -- the rules of the set algebra on a CSR collection (setops.hip: merge by group, intersect, subtract) that can be
// stated without a GPU: the key form of the merge, its keep rule and num cut, the row offsets of its result, the membership rule of
// the row filter over a loaded value, and the position arithmetic of the ordered compaction; and for sets that carry abundances the
// value modes of the filter with their range test, the payload the summing merge sorts with, and the run sum taken from one scan.
// Compiled for the device by setops.hip and for the host by capi_setops.cpp, capi_abund_set.cpp, tests/native/setops_core_emul.cpp
// and tests/native/abund_set_core_emul.cpp.
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

constexpr uint32_t SETOPS_BLOCK = 256;              // lanes of a workgroup of every kernel of setops.hip: four waves of 64
constexpr uint32_t SETOPS_WAVES = SETOPS_BLOCK / 64;
// Row-wise filter: a partner row of up to this many hashes is staged in LDS (48 KiB: three workgroups, twelve waves, share a CU's
// 160 KiB); a longer one is searched where it lies, in global memory.
constexpr uint32_t SETOPS_LDS_PARTNER = 6144;
// Filter: a row longer than this is cut into pieces of this many hashes, each a work item of its own with its own base in the
// output, so that one very long row does not wait on one CU.  A multiple of SETOPS_BLOCK.
constexpr uint64_t SETOPS_SPLIT = 65536;
// Positions kept in 32 bits: the pairs of a merge are counted by the run-length pass in 32 bits, and the query index of the
// one-sketch filter addresses the other sketch in 32 bits.  Both bounds are checked by the C entries (capi_setops.cpp).
constexpr uint64_t SETOPS_MERGE_MAX_HASHES = 0xfffffffeull;
constexpr uint64_t SETOPS_OTHER_MAX_HASHES = 0xfffffffeull;
// what a run can find wrong beside a HIP error: a piece of the filter wrote another number of hashes than it had counted
enum SetopsTrouble : uint32_t { SETOPS_OK = 0, SETOPS_COUNT_MISMATCH = 1 };

// number of bits of x: 0 for 0, 64 for values with the top bit set
SMG_HD uint32_t setops_bits(uint64_t x) {
    uint32_t b = 0;
    while (b < 64 && (x >> b)) ++b;
    return b;
}

// ---- the key form of the merge ------------------------------------------------------------------------------------------------
// Every hash of the input becomes a (group, hash) pair; sorting the pairs and counting the runs of equal pairs says how many rows
// of a group hold a hash.  hbits: the bits of max_hash, 64 when max_hash == 0 (a num set; scaled = 1 has max_hash = 2^64 - 1 and
// 64 bits too).  gbits: the bits of n_groups - 1, at least 1.  When both fit 64 bits the pair is ONE key, (group << hbits) | hash,
// and one sort orders it; otherwise (wide) the pair stays two words and two stable sorts order it, by hash and then by group.
// No key and no hash value is special: hash 0 is a member like any other.
struct SetopsKeyForm {
    uint32_t hbits, gbits;
    bool packed;
};
SMG_HD SetopsKeyForm setops_key_form(uint64_t max_hash, uint64_t n_groups) {
    SetopsKeyForm f;
    f.hbits = max_hash == 0 ? 64u : setops_bits(max_hash);
    f.gbits = n_groups > 1 ? setops_bits(n_groups - 1) : 1u;
    if (f.gbits < 1) f.gbits = 1;
    f.packed = f.hbits + f.gbits <= 64;
    return f;
}
// (packed form only: hbits <= 63)
SMG_HD uint64_t setops_pack(const SetopsKeyForm& f, uint64_t group, uint64_t hash) { return (group << f.hbits) | hash; }
SMG_HD uint64_t setops_packed_hash(const SetopsKeyForm& f, uint64_t key) { return key & ((1ull << f.hbits) - 1ull); }

// the row that holds position i of the hashes: the last r in [0, n) with offsets[r] <= i (empty rows in front of i are passed over);
// i must lie in [offsets[0], offsets[n])
SMG_HD uint64_t setops_row_of(const uint64_t* offsets, uint64_t n, uint64_t i) {
    uint64_t lo = 0, hi = n;                        // first r with offsets[r] > i, minus one
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// ---- the keep rule --------------------------------------------------------------------------------------------------------------
// The count a hash of group g needs: the caller's need[g], or with need_all the number of rows of the group (the intersection).
SMG_HD uint32_t setops_need(const uint32_t* need, uint32_t need_all, const uint32_t* group_rows, uint64_t g) {
    return need_all ? group_rows[g] : (need ? need[g] : 1u);
}
// A run of `count` equal (group, hash) pairs stays when the count reaches the need.  (A run has at least one pair, so a need of 0
// keeps what a need of 1 keeps; a group of fewer rows than its need keeps nothing.)
SMG_HD bool setops_keep(uint64_t count, uint32_t need) { return count >= (uint64_t)need; }

// the num cut of a merged row (MinHash.merge on a num sketch keeps the num smallest of the union)
SMG_HD uint64_t setops_num_cut(uint64_t len, uint64_t num) { return num && len > num ? num : len; }

// Row offsets of the result: the kept runs are ordered by (group, hash); group g starts at the first kept run whose group is >= g.
// For g = 0 .. n_groups, so that groups without a kept run -- groups without rows among them -- get empty rows.
SMG_HD uint64_t setops_group_start(const uint32_t* kept_groups, uint64_t n_kept, uint64_t g) {
    uint64_t lo = 0, hi = n_kept;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)kept_groups[mid] < g) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- the filter's membership rule ---------------------------------------------------------------------------------------------
// Is x, a loaded hash of a row, a member of the other sketch?  other_n: its hashes; other_max: its largest (meaningless when it
// has none).  An empty sketch holds nothing, and a hash above its largest is absent WITHOUT a lookup: the query index may only be
// asked for x <= qmax (qindex.hpp: q_find), and a binary search need not be made.  `find(x)` is the lookup: true when found.
template <class Find>
SMG_HD bool setops_member(uint64_t x, uint64_t other_n, uint64_t other_max, const Find& find) {
    if (other_n == 0 || x > other_max) return false;
    return find(x);
}
// subtract keeps the absent hashes, intersect the present ones
SMG_HD bool setops_filter_keeps(bool present, bool keep_present) { return present == keep_present; }

// the lookup of the row-wise form: binary search in an ascending row
SMG_HD bool setops_search(const uint64_t* row, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (row[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && row[lo] == x;
}

// the same search with the answer a value mover needs: the position of x in the row, SETOPS_NOT_FOUND when the row does not hold it.
// One statement for both address spaces: the row-wise filter calls it on a partner staged in LDS and on one left in global memory.
constexpr uint64_t SETOPS_NOT_FOUND = ~0ull;
SMG_HD uint64_t setops_find(const uint64_t* row, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (row[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && row[lo] == x ? lo : SETOPS_NOT_FOUND;
}
// the membership rule with a position for an answer: no lookup in an empty sketch, none for x > other_max
template <class Find>
SMG_HD uint64_t setops_member_at(uint64_t x, uint64_t other_n, uint64_t other_max, const Find& find) {
    if (other_n == 0 || x > other_max) return SETOPS_NOT_FOUND;
    return find(x);
}

// ---- values that move with the hashes (abundance sets) --------------------------------------------------------------------------
// What the filter does with values.  NONE: a flat set, no value is read or written.  CARRY: a kept hash keeps the receiver's own
// abundance (subtract, intersect on an abundance set).  TAKE: a hash is kept when the other sketch holds it and takes the OTHER's
// abundance at the found position (inflate).  RANGE: no other sketch; a hash is kept when its own abundance lies in [lo, hi], and
// keeps it (sig filter).  Every stored abundance is >= 1 (MinHash.set_abundances drops zeros).
enum SetopsValueMode : uint32_t { SETOPS_VALUES_NONE = 0, SETOPS_VALUES_CARRY = 1, SETOPS_VALUES_TAKE = 2, SETOPS_VALUES_RANGE = 3 };
// the range test, inclusive at both ends; "no upper bound" is hi = 2^64 - 1; lo > hi keeps nothing
SMG_HD bool setops_in_range(uint64_t a, uint64_t lo, uint64_t hi) { return lo <= a && a <= hi; }
// the value a kept hash is written with: its own (`own`) or the other's at the found position (`taken`)
SMG_HD uint64_t setops_filter_value(uint32_t mode, uint64_t own, uint64_t taken) { return mode == SETOPS_VALUES_TAKE ? taken : own; }

// What the merge writes beside a kept hash.  SUM: the sum of the abundances of the group's rows that hold it, wrapping u64
// (KmerMinHash::merge).  COUNT: the number of those rows (the run's length).
enum SetopsMergeValues : uint32_t { SETOPS_MERGE_FLAT = 0, SETOPS_MERGE_SUM = 1, SETOPS_MERGE_COUNT = 2 };
// The sort's payload of a summing merge: the pair's group above j, the hash's position in the input (both fit 32 bits under
// SETOPS_MERGE_MAX_HASHES and the group limit).  The abundance of a sorted pair is abunds[base + j].
SMG_HD uint64_t setops_payload(uint64_t group, uint64_t j) { return (group << 32) | j; }
SMG_HD uint64_t setops_payload_group(uint64_t p) { return p >> 32; }
SMG_HD uint64_t setops_payload_pos(uint64_t p) { return p & 0xffffffffull; }
// A run's sum from ONE inclusive scan (wrapping u64, so exact modulo 2^64 and the same on every run) of the sorted pairs'
// abundances: the run covers the sorted pairs [start, start + count), start from the exclusive scan of the runs' counts.
SMG_HD uint64_t setops_run_sum(const uint64_t* scan, uint64_t start, uint64_t count) {
    return scan[start + count - 1] - (start ? scan[start - 1] : 0ull);
}
SMG_HD uint64_t setops_merge_value(uint32_t mode, uint64_t count, uint64_t sum) { return mode == SETOPS_MERGE_COUNT ? count : sum; }

// ---- pieces of the filter -------------------------------------------------------------------------------------------------------
// work items of a row of len hashes: one for an empty or short row, ceil(len / SETOPS_SPLIT) otherwise
SMG_HD uint64_t setops_pieces(uint64_t len) { return len <= SETOPS_SPLIT ? 1 : (len + SETOPS_SPLIT - 1) / SETOPS_SPLIT; }

// ---- the ordered compaction -----------------------------------------------------------------------------------------------------
// A chunk is SETOPS_BLOCK consecutive elements, one a lane; `mask` is the 64-bit ballot of the kept lanes of a wave.
// rank of a kept lane among the kept lanes of its wave
SMG_HD uint32_t setops_lane_rank(uint64_t mask, uint32_t lane) { return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull)); }
SMG_HD uint32_t setops_wave_total(uint64_t mask) { return (uint32_t)__builtin_popcountll(mask); }
// the wave's base in the chunk: the kept lanes of the waves in front of it
SMG_HD uint32_t setops_wave_base(const uint32_t* wave_totals, uint32_t wave) {
    uint32_t b = 0;
    for (uint32_t w = 0; w < SETOPS_WAVES; ++w) b += w < wave ? wave_totals[w] : 0u;
    return b;
}
SMG_HD uint32_t setops_chunk_total(const uint32_t* wave_totals) {
    uint32_t b = 0;
    for (uint32_t w = 0; w < SETOPS_WAVES; ++w) b += wave_totals[w];
    return b;
}
// where a kept element goes: base of its piece (or of all runs) in the output + what the chunks in front of its own kept
// (`running`) + the wave's base in the chunk + the lane's rank in the wave
SMG_HD uint64_t setops_out_pos(uint64_t base, uint64_t running, uint32_t wave_base, uint32_t lane_rank) {
    return base + running + wave_base + lane_rank;
}

}  // namespace smg
