// compare_core.hpp -- the rules of the all-pairs compare family that can be stated without a GPU, each of them once: the lower
// bound every unit searches with; the hash-range slices of a heavy tile and the lock-step rounds of compare_hash_kernel (compare.hip)
// and compare_ext_kernel (compare_ext.hip); the table arithmetic of compare_hash_kernel; the walks of compare_ext_kernel and the
// sizes made from their counts; the list, slice, chunk, search and worklist arithmetic of abund_pairs.hip; and the cost model that
// picks the engine of a compare() (capi_compare.cpp: bitindex_build).
// Compiled for the device by compare.hip, compare_ext.hip, abund_pairs.hip, pair_ops.hip and bitindex.hip, and for the host by
// capi_compare.cpp and tests/native/compare_core_emul.cpp, which walks whole collections with these functions alone.
#pragma once
#include <stdint.h>
#include "smg_hd.hpp"

namespace smg {

// ---- the search ---------------------------------------------------------------------------------------------------------------
// first index in [lo, hi) of the sorted a whose value is not below x; hi when there is none.  (Searches that order by a second
// key as well -- ap_slice_kernel's (hash, row), the offsets[mid] <= i of other families -- are written where they are used.)
SMG_HD uint64_t lower_bound_u64(const uint64_t* __restrict__ a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// ... with 32-bit positions: rows and LDS copies shorter than 2^32
SMG_HD uint32_t lower_bound_u64(const uint64_t* a, uint32_t lo, uint32_t hi, uint64_t x) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- tile geometry --------------------------------------------------------------------------------------------------------------
// (in namespaces of their own: the units that only search or price a path see none of these short names; compare.hip and
//  compare_ext.hip say `using namespace cmp_tile`, abund_pairs.hip `using namespace ap_geom`)
namespace cmp_tile {
constexpr int CT = 16;            // compare.hip: tile edge (sketches)
constexpr int CMP_ZMAX = 16;      // hash-range slices per tile at most; a tile uses cmp_slice_count of them
constexpr int HR = CT;            // row sketches of a tile (inserted)
constexpr int HC = 32;            // column sketches of a tile (looked up)
constexpr int HSEG = 64;          // hashes staged per sketch and round: one per lane
constexpr unsigned long long H_EMPTY = ~0ull;   // never a key: a staged hash equal to 2^64 - 1 is counted out of band
constexpr int HWAVES = 8;         // waves per workgroup: sketch s = i * HWAVES + wave, so every wave holds HR / 8 rows
constexpr int HBLOCK = HWAVES * 64;
constexpr int HPW = (HR + HC) / HWAVES;   // sketches per wave
constexpr int NR = HR / HWAVES;   // row sketches per wave
constexpr int NC = HC / HWAVES;   // column sketches per wave
static_assert(HR % HWAVES == 0 && HC % HWAVES == 0, "");
static_assert(HR == 16 && NC == 4 && HC == 32, "the packed counters hold 16 rows x 4 columns per wave");

constexpr int XT = 16;                 // compare_ext.hip: tile edge (sketches)
constexpr int XSEG = 64;               // hashes staged per sketch and round
constexpr int XZMAX = 16;              // hash-range slices a tile of abundance sketches can be cut into (grid.z)
constexpr uint32_t XSLICE = 6144;      // hashes of the tile's longest sketch per slice: ordinary sketches (~5,000) are never cut
constexpr uint32_t XSLICE_SMALL = 1700;   // ... for small grids (cmp_ext_slice_len)
}  // namespace cmp_tile

// ---- the slice rule: compare_plan_kernel + compare_hash_kernel, compare_ext_kernel ----------------------------------------------
// A tile that holds an unusually long sketch is cut into zt hash ranges, each a work item of its own.  The LONGEST sketch of the
// tile decides -- the FIRST longest on a tie: compare_hash_kernel scans with a strict `>` (cmp_longest_first), compare_ext_kernel
// takes the lowest set bit of the ballot of the lanes that hold the maximum.  The pivots are values of that sketch at equal
// steps, and slice z of every sketch is its part between two lower bounds: [piv(z), piv(z + 1)), the first from the row's start,
// the last to its end.  A hash equal to a pivot belongs to the slice the pivot opens, in every sketch: counted once.
SMG_HD uint32_t cmp_slice_count(uint64_t longest, uint32_t slice_len, uint32_t zmax) {
    const uint32_t zt = (uint32_t)((longest + slice_len - 1) / slice_len);
    return zt < 1 ? 1 : (zt > zmax ? zmax : zt);
}
SMG_HD uint64_t cmp_slice_pivot_at(uint64_t best_pos, uint64_t best_len, uint32_t z, uint32_t zt) {
    return best_pos + (uint64_t)z * best_len / zt;
}
// the two pivot VALUES of slice z (0 and 2^64 - 1 stand for the open ends and are never searched for)
SMG_HD void cmp_slice_pivots(const uint64_t* __restrict__ hashes, uint64_t best_pos, uint64_t best_len, uint32_t z, uint32_t zt,
                             uint64_t* piv_lo, uint64_t* piv_hi) {
    *piv_lo = z == 0 ? 0ull : hashes[cmp_slice_pivot_at(best_pos, best_len, z, zt)];
    *piv_hi = z + 1 == zt ? ~0ull : hashes[cmp_slice_pivot_at(best_pos, best_len, z + 1, zt)];
}
SMG_HD void cmp_slice_cut(const uint64_t* __restrict__ hashes, uint64_t lo, uint64_t hi, uint32_t z, uint32_t zt, uint64_t piv_lo,
                          uint64_t piv_hi, uint64_t* a, uint64_t* b) {
    *a = z == 0 ? lo : lower_bound_u64(hashes, lo, hi, piv_lo);
    *b = z + 1 == zt ? hi : lower_bound_u64(hashes, *a, hi, piv_hi);
}
// the first longest of n sketches [pos[i], end[i])
SMG_HD void cmp_longest_first(const uint64_t* pos, const uint64_t* end, int n, uint64_t* best_pos, uint64_t* best_len) {
    *best_len = 0; *best_pos = 0;
    for (int i = 0; i < n; ++i) {
        const uint64_t len = end[i] - pos[i];
        if (len > *best_len) { *best_len = len; *best_pos = pos[i]; }
    }
}
// compare.hip's slice length: long enough that ordinary sketches (a few thousand hashes) are never cut when there are plenty of
// tiles, shorter when the tile count alone cannot fill 256 CUs x 4 workgroups.
SMG_HD uint32_t cmp_pick_slice_len(uint64_t n_tiles) {
    if (n_tiles >= 2048) return 8192;
    if (n_tiles >= 512) return 2048;
    return 1024;
}
// compare_ext.hip's: tiles of ordinary sketches are cut as well when the grid is small -- a 1,000-sketch collection is 2,016 tiles
// on 1,536 resident workgroups (two rounds, the second a third full); three slices per tile fill the rounds (5.83 -> 5.47 ms at C3)
SMG_HD uint32_t cmp_ext_slice_len(uint32_t tiles) { return tiles >= 16384 ? cmp_tile::XSLICE : cmp_tile::XSLICE_SMALL; }

// ---- the round rule: compare_hash_kernel, compare_ext_kernel --------------------------------------------------------------------
// Every sketch of a tile stages its next <= seg hashes.  A sketch with MORE to come than it has staged bounds the round with its
// seg-th staged hash; the round's bound hi is the smallest of those, 2^64 - 1 when there is none.  A sketch gives up (`take`) its
// staged hashes at or under the bound, so every sketch's hashes <= hi are among what the round consumes.  The round goes ahead
// while some row AND some column has data left.
SMG_HD bool cmp_round_bounds(uint32_t left, uint32_t seg) { return left > seg; }
constexpr uint32_t CMP_LIVE_ROWS = 1u, CMP_LIVE_COLS = 2u;
SMG_HD bool cmp_round_live(uint32_t live_bits) { return live_bits == (CMP_LIVE_ROWS | CMP_LIVE_COLS); }
SMG_HD bool cmp_round_live(uint32_t rows_with_data, uint32_t cols_with_data) { return rows_with_data != 0 && cols_with_data != 0; }
// compare_hash_kernel keeps 2^64 - 1 out of its table (H_EMPTY).  hi == 2^64 - 1 only when no sketch has more than it has staged:
// that LAST round takes everything left and is the only one that can meet the hash 2^64 - 1, which it counts out of band; the
// table sees the hashes at or under the cut.
SMG_HD bool cmp_round_last(uint64_t hi) { return hi == ~0ull; }
SMG_HD uint64_t cmp_round_cut(uint64_t hi) { return hi == ~0ull ? ~0ull - 1 : hi; }
SMG_HD uint32_t cmp_round_take(bool last, uint32_t left, uint32_t staged_at_or_under_cut) { return last ? left : staged_at_or_under_cut; }

// ---- the table of compare_hash_kernel -------------------------------------------------------------------------------------------
// 2^LOGT slots of 8 bytes addressed by BYTE offsets; a 16-bit row mask per slot, two to a 32-bit word.
template <int LOGT>
SMG_HD uint32_t pair_slot(uint64_t v) {           // the even slot a hash's probe sequence starts on
    // the hashes of a round share their top bits (a narrow value range), so the slot comes from the low word folded with
    // the high one; shifts and xors only -- a 32-bit multiply costs four of them on this VALU
    uint32_t x = (uint32_t)v ^ (uint32_t)(v >> 32);
    x ^= x >> 15;
    return (x & (uint32_t)((1 << (LOGT - 1)) - 1)) << 1;
}
// the byte offset `step` bytes on, wrapping: 8 for an insert's next slot, 16 for a lookup's next pair
template <int LOGT>
SMG_HD uint32_t cmp_probe_next(uint32_t off, uint32_t step) { return (off + step) & (uint32_t)((8 << LOGT) - 1); }
// slot at byte offset off -> its mask: half (slot & 1) of word slot >> 1, i.e. 16-bit cell slot
SMG_HD uint32_t cmp_mask_word(uint32_t off) { return off >> 4; }
SMG_HD uint32_t cmp_mask_shift(uint32_t off) { return (off & 8u) << 1; }
SMG_HD uint32_t cmp_mask_half(uint32_t off) { return off >> 3; }
// The per-lane 4-bit counters of a wave: acc[p][k] nibble j counts bit t = 4j + k of y_p = m[2p] | m[2p+1] << 16, i.e. row t & 15
// of column j' = 2p + (t >> 4) of this wave (tile column 8j' + wave).  A flush splits even and odd nibbles (half = j & 1) into
// byte lanes (byte = j >> 1): byte `byte` of (p, k, half) lands in the cell of row 8 (byte & 1) + 4 half + k, column
// 8 (2p + (byte >> 1)) + wave of the tile's HR x HC counters.
// The cell is the sum of a part that a lane and its wave fix (the kernel keeps it as a pointer) and a part per register and half.
SMG_HD int cmp_nibble_cell_of_lane(int byte, int wave) { return (8 * (byte & 1)) * cmp_tile::HC + (byte >> 1) * cmp_tile::HWAVES + wave; }
SMG_HD int cmp_nibble_cell_of_reg(int p, int k, int half) { return (4 * half + k) * cmp_tile::HC + 2 * cmp_tile::HWAVES * p; }
SMG_HD int cmp_nibble_cell(int p, int k, int half, int byte, int wave) {
    return cmp_nibble_cell_of_lane(byte, wave) + cmp_nibble_cell_of_reg(p, k, half);
}

// ---- the walks of compare_ext_kernel over two staged prefixes A[0 .. na), B[0 .. nb) (what the round takes) ---------------------
// Bottom-k: one step consumes exactly one element of A ∪ B in ascending order, so the intersection with the merged sketch
// truncated to `cap` is the equal heads met during the first cap steps (counted across rounds); what one side has left below the
// round's bound are union elements too, none common.
SMG_HD void ext_num_walk(const uint64_t* A, uint32_t na, const uint64_t* B, uint32_t nb, uint32_t cap, uint32_t* cnt, uint32_t* steps) {
    uint32_t ia = 0, ib = 0;
    while (ia < na && ib < nb && *steps < cap) {
        const uint64_t a = A[ia], b = B[ib];
        const bool lt = a < b, gt = b < a;
        *cnt += !(lt | gt);
        ia += !gt;
        ib += !lt;
        ++*steps;
    }
    *steps += (na - ia) + (nb - ib);
}
// Abundance: one step of the two-pointer walk with the heads' hashes and abundances; equal heads add 1 and wa * wb (u64, wrapping).
// No branch: with 64 walks per wave some lane meets a common hash at almost every step anyway.
template <typename AbT>
SMG_HD void ext_abund_step(uint64_t a, uint64_t b, AbT wa, AbT wb, uint32_t* ia, uint32_t* ib, uint32_t* cnt, unsigned long long* acc) {
    const bool lt = a < b, gt = b < a, eq = !(lt | gt);
    *cnt += eq;
    *acc += (unsigned long long)wa * (unsigned long long)(eq ? wb : (AbT)0);   // AbT = u32: select + one v_mad_u64_u32
    *ia += !gt;
    *ib += !lt;
}
// bottom-k: |merged| = min(num of the pair, n_i + n_j - common); a sketch with itself: its own size
SMG_HD uint64_t num_union_size(uint64_t ni, uint64_t nj, uint64_t common, uint32_t num, bool diagonal) {
    uint64_t u = ni + nj - common;
    if (diagonal) u = ni;
    if (u > num) u = num;
    return u;
}
// common / max(1, size): one IEEE divide (minhash.rs:624-631)
SMG_HD double jaccard_of(uint64_t common, uint64_t size) { return (double)common / (double)(size > 1 ? size : 1); }
SMG_HD double jaccard_scaled(uint64_t common, uint64_t ni, uint64_t nj) { return jaccard_of(common, ni + nj - common); }

// (ap_join_kernel keeps its own inline copies of ap_tile_of, ap_slice_bounds, ap_trim_to_runs, ap_find, ap_run_len and
//  ap_work_pack / ap_work_unpack, compare_ext_kernel<X_NUM> of ext_num_walk, compare_hash_kernel of cmp_round_take, cmp_longest_first,
//  cmp_slice_pivots, cmp_slice_cut and cmp_nibble_cell_of_lane: as calls they changed those kernels' instructions.  Of
//  these the functions here are what tests/native/compare_core_emul.cpp walks; the kernels' copies are held to them by
//  tests/test_gpu_compare_edges.py, not by the CPU suite.  A change to one side must be made on the other.)
// ---- abund_pairs.hip --------------------------------------------------------------------------------------------------------------
namespace ap_geom {
constexpr int AP_T = 64;                 // sketches per block = tile edge
constexpr int AP_TS = AP_T + 1;          // row stride of the tile's accumulators in LDS: a hash shared by a whole block puts the 64
                                         // lanes of a wave on 64 different rows and ONE column -- at a stride of 64 that is one bank
constexpr int AP_THREADS = 1024;
constexpr int AP_CHUNK = 4096;           // entries of list B staged per round (64 KB of hashes + payloads)
constexpr int AP_ZMAX = 16;              // hash slices per tile at most
#ifndef AP_INLINE_N
#define AP_INLINE_N 16
#endif
constexpr int AP_INLINE = AP_INLINE_N;   // an entry of list A that meets at most this many entries of B adds its products itself
constexpr int AP_G = 16;                 // lanes that share a longer run
constexpr int SM_CAP = 2048;             // entries of a (block, slice) merged in LDS
constexpr int SM_BUCKETS = 2048;         // sub-buckets of a slice
constexpr int SM_BUCKET_BITS = 11;
constexpr int SM_THREADS = 256;
constexpr int SM_TARGET = 640;           // entries per (block, slice) aimed at; the shift lands between this and twice this
static_assert(AP_CHUNK <= 4096 && AP_T <= 64, "a worklist word holds a 12-bit run start, a 7-bit length and a 6-bit row");
static_assert((AP_CHUNK & (AP_CHUNK - 1)) == 0 && AP_T == 64, "the searches halve a power of two");
static_assert(AP_THREADS == 1024 && AP_G == 16, "the list walk deals 64 groups of 16 lanes, four to a wave");
}  // namespace ap_geom

// The lists: the hash space is cut into n_slices equal slices, slice s = hash >> shift, at most s_max of them.
struct ApPlan { uint32_t shift, n_slices; };
SMG_HD uint32_t ap_s_max(uint64_t total, uint32_t nb) {
    const uint64_t per_block = total / nb / (uint64_t)ap_geom::SM_TARGET;
    return (uint32_t)(per_block < 2 ? 2 : (per_block > 0x100000ull ? 0x100000ull : per_block));
}
SMG_HD ApPlan ap_plan(uint64_t max_hash, uint32_t s_max) {
    uint32_t shift = 0;
    while ((max_hash >> shift) >= (uint64_t)s_max) ++shift;                  // s_max >= 2: ends at 63 at the latest
    return ApPlan{shift, (uint32_t)(max_hash >> shift) + 1u};                 // <= s_max slices
}
// cuts[r][s], s = 0 .. s_max: the first entry of a row of len hashes that belongs to slice s or a later one
SMG_HD uint32_t ap_cut(const uint64_t* row, uint32_t len, uint32_t s, ApPlan plan) {
    if (s >= plan.n_slices) return len;
    if (s == 0) return 0;
    return lower_bound_u64(row, 0u, len, (uint64_t)s << plan.shift);          // <= the largest hash: no overflow
}
// the order-preserving sub-bucket, of SM_BUCKETS, of hash h in the slice that starts at base = s << shift
SMG_HD uint32_t ap_bucket(uint64_t h, uint64_t base, uint32_t shift) {
    const uint64_t rel = h - base;
    return (uint32_t)(shift > (uint32_t)ap_geom::SM_BUCKET_BITS ? rel >> (shift - ap_geom::SM_BUCKET_BITS) : rel);
}
// Hash slices per tile of the join: enough work items to fill the chip twice over when the tiles alone do not -- ~2.5 workgroups
// per CU, and an ODD count: C3 (136 tiles, round 6) 1.49 / 1.19 / 1.28 / 1.18 / 1.28 / 1.21 / 1.27 ms for the call at 2 / 3 / 4 /
// 5 / 6 / 7 / 8 slices -- with an even count the slices of one tile sit on workgroup ids that differ by less than 8 and so on
// different XCDs at the same moment, all adding into the same output tile through eight L2s.  (SMG_ABUND_SLICES overrides.)
SMG_HD uint32_t ap_slices_per_tile(uint64_t tiles) {
    uint32_t Z = tiles >= 640 ? 1u : (uint32_t)((640 + tiles - 1) / tiles) | 1u;
    if (Z > (uint32_t)ap_geom::AP_ZMAX - 1u) Z = (uint32_t)ap_geom::AP_ZMAX - 1u;
    return Z;
}
// tile t = (bi, bj), bi <= bj, enumerated row by row of the upper triangle of nb x nb blocks
SMG_HD void ap_tile_of(uint32_t t, uint32_t nb, uint32_t* bi, uint32_t* bj) {
    uint32_t i = 0;
    while (t >= nb - i) { t -= nb - i; ++i; }                                  // (nb is small: at most a few hundred steps)
    *bi = i; *bj = i + t;
}
// slice z of Z of a tile's join: an equal share of list A's entries [A0, A1), moved to the start of a run of equal hashes; list B
// [B0, B1) between the same two hash values.  out = {a0, a1, b0, b1}
SMG_HD void ap_slice_bounds(const uint64_t* __restrict__ l_hash, uint64_t A0, uint64_t A1, uint64_t B0, uint64_t B1, uint32_t z, uint32_t Z,
                            uint64_t* out) {
    uint64_t a0 = A0 + (A1 - A0) * z / Z, a1 = z + 1 == Z ? A1 : A0 + (A1 - A0) * (z + 1) / Z;
    if (a0 > A0 && a0 < A1) a0 = lower_bound_u64(l_hash, A0, a0, l_hash[a0]);
    if (a1 > A0 && a1 < A1) a1 = lower_bound_u64(l_hash, A0, a1, l_hash[a1]);
    uint64_t b0 = B0, b1 = B1;
    if (a0 < a1) {
        if (a0 > A0) b0 = lower_bound_u64(l_hash, B0, B1, l_hash[a0]);
        if (a1 < A1) b1 = lower_bound_u64(l_hash, b0, B1, l_hash[a1]);
    } else b1 = b0;
    out[0] = a0; out[1] = a1; out[2] = b0; out[3] = b1;
}
// a staged chunk of n_staged entries of list B is used in whole runs of equal hashes: when more of the list follows, the run the
// chunk ends in may go on and is left for the next round.  (> 0: a run holds at most AP_T entries, fewer than a chunk.)
SMG_HD uint64_t ap_trim_to_runs(const uint64_t* staged, uint64_t n_staged, bool more_follow) {
    if (!more_follow) return n_staged;
    const uint64_t last = staged[n_staged - 1];
    uint64_t cut = n_staged - 1;
    while (cut > 0 && staged[cut - 1] == last) --cut;
    return cut;
}
// The searches of the join over the AP_CHUNK staged hashes (entries past the staged ones hold 2^64 - 1), in fixed steps: twelve
// for the lower bound of h, six for the length of its run from lo (at most AP_T entries, all below n_staged).
SMG_HD uint32_t ap_find(const uint64_t* staged, uint64_t h) {
    uint32_t lo = 0;
    SMG_UNROLL
    for (uint32_t len = ap_geom::AP_CHUNK / 2; len; len >>= 1) lo += staged[lo + len - 1] < h ? len : 0u;
    return lo;
}
SMG_HD uint32_t ap_run_len(const uint64_t* staged, uint32_t lo, uint32_t n_staged, uint64_t h) {
    uint32_t cnt = 1;
    SMG_UNROLL
    for (uint32_t len = ap_geom::AP_T / 2; len; len >>= 1) {
        const uint32_t at = lo + cnt + len - 1;
        if (at < n_staged && staged[at] == h) cnt += len;
    }
    return cnt;
}
// a worklist word: run start (12 bits) | run length << 12 (7 bits) | row of A's entry << 19
SMG_HD uint32_t ap_work_pack(uint32_t lo, uint32_t cnt, uint32_t row) { return lo | (cnt << 12) | (row << 19); }
SMG_HD void ap_work_unpack(uint32_t e, uint32_t* lo, uint32_t* cnt, uint32_t* row) {
    *lo = e & 4095u; *cnt = (e >> 12) & 127u; *row = e >> 19;
}

// ---- the path choice of a compare() (capi_compare.cpp: bitindex_build) -----------------------------------------------------------
// measured rates behind the cost model (1 x MI355X)
constexpr double RATE_MERGE_STEPS = 6.0e12;   // merge-step equivalents / s of compare_hash_kernel (a pair of sketches = n_i + n_j steps): 5.7e12 at 1,000 x 5,000
                                              // hashes, 7.0e12 at 2,000, 9.5e12 at C4 (profiles/r06_compare_small.jsonl) -- the smaller one decides small problems
constexpr double MERGE_ROUND_FLOOR = 6.0e-8;  // seconds per hash of the mean sketch: the latency floor of the general kernel's rounds
constexpr double RATE_BIT_WORDS = 9.5e12;     // 32-bit AND+popcount / s (bitmatrix_kernel at C4: the VALU roof)
constexpr double RATE_PAIR_ATOMICS = 4.0e9;   // matrix increments / s (rare_pairs_kernel)
// the all-pairs callers compute the triangle and mirror it: a pair costs ONE visit of its tile / ONE increment, like the
// n * total / 2 ... steps the merge rate is calibrated on.  (A bit column costs n^2/2 pairs x 1/32 word, a rare hash held by
// m sketches m^2/2 increments: they meet at m = n * sqrt(RATE_PAIR_ATOMICS / (32 * 2 * RATE_BIT_WORDS)), the threshold below.)
constexpr double TRIANGLE = 0.5;
constexpr uint32_t COMPARE_DICT_MAX_N = 2u << 20;          // the dictionary builder's slice bounds take 2 KB per sketch: past two
                                                           // million sketches the sort's scratch is the smaller one
constexpr double COMPARE_BITMAP_CAP_BYTES = 8.0 * (1ull << 30);

struct ComparePathModel {
    uint32_t threshold;      // holders from which a hash becomes a bit column
    double t_merge;          // seconds the general kernel is expected to take
    bool try_dict, try_sort; // whether each builder is worth starting at all
};
// n >= 1 sketches with 1 <= total <= 2^32 - 1 hashes in all.  An index that serves ONE compare (one_shot) must also pay for its own
// build: the dictionary ~0.1 ms of launches + three passes over the elements; the sort ~0.6 ms of fixed cost + total / 1.4e9 s
// (round 6: a collection of mostly private hashes, 1,000 / 2,000 sketches of 5,000: 3.8 / 8.2 ms through that builder against
// 0.88 / 2.8 ms for the general kernel -- the earlier total / 5e9 sent such collections there, tools/bench_compare_small.py).
// A forced threshold asks for an index whatever it costs.
SMG_HD ComparePathModel compare_path_model(uint32_t n, uint64_t total, uint32_t forced_threshold, bool one_shot) {
    ComparePathModel m;
    // (the general kernel walks a tile's sketches in lock-step rounds of <= 64 hashes, ~4 us a round however few tiles there are:
    //  sixteen 5,000-hash sketches take 0.32 ms, 256 of them 0.43 -- tools/bench_compare_small.py, profiles/r06_compare_small.jsonl)
    const double by_steps = (double)n * (double)total / RATE_MERGE_STEPS, by_rounds = (double)total / (double)n * MERGE_ROUND_FLOOR;
    m.t_merge = by_steps < by_rounds ? by_rounds : by_steps;
    // a hash held by m sketches costs m^2 increments as a rare hash, or one bit column (n^2/2 pairs x 1/32 word) as
    // a frequent one: the two meet at m ~ n * sqrt(RATE_PAIR_ATOMICS / (64 * RATE_BIT_WORDS))
    m.threshold = (uint32_t)((double)n * __builtin_sqrt(RATE_PAIR_ATOMICS / (64.0 * RATE_BIT_WORDS)));
    if (m.threshold < 1) m.threshold = 1;
    if (forced_threshold) m.threshold = forced_threshold;
    const bool must_pay = one_shot && !forced_threshold;
    m.try_dict = n <= COMPARE_DICT_MAX_N && !(must_pay && m.t_merge < 0.1e-3 + (double)total / 4.0e10);
    m.try_sort = !(must_pay && m.t_merge < 0.6e-3 + (double)total / 1.4e9);
    return m;
}
// What a builder found -- n_freq frequent hashes, rare_pairs increments for the rare ones -- against the general kernel: the words
// of a bit row (whole 32-word k-steps), or a refusal when the general kernel is expected to win (unless forced) or the bit rows
// would pass the 8 GiB cap.
struct CompareIndexAccept { bool accept; uint32_t words; };
SMG_HD CompareIndexAccept compare_index_accept(uint32_t n, uint64_t n_freq, uint64_t rare_pairs, uint64_t total, double t_merge, bool forced) {
    const uint32_t words = n_freq ? (uint32_t)(((n_freq + 31) / 32 + 31) / 32 * 32) : 0;
    const double pairs = 0.5 * (double)n * (double)n;
    const double t_index = TRIANGLE * (pairs * (double)words / RATE_BIT_WORDS + 2.0 * (double)rare_pairs / RATE_PAIR_ATOMICS) +
                           (double)total / 2.0e10;                                         // + one pass over the elements
    const bool refuse = (t_index > t_merge && !forced) || (double)n * words * 4.0 > COMPARE_BITMAP_CAP_BYTES;
    return CompareIndexAccept{!refuse, words};
}

}  // namespace smg
