// uniform_sort_core.hpp -- the rules of the sort + unique for uniformly spread keys (uniform_sort.hip) that the host and the
// device share.  Plain C++ on the host (tests/native/uniform_sort_emul.cpp compiles it with g++ and walks the kernels' lane code
// with lanes as loop indices).
//
// Kept hashes are MurmurHash3 values, uniform on [1, thr]: the top bits of a key give its place in the sorted output to within a
// few hundred positions.  The plan cuts the key space into L = (thr >> shift) + 1 leaves of equal width; every leaf owns a region
// of US_LEAF_CAP slots in the workspace.  `shift` is the largest one whose expected leaf load, for n_max keys, stays 8 standard
// deviations (sqrt(load)) under the capacity.  Keys are scattered to their leaves in one 256-way pass (L <= 256) or two (coarse
// region = leaf >> 8, then leaf); one workgroup sorts a leaf in LDS and drops duplicates; a scan of the leaves' distinct counts and
// a copy finish.  A key outside [0, thr], or a reservation that would pass a region's end, raises the caller's fall-back flag and
// writes nothing: the keys were not uniform and the caller's general sort takes the untouched input.  With n_max small enough one
// workgroup sorts everything in LDS and no assumption about the keys is made at all.
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

constexpr uint32_t US_SMALL_MAX = 16384;   // keys one workgroup sorts in LDS (128 KiB of the CU's 160)
constexpr uint32_t US_LEAF_CAP = 1024;     // slots of a leaf region: 8 KiB of LDS in the leaf kernel
constexpr uint32_t US_FANOUT = 256;        // digits of one scatter pass
constexpr uint32_t US_TILE = 4096;         // keys a scatter workgroup takes
constexpr uint64_t US_MAX_LEAVES = (uint64_t)US_FANOUT * US_FANOUT;

enum UsForm : uint32_t { US_DECLINE = 0, US_SMALL = 1, US_ONE_PASS = 2, US_TWO_PASS = 3 };

struct UsPlan {
    uint32_t form;
    uint32_t shift;        // leaf = key >> shift
    uint64_t leaves;       // L
    uint64_t regions;      // coarse regions of the first pass (two-pass form), region = leaf >> 8
    uint64_t region_cap;   // slots of a coarse region
    uint64_t thr;
};

SMG_HD uint64_t us_isqrt_up(uint64_t x) {   // smallest r with r * r >= x
    uint64_t r = 0;
    while (r * r < x) ++r;
    return r;
}

// whether `cap` slots hold a Poisson load of mean `load` with 8 standard deviations to spare
SMG_HD bool us_load_fits(uint64_t load, uint64_t cap) {
    if (load >= cap) return false;
    const uint64_t spare = cap - load;
    return spare * spare >= 64 * load;
}

SMG_HD uint64_t us_leaves(uint64_t thr, uint32_t shift) { return (thr >> shift) + 1; }

// a function of n_max and thr alone
SMG_HD UsPlan us_plan(uint64_t n_max, uint64_t thr) {
    UsPlan p{US_DECLINE, 0, 0, 0, 0, thr};
    if (n_max <= US_SMALL_MAX) { p.form = US_SMALL; return p; }
    if (n_max > 0xffffffffull) return p;
    int shift = 63;
    for (; shift >= 0; --shift) {
        const uint64_t L = us_leaves(thr, (uint32_t)shift);
        if (L > US_MAX_LEAVES) return p;                         // more leaves than two 256-way passes reach
        if (us_load_fits((n_max + L - 1) / L, US_LEAF_CAP)) break;
    }
    if (shift < 0) return p;                                     // more keys than the values up to thr spread over
    p.shift = (uint32_t)shift;
    p.leaves = us_leaves(thr, p.shift);
    if (p.leaves <= US_FANOUT) { p.form = US_ONE_PASS; return p; }
    p.form = US_TWO_PASS;
    p.regions = ((p.leaves - 1) >> 8) + 1;
    const uint64_t load = ((n_max + p.leaves - 1) / p.leaves) * US_FANOUT;    // expected keys of a full region
    p.region_cap = load + 8 * us_isqrt_up(load);
    return p;
}

// ---- scatter ------------------------------------------------------------------------------------------------------------------
SMG_HD uint64_t us_leaf_of(const UsPlan& p, uint64_t key) { return key >> p.shift; }
// the digit of `key` in the first pass (coarse region, or the leaf itself in the one-pass form); US_FANOUT = not a key of [0, thr]
SMG_HD uint32_t us_digit_first(const UsPlan& p, uint64_t key) {
    if (key > p.thr) return US_FANOUT;
    const uint64_t leaf = us_leaf_of(p, key);
    return (uint32_t)(p.form == US_TWO_PASS ? leaf >> 8 : leaf);
}
// the digit of `key` in the second pass, inside coarse region `region`; US_FANOUT = the key does not belong there
SMG_HD uint32_t us_digit_second(const UsPlan& p, uint64_t region, uint64_t key) {
    if (key > p.thr) return US_FANOUT;
    const uint64_t leaf = us_leaf_of(p, key);
    return (leaf >> 8) == region ? (uint32_t)(leaf & 0xff) : US_FANOUT;
}
// whether `count` keys reserved at `base` (the cursor's value before the add) lie inside a region of `cap` slots
SMG_HD bool us_reserve_ok(uint64_t base, uint64_t count, uint64_t cap) { return base <= cap && count <= cap - base; }

// ---- sorting in LDS, the usual way: counting sort by the key's next bits, then ranks inside a bin -------------------------------
// n keys that are uniform over the span of one workgroup's share (a leaf; the whole of [0, thr] in the one-workgroup form) fall into
// bins of about one key each.  A key's bin and its arrival number there (an LDS atomic) give it a slot in a staging copy grouped by
// bin; its place in the sorted order is its bin's start plus the keys of the bin that come before it (us_before: smaller, or equal
// and staged earlier -- equal keys always share a bin, so they end up adjacent).  A bin with more than US_BIN_LIMIT keys means the
// keys do not spread: the workgroup takes the sorting network below instead, whose cost does not depend on the keys.
constexpr uint32_t US_LEAF_BINS = 1024;
constexpr uint32_t US_SMALL_BINS = 4096;
constexpr uint32_t US_BIN_LIMIT = 32;
// a leaf's keys share the bits from `shift` up: the 10 bits under them (all of them when there are fewer) are the bin
SMG_HD uint32_t us_bin_leaf(uint32_t shift, uint64_t key) { return (uint32_t)(key >> (shift > 10 ? shift - 10 : 0)) & (US_LEAF_BINS - 1); }
// one workgroup: the smallest shift that leaves thr inside the bins; any key may come, those above thr share the last bin
SMG_HD uint32_t us_small_shift(uint64_t thr) {
    uint32_t s = 0;
    while (s < 63 && (thr >> s) >= US_SMALL_BINS) ++s;
    return s;
}
SMG_HD uint32_t us_bin_small(uint32_t small_shift, uint64_t key) {
    const uint64_t b = key >> small_shift;
    return b < US_SMALL_BINS ? (uint32_t)b : US_SMALL_BINS - 1;
}
// whether the key `other` staged at slot `other_at` sorts in front of `key` staged at `at`
SMG_HD bool us_before(uint64_t other, uint32_t other_at, uint64_t key, uint32_t at) { return other < key || (other == key && other_at < at); }

// ---- the sorting network: a bitonic sort whose compare-exchanges all point the same way, so that padding is by index ------------
// Slots [n, P) of the P = us_pow2(n) slots count as +infinity and are never read or written: a pair (a, b), a < b, with b >= n has
// nothing to do.  Merge width k = 2, 4 .. P: first the flip (j == 0), then the halvings j = k / 4, k / 8 .. 1.
SMG_HD uint32_t us_pow2(uint32_t n) {
    uint32_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
// pair number t (0 .. P / 2) of a step -> its two slots, a < b
SMG_HD void us_pair(uint32_t t, uint32_t k, uint32_t j, uint32_t& a, uint32_t& b) {
    // k and j are powers of two: the pair's place inside its block of k / 2 (j) pairs is a mask away
    const uint32_t off = t & ((j == 0 ? k >> 1 : j) - 1);
    a = 2 * (t - off) + off;
    b = j == 0 ? 2 * (t - off) + k - 1 - off : a + j;
}
SMG_HD void us_compare_exchange(uint64_t* keys, uint32_t n, uint32_t a, uint32_t b) {
    if (b >= n) return;
    const uint64_t x = keys[a], y = keys[b];
    if (x > y) { keys[a] = y; keys[b] = x; }
}
// the step after (k, j); k > P when the network is through.  Start with k = 2, j = 0.
SMG_HD void us_next_step(uint32_t& k, uint32_t& j) {
    if (j == 0) j = k >> 2; else j >>= 1;
    if (j == 0) k <<= 1;
}

// ---- duplicates: slot i of the sorted keys[0, n) opens a run / closes one ------------------------------------------------------
SMG_HD bool us_is_head(const uint64_t* keys, uint32_t i) { return i == 0 || keys[i] != keys[i - 1]; }
SMG_HD bool us_is_tail(const uint64_t* keys, uint32_t n, uint32_t i) { return i + 1 == n || keys[i] != keys[i + 1]; }

}  // namespace smg
