// Host emulation of uniform_sort.hip: the plan and the lane code of sourmash_amd/csrc/uniform_sort_core.hpp, walked with lanes as
// loop indices the way the kernels walk them (scatter histogram / reservation / ranked writes, the counting sort in LDS with ranks
// inside a bin and the sorting network behind a crowded bin, the head / tail pass that drops duplicates and counts them, scan and
// pack), against std::sort + std::unique.  A stand-alone program:
//     uniform_sort_emul                 the built-in cases; prints "uniform sort ok: N cases"
//     uniform_sort_emul FILE            cases from a file (tests/test_uniform_sort_core_cpu.py writes the GPU tests' inputs):
//                                       records {u64 n_max, count, thr, want: 0 must not fall back / 1 must / 2 either, n_keys}
//                                       + keys; prints one line per record and the same last line
// Every buffer has its exact size, so under -fsanitize=address,undefined a read or write outside one is a report.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../sourmash_amd/csrc/uniform_sort_core.hpp"

using namespace smg;
typedef std::vector<uint64_t> Keys;

static int g_cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); \
                                              fprintf(stderr, "\n"); exit(1); } } while (0)

// us_sort_lds<T>: every step's pairs by the lanes t, t + T ..; a barrier between steps
static void emul_sort(uint64_t* keys, uint32_t n, uint32_t T) {
    const uint32_t P = us_pow2(n);
    for (uint32_t k = 2, j = 0; k <= P; us_next_step(k, j))
        for (uint32_t lane = 0; lane < T; ++lane)
            for (uint32_t t = lane; t < P / 2; t += T) {
                uint32_t a, b;
                us_pair(t, k, j, a, b);
                CHECK(a < b && b < P, "pair (%u, %u) of step (%u, %u)", a, b, k, j);
                us_compare_exchange(keys, n, a, b);
            }
}

// us_sort_keys<T, E, B, LEAF>: src[0, n) -> sorted s[0, n); the counting sort over B bins with ranks inside a bin, or the network
// when a bin holds more than US_BIN_LIMIT keys.  -> whether the network ran
static bool emul_sort_keys(const uint64_t* src, uint32_t n, uint32_t T, uint32_t E, uint32_t B, bool leaf, uint32_t bin_shift, uint64_t* s) {
    auto bin_of = [&](uint64_t key) { return leaf ? us_bin_leaf(bin_shift, key) : us_bin_small(bin_shift, key); };
    std::vector<uint32_t> bins(B + 1, 0), at((size_t)T * E, 0);
    std::vector<uint64_t> key((size_t)T * E, 0);
    CHECK(n <= T * E, "keys per workgroup");
    for (uint32_t lane = 0; lane < T; ++lane)
        for (uint32_t e = 0; e < E; ++e) {
            const uint32_t i = lane + e * T;
            if (i >= n) continue;
            key[lane * E + e] = src[i];
            CHECK(bin_of(src[i]) < B, "bin");
            at[lane * E + e] = bins[bin_of(src[i])]++;
        }
    uint32_t most = 0, start = 0;
    for (uint32_t b = 0; b < B; ++b) most = std::max(most, bins[b]);
    if (most > US_BIN_LIMIT) {
        for (uint32_t lane = 0; lane < T; ++lane)
            for (uint32_t e = 0; e < E; ++e)
                if (lane + e * T < n) s[lane + e * T] = key[lane * E + e];
        emul_sort(s, n, T);
        return true;
    }
    for (uint32_t b = 0; b < B; ++b) { const uint32_t c = bins[b]; bins[b] = start; start += c; }
    bins[B] = start;
    CHECK(start == n, "bins hold %u of %u keys", start, n);
    for (uint32_t lane = 0; lane < T; ++lane)
        for (uint32_t e = 0; e < E; ++e) {
            if (lane + e * T >= n) continue;
            at[lane * E + e] += bins[bin_of(key[lane * E + e])];
            s[at[lane * E + e]] = key[lane * E + e];
        }
    std::vector<uint32_t> rank((size_t)T * E, 0);
    for (uint32_t lane = 0; lane < T; ++lane)
        for (uint32_t e = 0; e < E; ++e) {
            if (lane + e * T >= n) continue;
            const uint32_t b = bin_of(key[lane * E + e]);
            uint32_t r = bins[b];
            for (uint32_t m = bins[b]; m < bins[b + 1]; ++m) r += us_before(s[m], m, key[lane * E + e], at[lane * E + e]) ? 1 : 0;
            rank[lane * E + e] = r;
        }
    std::vector<char> taken(n, 0);
    for (uint32_t lane = 0; lane < T; ++lane)                      // behind the barrier: the staging copy becomes the sorted one
        for (uint32_t e = 0; e < E; ++e) {
            if (lane + e * T >= n) continue;
            CHECK(rank[lane * E + e] < n && !taken[rank[lane * E + e]], "rank %u twice", rank[lane * E + e]);
            taken[rank[lane * E + e]] = 1;
            s[rank[lane * E + e]] = key[lane * E + e];
        }
    return false;
}

static uint64_t g_network_runs = 0, g_counting_runs = 0;

// us_unique_write<T, E, CT>: lane t owns the slots [t * E, t * E + E)
template <typename CT>
static uint32_t emul_unique_write(const uint64_t* keys, uint32_t n, uint32_t T, uint32_t E, uint64_t* out, CT* counts) {
    std::vector<uint32_t> heads(T, 0), first(T, 0);
    for (uint32_t lane = 0; lane < T; ++lane)
        for (uint32_t e = 0; e < E; ++e)
            if (lane * E + e < n && us_is_head(keys, lane * E + e)) ++heads[lane];
    uint32_t total = 0;
    for (uint32_t lane = 0; lane < T; ++lane) { first[lane] = total; total += heads[lane]; }
    for (uint32_t lane = 0; lane < T; ++lane) {
        uint32_t q = first[lane];
        for (uint32_t e = 0; e < E; ++e) {
            const uint32_t i = lane * E + e;
            if (i < n && us_is_head(keys, i)) {
                out[q] = keys[i];
                if (counts) counts[q] = (CT)0 - (CT)i;
                ++q;
            }
        }
    }
    if (counts)
        for (uint32_t lane = 0; lane < T; ++lane) {             // behind the barrier
            uint32_t q = first[lane];
            for (uint32_t e = 0; e < E; ++e) {
                const uint32_t i = lane * E + e;
                if (i >= n) break;
                if (us_is_head(keys, i)) ++q;
                if (us_is_tail(keys, n, i)) counts[q - 1] += (CT)(i + 1);
            }
        }
    return total;
}

// one us_scatter_kernel launch.  second: src holds the coarse regions, src_cursor their fill
static void emul_scatter(const UsPlan& p, bool second, const uint64_t* src, uint64_t n_first, const std::vector<uint32_t>& src_cursor,
                         std::vector<uint32_t>& cursor, Keys& dst, uint64_t dst_cap, uint32_t& fellback) {
    const uint64_t tiles_per_region = second ? (p.region_cap + US_TILE - 1) / US_TILE : 1;
    const uint64_t blocks = second ? p.regions * tiles_per_region : (n_first + US_TILE - 1) / US_TILE;
    for (uint64_t blk = 0; blk < blocks; ++blk) {
        uint64_t region = 0, n = n_first, begin = blk * US_TILE, src_at = 0, cur_at = 0, dst_at = 0;
        if (second) {
            region = blk / tiles_per_region;
            n = std::min<uint64_t>(src_cursor[region], p.region_cap);
            begin = (blk % tiles_per_region) * US_TILE;
            src_at = region * p.region_cap;
            cur_at = region * US_FANOUT;
            dst_at = region * US_FANOUT * dst_cap;
        }
        if (begin >= n) continue;
        uint32_t hist[US_FANOUT] = {0}, base[US_FANOUT];
        std::vector<uint64_t> key(US_TILE, 0);
        std::vector<uint32_t> digit(US_TILE, US_FANOUT), rank(US_TILE, 0);
        for (uint32_t lane = 0; lane < 256; ++lane)
            for (uint32_t e = 0; e < US_TILE / 256; ++e) {
                const uint64_t i = begin + (uint64_t)e * 256 + lane;
                const uint32_t slot = e * 256 + lane;
                if (i >= n) continue;
                key[slot] = src[src_at + i];
                digit[slot] = second ? us_digit_second(p, region, key[slot]) : us_digit_first(p, key[slot]);
                if (digit[slot] < US_FANOUT) rank[slot] = hist[digit[slot]]++;
                else fellback = 1;
            }
        for (uint32_t d = 0; d < US_FANOUT; ++d) {
            base[d] = 0xffffffffu;
            if (!hist[d]) continue;
            const uint32_t at = cursor.at(cur_at + d);
            cursor.at(cur_at + d) += hist[d];
            if (us_reserve_ok(at, hist[d], dst_cap)) base[d] = at; else fellback = 1;
        }
        for (uint32_t slot = 0; slot < US_TILE; ++slot)
            if (digit[slot] < US_FANOUT && base[digit[slot]] != 0xffffffffu)
                dst.at(dst_at + (uint64_t)digit[slot] * dst_cap + base[digit[slot]] + rank[slot]) = key[slot];
    }
}

struct Result { uint32_t form = 0, fellback = 0; Keys out, counts; };

static Result emul_sort_unique(const Keys& keys, uint64_t count, uint64_t n_max, uint64_t thr) {
    Result r;
    const UsPlan p = us_plan(n_max, thr);
    r.form = p.form;
    const uint64_t n = std::min(count, n_max);
    CHECK(n <= keys.size(), "count");
    if (p.form == US_DECLINE) { r.fellback = 1; return r; }
    if (p.form == US_SMALL) {
        Keys s(n);
        (emul_sort_keys(keys.data(), (uint32_t)n, 1024, US_SMALL_MAX / 1024, US_SMALL_BINS, false, us_small_shift(thr), s.data()) ? g_network_runs
                                                                                                                                   : g_counting_runs)++;
        r.out.assign(n, 0);
        r.counts.assign(n, 0);
        const uint32_t total = emul_unique_write<uint64_t>(s.data(), (uint32_t)n, 1024, US_SMALL_MAX / 1024, r.out.data(), r.counts.data());
        r.out.resize(total);
        r.counts.resize(total);
        return r;
    }
    const uint64_t n_leaves = p.form == US_TWO_PASS ? p.regions * US_FANOUT : US_FANOUT;
    std::vector<uint32_t> coarse_cursor(US_FANOUT, 0), leaf_cursor(n_leaves, 0), none;
    Keys coarse(p.regions * p.region_cap, 0xDEADDEADDEADDEADull), leaves(p.leaves * US_LEAF_CAP, 0xDEADDEADDEADDEADull);
    if (p.form == US_ONE_PASS) {
        emul_scatter(p, false, keys.data(), n, none, leaf_cursor, leaves, US_LEAF_CAP, r.fellback);
    } else {
        emul_scatter(p, false, keys.data(), n, none, coarse_cursor, coarse, p.region_cap, r.fellback);
        if (!r.fellback) emul_scatter(p, true, coarse.data(), 0, coarse_cursor, leaf_cursor, leaves, US_LEAF_CAP, r.fellback);
    }
    if (r.fellback) return r;
    std::vector<uint32_t> leaf_counts(p.leaves * US_LEAF_CAP, 0), distinct(n_leaves, 0), offsets(n_leaves + 1, 0);
    for (uint64_t leaf = 0; leaf < p.leaves; ++leaf) {
        const uint32_t ln = std::min<uint32_t>(leaf_cursor[leaf], US_LEAF_CAP);
        Keys src(leaves.begin() + leaf * US_LEAF_CAP, leaves.begin() + leaf * US_LEAF_CAP + ln), s(ln);
        (emul_sort_keys(src.data(), ln, 256, US_LEAF_CAP / 256, US_LEAF_BINS, true, p.shift, s.data()) ? g_network_runs : g_counting_runs)++;
        distinct[leaf] = emul_unique_write<uint32_t>(s.data(), ln, 256, US_LEAF_CAP / 256, &leaves[leaf * US_LEAF_CAP],
                                                     &leaf_counts[leaf * US_LEAF_CAP]);
    }
    for (uint64_t leaf = 0; leaf < p.leaves; ++leaf) offsets[leaf + 1] = offsets[leaf] + distinct[leaf];
    r.out.assign(offsets[p.leaves], 0);
    r.counts.assign(offsets[p.leaves], 0);
    for (uint64_t leaf = 0; leaf < p.leaves; ++leaf)
        for (uint32_t i = 0; i < distinct[leaf]; ++i) {
            r.out.at(offsets[leaf] + i) = leaves[leaf * US_LEAF_CAP + i];
            r.counts.at(offsets[leaf] + i) = leaf_counts[leaf * US_LEAF_CAP + i];
        }
    return r;
}

enum Want { NO_FALLBACK = 0, FALLBACK = 1, EITHER = 2 };

static Result run_case(const char* what, const Keys& keys, uint64_t count, uint64_t n_max, uint64_t thr, int want, int form = -1) {
    Result r = emul_sort_unique(keys, count, n_max, thr);
    ++g_cases;
    if (form >= 0) CHECK((int)r.form == form, "%s: form %u, expected %d", what, r.form, form);
    if (want == NO_FALLBACK) CHECK(!r.fellback, "%s fell back", what);
    if (want == FALLBACK) CHECK(r.fellback, "%s did not fall back", what);
    if (r.fellback) return r;
    Keys ref(keys.begin(), keys.begin() + std::min(count, n_max));
    std::sort(ref.begin(), ref.end());
    Keys uniq, cnt;
    for (size_t i = 0; i < ref.size(); ++i) {
        if (i == 0 || ref[i] != ref[i - 1]) { uniq.push_back(ref[i]); cnt.push_back(0); }
        ++cnt.back();
    }
    CHECK(r.out == uniq, "%s: keys differ (%zu, %zu)", what, r.out.size(), uniq.size());
    CHECK(r.counts == cnt, "%s: counts differ", what);
    return r;
}

static uint64_t uniform_key(std::mt19937_64& g, uint64_t thr) {     // on [1, thr]
    if (thr == ~0ull) { uint64_t v; do v = g(); while (v == 0); return v; }
    return 1 + g() % thr;
}
static Keys uniform_keys(uint64_t n, uint64_t thr, uint64_t seed, double twice = 0.0) {
    std::mt19937_64 g(seed);
    Keys k;
    while (k.size() < n) {
        const uint64_t v = uniform_key(g, thr);
        k.push_back(v);
        if (k.size() < n && (double)(g() % 1000) < twice * 1000) k.push_back(v);
    }
    std::shuffle(k.begin(), k.end(), g);
    return k;
}

static void plan_cases() {
    // the rule itself, over sizes and thresholds: a function of n_max and thr; the chosen shift fits and the next larger one does not
    const uint64_t thrs[] = {1, 2, 20, 40, 255, 256, 1ull << 24, (1ull << 24) + 1, 18446744073709551ull, (256ull << 40) - 1, 256ull << 40,
                             (255ull << 40) - 1, 257ull << 40, (1ull << 63) - 1, 1ull << 63, ~0ull};
    const uint64_t sizes[] = {0, 1, 2, US_SMALL_MAX - 1, US_SMALL_MAX, US_SMALL_MAX + 1, 20000, 100000, 150000, 2000000, 12529394, 51000000,
                              60000000, 0xffffffffull, 0x100000000ull};
    for (uint64_t thr : thrs)
        for (uint64_t n_max : sizes) {
            const UsPlan p = us_plan(n_max, thr);
            ++g_cases;
            if (n_max <= US_SMALL_MAX) { CHECK(p.form == US_SMALL, "small"); continue; }
            if (p.form == US_DECLINE) {
                // no shift fits at all, or the first that fits needs more leaves than two passes reach, or 2^32 keys and more
                bool fits = false;
                for (int s = 63; s >= 0 && !fits; --s) {
                    const uint64_t L = us_leaves(thr, s);
                    if (L > US_MAX_LEAVES) break;
                    fits = us_load_fits((n_max + L - 1) / L, US_LEAF_CAP);
                }
                CHECK(!fits || n_max > 0xffffffffull, "declined n_max %llu thr %llu", (unsigned long long)n_max, (unsigned long long)thr);
                continue;
            }
            CHECK(p.leaves == (thr >> p.shift) + 1 && p.leaves <= US_MAX_LEAVES, "leaves");
            const uint64_t load = (n_max + p.leaves - 1) / p.leaves;
            CHECK(load + 8 * us_isqrt_up(load) <= US_LEAF_CAP + 8, "load %llu", (unsigned long long)load);
            CHECK(us_load_fits(load, US_LEAF_CAP), "fits");
            if (p.shift < 63) {
                const uint64_t L1 = us_leaves(thr, p.shift + 1);
                CHECK(!us_load_fits((n_max + L1 - 1) / L1, US_LEAF_CAP), "a larger shift fits too");
            }
            CHECK((p.form == US_ONE_PASS) == (p.leaves <= US_FANOUT), "passes");
            if (p.form == US_TWO_PASS) {
                CHECK(p.regions == (p.leaves + 255) / 256 && p.regions <= US_FANOUT, "regions");
                CHECK(us_load_fits(load * US_FANOUT, p.region_cap + 1), "region capacity");
            }
            // every key of [0, thr] has a digit in both passes, every other key has none
            const uint64_t probes[] = {0, 1, thr / 2, thr - 1, thr};
            for (uint64_t k : probes) {
                if (k > thr) continue;
                const uint32_t d1 = us_digit_first(p, k);
                CHECK(d1 < US_FANOUT, "first digit");
                if (p.form == US_TWO_PASS) {
                    CHECK(d1 < p.regions && us_digit_second(p, d1, k) < US_FANOUT && us_digit_second(p, d1 + 1, k) == US_FANOUT, "second digit");
                    CHECK((uint64_t)d1 * 256 + us_digit_second(p, d1, k) == us_leaf_of(p, k), "leaf");
                } else {
                    CHECK(d1 == us_leaf_of(p, k) && d1 < p.leaves, "leaf");
                }
            }
            if (thr != ~0ull) CHECK(us_digit_first(p, thr + 1) == US_FANOUT && us_digit_first(p, ~0ull) == US_FANOUT, "stray key");
        }
    // L on either side of 256 and 257 (150,000 keys: 128 leaves are too few, shift 40 it is); L = 1 and 2 exist only where the
    // one-workgroup form has taken the input (a leaf holds 798 keys at the most, US_SMALL_MAX is 16,384)
    CHECK(us_plan(150000, (255ull << 40) - 1).leaves == 255 && us_plan(150000, (255ull << 40) - 1).form == US_ONE_PASS, "L 255");
    CHECK(us_plan(150000, (256ull << 40) - 1).leaves == 256 && us_plan(150000, (256ull << 40) - 1).form == US_ONE_PASS, "L 256");
    CHECK(us_plan(150000, 256ull << 40).leaves == 257 && us_plan(150000, 256ull << 40).form == US_TWO_PASS, "L 257");
    CHECK(us_plan(150000, 257ull << 40).leaves == 258 && us_plan(150000, 257ull << 40).form == US_TWO_PASS, "L 258");
    CHECK(us_leaves(1, 1) == 1 && us_leaves(1, 0) == 2 && us_plan(16384, 1).form == US_SMALL, "L 1 and 2");
    // the sketch of 10^10 bases at scaled = 1000
    const UsPlan c2 = us_plan(12529394, 18446744073709551ull);
    CHECK(c2.form == US_TWO_PASS && c2.shift == 40 && c2.leaves == 16778, "C2 plan: shift %u leaves %llu", c2.shift, (unsigned long long)c2.leaves);
}

static void sort_cases() {
    const uint64_t MAX = ~0ull;
    // ---- the sorting network by itself (the kernels reach it only through a crowded bin), and the bin rules
    for (uint32_t n : {0, 1, 2, 3, 5, 64, 65, 1000, 1023, 1024, 1025, 4097}) {
        for (uint32_t T : {256u, 1024u}) {
            Keys k = uniform_keys(n, MAX, 900 + n, 0.3), ref = k;
            emul_sort(k.data(), n, T);
            std::sort(ref.begin(), ref.end());
            CHECK(k == ref, "network n %u", n);
            ++g_cases;
        }
    }
    for (uint64_t thr : std::vector<uint64_t>{1, 4095, 4096, 4097, 18446744073709551ull, MAX - 1, MAX}) {
        const uint32_t sh = us_small_shift(thr);
        CHECK((thr >> sh) < US_SMALL_BINS && (sh == 0 || (thr >> (sh - 1)) >= US_SMALL_BINS), "small shift of %llu", (unsigned long long)thr);
        CHECK(us_bin_small(sh, 0) == 0 && us_bin_small(sh, thr) == (thr >> sh) && us_bin_small(sh, MAX) <= US_SMALL_BINS - 1, "small bins");
        CHECK(us_bin_small(sh, thr / 2) <= us_bin_small(sh, thr / 2 + 1), "monotone");
        ++g_cases;
    }
    for (uint32_t shift : {0u, 1u, 9u, 10u, 11u, 40u, 46u, 63u}) {
        const uint64_t lo = shift == 63 ? 1ull << 63 : 5ull << shift, hi = lo + ((1ull << shift) - 1);
        CHECK(us_bin_leaf(shift, lo) <= us_bin_leaf(shift, lo + (hi - lo) / 2) && us_bin_leaf(shift, lo + (hi - lo) / 2) <= us_bin_leaf(shift, hi), "leaf bins");
        ++g_cases;
    }
    // ---- one workgroup: any keys; sizes around the powers of two of the network
    for (uint64_t n : {0, 1, 2, 3, 4, 5, 63, 64, 65, 1000, 1023, 1024, 1025, 4518, 8191, 8192, 8193, 16383, 16384}) {
        run_case("small uniform", uniform_keys(n, MAX, 100 + n, 0.3), n, n, MAX, NO_FALLBACK, US_SMALL);
        run_case("small all equal", Keys(n, 77), n, n, 1000, NO_FALLBACK, US_SMALL);
        Keys alt(n);
        for (uint64_t i = 0; i < n; ++i) alt[i] = i & 1 ? MAX : 1;
        run_case("small alternating 1 and 2^64 - 1", alt, n, n, MAX, NO_FALLBACK, US_SMALL);
    }
    {   // a device count below and above n_max
        const Keys k = uniform_keys(5000, MAX, 7, 0.2);
        run_case("small count below", k, 1234, 5000, MAX, NO_FALLBACK, US_SMALL);
        run_case("small count above", k, 999999, 5000, MAX, NO_FALLBACK, US_SMALL);
        run_case("small count 0", k, 0, 5000, MAX, NO_FALLBACK, US_SMALL);
    }
    // ---- bucket form.  thr and n_max as in plan_cases: 255 / 256 leaves in one pass, 257 / 258 in two
    const uint64_t thrs[] = {(255ull << 40) - 1, (256ull << 40) - 1, 256ull << 40, 257ull << 40};
    for (uint64_t thr : thrs) {
        const UsPlan p = us_plan(150000, thr);
        Keys k = uniform_keys(149000, thr, thr % 1000, 0.3);
        k[0] = 1; k[1] = thr; k[2] = thr; k[3] = 0;
        run_case("bucket uniform", k, k.size(), 150000, thr, NO_FALLBACK, p.form);
        run_case("bucket count below", k, 100001, 150000, thr, NO_FALLBACK, p.form);
        run_case("bucket count above", k, 1ull << 40, 149000, thr, NO_FALLBACK, p.form);
        run_case("bucket count 0", k, 0, 150000, thr, NO_FALLBACK, p.form);
        // keys on both sides of every leaf boundary
        Keys edges = uniform_keys(100000, thr, 5);
        for (uint64_t j = 1; j < p.leaves; ++j) { edges.push_back(j << p.shift); edges.push_back((j << p.shift) - 1); edges.push_back(j << p.shift); }
        run_case("bucket leaf boundaries", edges, edges.size(), 150000, thr, NO_FALLBACK, p.form);
        // leaf loads 0, 1, C - 1, C (distinct and not), the rest uniform outside those leaves; then C + 1
        for (uint32_t over = 0; over < 2; ++over) {
            Keys q;
            std::mt19937_64 g(11);
            while (q.size() < 100000) {
                const uint64_t v = uniform_key(g, thr);
                const uint64_t leaf = v >> p.shift;
                if (leaf < 5 || leaf > 9) q.push_back(v);
            }
            for (uint32_t i = 0; i < US_LEAF_CAP + over; ++i) q.push_back((5ull << p.shift) + 3 * i);
            for (uint32_t i = 0; i < US_LEAF_CAP - 1; ++i) q.push_back((6ull << p.shift) + i);
            q.push_back((7ull << p.shift) + 12345);
            for (uint32_t i = 0; i < US_LEAF_CAP; ++i) q.push_back((9ull << p.shift) + i % 3);
            std::shuffle(q.begin(), q.end(), g);
            run_case(over ? "bucket leaf load C + 1" : "bucket leaf loads 0, 1, C - 1, C", q, q.size(), 150000, thr, over ? FALLBACK : NO_FALLBACK, p.form);
        }
        run_case("bucket all equal", Keys(100000, thr / 3), 100000, 150000, thr, FALLBACK, p.form);
        Keys alt(100000);
        for (size_t i = 0; i < alt.size(); ++i) alt[i] = i & 1 ? thr : 1;
        run_case("bucket alternating", alt, alt.size(), 150000, thr, FALLBACK, p.form);
        Keys stray = uniform_keys(100000, thr, 6);
        stray[777] = thr + 1;
        run_case("bucket key above thr", stray, stray.size(), 150000, thr, FALLBACK, p.form);
        stray[777] = MAX;
        run_case("bucket key 2^64 - 1 above thr", stray, stray.size(), 150000, thr, FALLBACK, p.form);
    }
    {   // all 64 bits: keys 1 and 2^64 - 1 are legal
        Keys k = uniform_keys(40000, MAX, 21, 0.3);
        k[5] = 1; k[6] = MAX; k[7] = MAX; k[8] = MAX - 1;
        const UsPlan p = us_plan(40000, MAX);
        Result r = run_case("bucket thr 2^64 - 1", k, k.size(), 40000, MAX, NO_FALLBACK, p.form);
        CHECK(r.out.back() == MAX && r.counts.back() == 2 && r.out.front() == 1, "ends");
    }
    {   // fewer distinct values than keys in a leaf can be: thr = 40 gives 41 leaves of one value each; thr = 20 cannot hold 20,000 keys
        Keys k = uniform_keys(20000, 40, 31);
        run_case("bucket thr 40", k, k.size(), 20000, 40, NO_FALLBACK, US_ONE_PASS);
        run_case("declined thr 20", uniform_keys(20000, 20, 32), 20000, 20000, 20, FALLBACK, US_DECLINE);
        // scaled around 2^40: thr = 2^24
        run_case("bucket thr 2^24", uniform_keys(20000, 1ull << 24, 33, 0.3), 20000, 20000, 1ull << 24, NO_FALLBACK);
        run_case("bucket thr 2^24, 2 x 10^6", uniform_keys(2000000, 1ull << 24, 34), 2000000, 2000000, 1ull << 24, NO_FALLBACK, US_TWO_PASS);
    }
    {   // the size of the flagship's leaves: 2 x 10^6 hashes under the max_hash of scaled = 1000, a third drawn twice or more
        const uint64_t thr = 18446744073709551ull;
        run_case("bucket 2 x 10^6", uniform_keys(2000000, thr, 41, 0.33), 2000000, 2000000, thr, NO_FALLBACK, US_TWO_PASS);
    }
}

static int file_cases(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return 2; }
    uint64_t head[5];
    while (fread(head, 8, 5, f) == 5) {
        Keys k(head[4]);
        if (head[4] && fread(k.data(), 8, head[4], f) != head[4]) { fprintf(stderr, "short file\n"); return 2; }
        char what[64];
        snprintf(what, sizeof what, "file case %d", g_cases);
        Result r = run_case(what, k, head[1], head[0], head[2], (int)head[3]);
        printf("case %d: form %u fellback %u distinct %zu\n", g_cases - 1, r.form, r.fellback, r.out.size());
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        if (int rc = file_cases(argv[1])) return rc;
    } else {
        plan_cases();
        sort_cases();
        CHECK(g_network_runs > 50 && g_counting_runs > 10000, "both ways of sorting in LDS ran: %llu, %llu", (unsigned long long)g_network_runs,
              (unsigned long long)g_counting_runs);
    }
    printf("uniform sort ok: %d cases\n", g_cases);
    return 0;
}
