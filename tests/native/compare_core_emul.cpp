// Host walk of the all-pairs compare family with the functions of sourmash_amd/csrc/compare_core.hpp alone (test-only artefact): a
// workgroup is a loop, a lane a loop index, LDS a vector, an atomic a plain update.  A program of its own:
//
//     compare_core_emul CASE_FILE RESULT_FILE
//
// CASE_FILE (u64 words): mode, n, total, has_abund, has_nums, 8 parameters, offsets[n + 1], hashes[total], abunds[total] if any,
// nums[n] if any.  RESULT_FILE (u64 words): what the mode computes, see main().  tests/test_compare_core_cpu.py writes the cases of
// tests/compare_cases.py, runs this program plain and under the sanitizers, and compares the results with numpy.
//   mode 0  scaled counts as compare_plan_kernel + compare_hash_kernel: parameters symmetric (0 strip, 1 whole, 2 blocks), row_lo,
//           row_hi, rb_first, rb_stride, rb_count -> out_rows x n counts
//   mode 1  bottom-k as compare_ext_kernel<X_NUM> + ext_rows_kernel + num_jaccard_kernel -> common, union size, jaccard bits (n x n each)
//   mode 2  abundance walk as compare_ext_kernel<X_ABUND*>: parameter narrow -> common, prod (n x n each)
//   mode 3  abundance join as abund_pairs.hip: parameters narrow, slices (0: ap_slices_per_tile) -> common, prod (n x n each)
//   mode 4  the path choice: n rows of 6 words in `hashes` (n, total, forced threshold, one_shot, n_freq, rare_pairs) -> per row
//           threshold, t_merge bits, try_dict, try_sort, accept, words
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../sourmash_amd/csrc/compare_core.hpp"

using namespace smg;
using namespace smg::cmp_tile;
using namespace smg::ap_geom;
typedef std::vector<uint64_t> V64;

namespace {

struct Case {
    uint64_t mode = 0, n = 0, total = 0, par[8] = {0};
    V64 offsets, hashes, abunds, nums;
};

[[noreturn]] void fail(const char* what, uint64_t a = 0, uint64_t b = 0) {
    fprintf(stderr, "compare_core_emul: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    exit(1);
}

// a sketch's staged segment of a round: its next <= seg hashes
struct Staged { const uint64_t* e; uint32_t have; };
uint32_t at_or_under(const Staged& s, uint64_t bound) {
    uint32_t k = 0;
    for (uint32_t l = 0; l < s.have; ++l) k += s.e[l] <= bound;
    return k;
}

// ---- mode 0: scaled counts ------------------------------------------------------------------------------------------------------
constexpr int LOGT = 12, HT = 1 << LOGT;

struct WorkItem { uint32_t ty, cb, z, zt; };

void scaled_item(const Case& c, const WorkItem& it, int symmetric, uint32_t row_lo, uint32_t row_hi, uint32_t rb_first, uint32_t rb_stride,
                 std::vector<uint64_t>& key, std::vector<uint32_t>& mask, V64& common) {
    const uint32_t n = (uint32_t)c.n;
    const uint64_t* hashes = c.hashes.data();
    uint16_t* mask16 = reinterpret_cast<uint16_t*>(mask.data());
    const uint32_t rb = rb_first + it.ty * rb_stride;
    const uint32_t row0 = row_lo + rb * HR, col0 = it.cb * HC;
    uint64_t s_pos[HR + HC], s_end[HR + HC];
    for (int t = 0; t < HR + HC; ++t) {
        const uint32_t s = t < HR ? row0 + t : col0 + (t - HR);
        const bool ok = t < HR ? s < row_hi : s < n;
        s_pos[t] = ok ? c.offsets[s] : 0;
        s_end[t] = ok ? c.offsets[s + 1] : 0;
    }
    if (it.zt > 1) {
        uint64_t best_pos, best_len, piv_lo, piv_hi;
        cmp_longest_first(s_pos, s_end, HR + HC, &best_pos, &best_len);
        cmp_slice_pivots(hashes, best_pos, best_len, it.z, it.zt, &piv_lo, &piv_hi);
        for (int t = 0; t < HR + HC; ++t) cmp_slice_cut(hashes, s_pos[t], s_end[t], it.z, it.zt, piv_lo, piv_hi, &s_pos[t], &s_end[t]);
    }
    // sketch (i, wave) of the kernel is tile sketch i * HWAVES + wave: rows first, then columns
    uint32_t s_cnt[HR * HC] = {0}, s_top[2] = {0, 0};
    static uint32_t acc[HWAVES][64][NC / 2][4];
    memset(acc, 0, sizeof(acc));
    uint32_t since[HWAVES] = {0};
    auto flush = [&](int wave) {
        for (int lane = 0; lane < 64; ++lane)
            for (int p = 0; p < NC / 2; ++p)
                for (int k = 0; k < 4; ++k) {
                    for (int j = 0; j < 8; ++j) s_cnt[cmp_nibble_cell(p, k, j & 1, j >> 1, wave)] += (acc[wave][lane][p][k] >> (4 * j)) & 15u;
                    acc[wave][lane][p][k] = 0;
                }
        since[wave] = 0;
    };
    for (;;) {
        Staged st[HR + HC];
        uint64_t hi = ~0ull;
        uint32_t live = 0;
        for (int t = 0; t < HR + HC; ++t) {
            const uint64_t left = s_end[t] - s_pos[t];
            if (left >> 32) fail("a slice of a sketch holds 2^32 hashes or more", t);
            st[t] = Staged{hashes + s_pos[t], (uint32_t)(left < (uint64_t)HSEG ? left : (uint64_t)HSEG)};
            if (cmp_round_bounds((uint32_t)left, (uint32_t)HSEG) && st[t].e[HSEG - 1] < hi) hi = st[t].e[HSEG - 1];
            if (left) live |= t < HR ? CMP_LIVE_ROWS : CMP_LIVE_COLS;
        }
        if (!cmp_round_live(live)) break;
        const bool last = cmp_round_last(hi);
        const uint64_t cut = cmp_round_cut(hi);
        uint32_t take[HR + HC];
        for (int t = 0; t < HR + HC; ++t) {
            take[t] = cmp_round_take(last, (uint32_t)(s_end[t] - s_pos[t]), at_or_under(st[t], cut));
            if (take[t] > st[t].have) fail("a round takes more than is staged", t, take[t]);
            if (last)
                for (uint32_t l = 0; l < take[t]; ++l)
                    if (st[t].e[l] == H_EMPTY) s_top[t < HR ? 0 : 1] |= 1u << (t < HR ? t : t - HR);
        }
        // rows: insert (linear probing from the even slot), then the masks
        std::vector<uint32_t> held;
        for (int r = 0; r < HR; ++r)
            for (uint32_t l = 0; l < st[r].have; ++l) {
                const uint64_t e = st[r].e[l];
                if (!(e <= cut)) continue;
                uint32_t off = pair_slot<LOGT>(e) * 8u;
                for (int tries = 0;; ++tries) {
                    if (tries > HT) fail("the table is full");
                    if (key[off >> 3] == H_EMPTY) { key[off >> 3] = e; break; }
                    if (key[off >> 3] == e) break;
                    off = cmp_probe_next<LOGT>(off, 8u);
                }
                mask[cmp_mask_word(off)] |= (1u << r) << cmp_mask_shift(off);
                held.push_back(off);
            }
        // columns: one lookup per hash, a pair of slots per probe; the masks found go to the lanes' nibble counters
        for (int wave = 0; wave < HWAVES; ++wave) {
            bool hit = false;
            uint32_t m[64][NC];
            memset(m, 0, sizeof(m));
            for (int j = 0; j < NC; ++j) {
                const Staged& s = st[HR + j * HWAVES + wave];
                for (uint32_t l = 0; l < s.have; ++l) {
                    const uint64_t e = s.e[l];
                    if (!(e <= cut)) continue;
                    uint32_t co = pair_slot<LOGT>(e) * 8u;
                    for (int tries = 0;; ++tries) {
                        if (tries > HT) fail("a lookup does not end");
                        const uint64_t x = key[co >> 3], y = key[(co >> 3) + 1];
                        if (x == e || y == e) { m[l][j] = mask16[cmp_mask_half(co) + (y == e ? 1u : 0u)]; hit = true; break; }
                        if (y == H_EMPTY) break;
                        co = cmp_probe_next<LOGT>(co, 16u);
                    }
                }
            }
            if (!hit) continue;
            for (int lane = 0; lane < 64; ++lane)
                for (int p = 0; p < NC / 2; ++p) {
                    const uint32_t y = m[lane][2 * p] | (m[lane][2 * p + 1] << 16);
                    for (int k = 0; k < 4; ++k) acc[wave][lane][p][k] += (y >> k) & 0x11111111u;
                }
            if (++since[wave] == 15u) flush(wave);
        }
        for (uint32_t off : held) { key[off >> 3] = H_EMPTY; mask16[cmp_mask_half(off)] = 0; }
        for (int t = 0; t < HR + HC; ++t) s_pos[t] += take[t];
    }
    for (int wave = 0; wave < HWAVES; ++wave)
        if (since[wave]) flush(wave);
    for (int k = 0; k < HT; ++k)
        if (key[k] != H_EMPTY || (k < HT / 2 && mask[k])) fail("the table is not empty after a work item", k);
    for (int k = 0; k < HR * HC; ++k) {
        uint32_t cnt = s_cnt[k];
        if (((s_top[0] >> (k / HC)) & 1u) && ((s_top[1] >> (k % HC)) & 1u)) cnt += 1;
        const uint32_t r = (uint32_t)k / HC, cc = (uint32_t)k % HC, row = row0 + r, col = col0 + cc;
        if (row < row_hi && col < n && cnt) {
            const uint64_t idx = (uint64_t)(it.ty * HR + r) * n + col;
            if (!symmetric) common[idx] += cnt;
            else if (col >= row) {
                common[idx] += cnt;
                if (symmetric == 1 && col != row) common[(uint64_t)(col - row_lo) * n + row] += cnt;
            }
        }
    }
}

V64 run_scaled(const Case& c) {
    const uint32_t n = (uint32_t)c.n;
    const int symmetric = (int)c.par[0];
    const uint32_t row_lo = symmetric == 0 ? (uint32_t)c.par[1] : 0u, row_hi = symmetric == 0 ? (uint32_t)c.par[2] : n;
    const uint32_t rb_first = symmetric == 2 ? (uint32_t)c.par[3] : 0u, rb_stride = symmetric == 2 ? (uint32_t)c.par[4] : 1u;
    const uint32_t n_row_tiles = symmetric == 2 ? (uint32_t)c.par[5] : (row_hi - row_lo + CT - 1) / CT;
    const uint32_t n_col_tiles = (n + HC - 1) / HC;
    const uint64_t tiles = (uint64_t)n_row_tiles * n_col_tiles;
    const uint64_t out_rows = symmetric == 2 ? (uint64_t)n_row_tiles * CT : (uint64_t)(row_hi - row_lo);
    V64 common(out_rows * n, 0);
    const uint32_t slice_len = cmp_pick_slice_len(tiles / (symmetric ? 2 : 1));
    // the plan: heavy items (sliced tiles) are drained first
    std::vector<WorkItem> heavy, light;
    for (uint64_t t = 0; t < tiles; ++t) {
        const uint32_t ty = (uint32_t)(t / n_col_tiles), cb = (uint32_t)(t % n_col_tiles);
        const uint32_t rb = rb_first + ty * rb_stride;
        const uint32_t row0 = row_lo + rb * CT, col0 = cb * HC;
        if (symmetric && col0 + HC <= row0) continue;
        uint64_t best = 0;
        for (uint32_t i = 0; i < (uint32_t)HC; ++i) {
            const uint32_t r = row0 + i, cc = col0 + i;
            if (i < (uint32_t)CT && r < row_hi) best = std::max(best, c.offsets[r + 1] - c.offsets[r]);
            if (cc < n) best = std::max(best, c.offsets[cc + 1] - c.offsets[cc]);
        }
        if (best == 0) continue;
        const uint32_t zt = cmp_slice_count(best, slice_len, (uint32_t)CMP_ZMAX);
        for (uint32_t z = 0; z < zt; ++z) (zt > 1 ? heavy : light).push_back(WorkItem{ty, cb, z, zt});
    }
    std::vector<uint64_t> key(HT, H_EMPTY);
    std::vector<uint32_t> mask(HT / 2, 0);
    for (const auto* list : {&heavy, &light})
        for (const WorkItem& it : *list) scaled_item(c, it, symmetric, row_lo, row_hi, rb_first, rb_stride, key, mask, common);
    return common;
}

// ---- modes 1 and 2: the tiles of compare_ext_kernel -----------------------------------------------------------------------------
// MODE 0 num, 1 abundances of 32 bits, 2 of 64
void run_ext(const Case& c, int MODE, V64& common, V64& prod) {
    const uint32_t n = (uint32_t)c.n, nt = (n + XT - 1) / XT;
    const uint64_t* hashes = c.hashes.data();
    const bool ABUND = MODE != 0;
    const uint32_t slice_len = ABUND ? cmp_ext_slice_len(nt * (nt + 1) / 2) : XSLICE;
    for (uint32_t rt = 0; rt < nt; ++rt)
        for (uint32_t ct = rt; ct < nt; ++ct)
            for (uint32_t z = 0; z < (ABUND ? (uint32_t)XZMAX : 1u); ++z) {
                const uint32_t row0 = rt * XT, col0 = ct * XT;
                uint64_t s_pos[2 * XT], s_end[2 * XT];
                for (int t = 0; t < 2 * XT; ++t) {
                    const uint32_t s = t < XT ? row0 + t : col0 + (t - XT);
                    s_pos[t] = s < n ? c.offsets[s] : 0;
                    s_end[t] = s < n ? c.offsets[s + 1] : 0;
                }
                if (ABUND) {
                    uint64_t best_pos, best_len, piv_lo, piv_hi;
                    cmp_longest_first(s_pos, s_end, 2 * XT, &best_pos, &best_len);
                    const uint32_t zt = cmp_slice_count(best_len, slice_len, (uint32_t)XZMAX);
                    if (z >= zt) continue;
                    if (zt > 1) {
                        cmp_slice_pivots(hashes, best_pos, best_len, z, zt, &piv_lo, &piv_hi);
                        for (int t = 0; t < 2 * XT; ++t) cmp_slice_cut(hashes, s_pos[t], s_end[t], z, zt, piv_lo, piv_hi, &s_pos[t], &s_end[t]);
                    }
                }
                uint32_t cnt[XT][XT] = {{0}}, steps[XT][XT] = {{0}};
                unsigned long long acc[XT][XT] = {{0}};
                for (;;) {
                    Staged st[2 * XT];
                    uint64_t hi = ~0ull;
                    uint32_t live = 0;
                    for (int t = 0; t < 2 * XT; ++t) {
                        const uint64_t left = s_end[t] - s_pos[t];
                        if (left >> 32) fail("the cases keep a sketch below 2^32 hashes", t);
                        st[t] = Staged{hashes + s_pos[t], (uint32_t)(left < (uint64_t)XSEG ? left : (uint64_t)XSEG)};
                        if (cmp_round_bounds((uint32_t)left, (uint32_t)XSEG)) hi = std::min(hi, st[t].e[XSEG - 1]);
                        if (st[t].have) live |= t < XT ? CMP_LIVE_ROWS : CMP_LIVE_COLS;
                    }
                    if (!cmp_round_live(live)) break;
                    uint32_t take[2 * XT];
                    for (int t = 0; t < 2 * XT; ++t) take[t] = at_or_under(st[t], hi);   // (2^64 - 1 is an ordinary hash here)
                    for (int r = 0; r < XT; ++r)
                        for (int cc = 0; cc < XT; ++cc) {
                            const uint32_t row = row0 + r, col = col0 + cc;
                            if (!(row < n && col < n && col > row)) continue;
                            const uint32_t na = take[r], nb = take[XT + cc];
                            if (MODE == 0) {
                                ext_num_walk(st[r].e, na, st[XT + cc].e, nb, (uint32_t)c.nums[row], &cnt[r][cc], &steps[r][cc]);
                            } else {
                                const uint64_t *WA = c.abunds.data() + s_pos[r], *WB = c.abunds.data() + s_pos[XT + cc];
                                uint32_t ia = 0, ib = 0;
                                while (ia < na && ib < nb) {
                                    if (MODE == 1) ext_abund_step<uint32_t>(st[r].e[ia], st[XT + cc].e[ib], (uint32_t)WA[ia], (uint32_t)WB[ib], &ia, &ib, &cnt[r][cc], &acc[r][cc]);
                                    else ext_abund_step<uint64_t>(st[r].e[ia], st[XT + cc].e[ib], WA[ia], WB[ib], &ia, &ib, &cnt[r][cc], &acc[r][cc]);
                                }
                            }
                        }
                    for (int t = 0; t < 2 * XT; ++t) s_pos[t] += take[t];
                }
                for (int r = 0; r < XT; ++r)
                    for (int cc = 0; cc < XT; ++cc) {
                        const uint32_t row = row0 + r, col = col0 + cc;
                        if (!(row < n && col < n && col > row)) continue;
                        common[(uint64_t)row * n + col] += cnt[r][cc]; common[(uint64_t)col * n + row] += cnt[r][cc];
                        if (ABUND) { prod[(uint64_t)row * n + col] += acc[r][cc]; prod[(uint64_t)col * n + row] += acc[r][cc]; }
                    }
            }
}

// the diagonal, as ext_rows_kernel: a sketch's size and its sum of squared abundances
void ext_rows(const Case& c, V64& common, V64* prod) {
    for (uint64_t s = 0; s < c.n; ++s) {
        common[s * c.n + s] = c.offsets[s + 1] - c.offsets[s];
        if (!prod) continue;
        unsigned long long t = 0;
        for (uint64_t p = c.offsets[s]; p < c.offsets[s + 1]; ++p) t += (unsigned long long)c.abunds[p] * c.abunds[p];
        (*prod)[s * c.n + s] = t;
    }
}

// ---- mode 3: the abundance join -------------------------------------------------------------------------------------------------
void run_join(const Case& c, bool narrow, uint32_t z_forced, V64& common, V64& prod) {
    const uint32_t n = (uint32_t)c.n, nb = (n + AP_T - 1) / AP_T;
    const uint64_t total = c.total, tiles = (uint64_t)nb * (nb + 1) / 2;
    const uint64_t* hashes = c.hashes.data();
    if (total == 0) return;
    // plan and cuts
    const uint32_t s_max = ap_s_max(total, nb);
    uint64_t max_hash = 0;
    for (uint32_t r = 0; r < n; ++r)
        if (c.offsets[r + 1] > c.offsets[r]) max_hash = std::max(max_hash, hashes[c.offsets[r + 1] - 1]);
    const ApPlan plan = ap_plan(max_hash, s_max);
    if (plan.shift > 63 || plan.n_slices > s_max || plan.n_slices < 1) fail("plan out of range", plan.shift, plan.n_slices);
    std::vector<uint32_t> cuts((uint64_t)n * (s_max + 1u));
    for (uint32_t r = 0; r < n; ++r)
        for (uint32_t s = 0; s <= s_max; ++s)
            cuts[(uint64_t)r * (s_max + 1u) + s] = ap_cut(hashes + c.offsets[r], (uint32_t)(c.offsets[r + 1] - c.offsets[r]), s, plan);
    // the lists: one (block, slice) at a time, placed by both branches of ap_slice_kernel, which must agree
    V64 l_hash(total, 0), l_ab(total, 0);
    std::vector<uint8_t> l_row(total, 0), written(total, 0);
    for (uint32_t b = 0; b < nb; ++b)
        for (uint32_t s = 0; s < plan.n_slices; ++s) {
            const uint32_t r0 = b * AP_T, nr = std::min(n - r0, (uint32_t)AP_T);
            uint32_t c0[AP_T], len[AP_T], tot = 0;
            uint64_t below = 0;
            for (uint32_t t = 0; t < nr; ++t) {
                const uint64_t at = (uint64_t)(r0 + t) * (s_max + 1u) + s;
                c0[t] = cuts[at]; len[t] = cuts[at + 1] - c0[t];
                below += c0[t]; tot += len[t];
            }
            if (tot == 0) continue;
            const uint64_t out0 = c.offsets[r0] + below, base = (uint64_t)s << plan.shift;
            // the ranking branch (any size): entries of the other rows' parts in front (equal hashes: the earlier rows') + own index
            V64 place;
            for (uint32_t rr = 0; rr < nr; ++rr)
                for (uint32_t i = 0; i < len[rr]; ++i) {
                    const uint64_t h = hashes[c.offsets[r0 + rr] + c0[rr] + i];
                    uint64_t rank = i;
                    for (uint32_t o = 0; o < nr; ++o) {
                        if (o == rr) continue;
                        const uint64_t* other = hashes + c.offsets[r0 + o] + c0[o];
                        uint32_t lo = 0, hi = len[o];
                        while (lo < hi) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (other[mid] < h || (other[mid] == h && o < rr)) lo = mid + 1; else hi = mid;
                        }
                        rank += lo;
                    }
                    place.push_back(out0 + rank);
                }
            if (tot <= (uint32_t)SM_CAP) {              // the LDS branch: sub-buckets, then the rank within the bucket
                std::vector<uint32_t> cnt(SM_BUCKETS, 0), start(SM_BUCKETS + 1, 0);
                for (uint32_t rr = 0; rr < nr; ++rr)
                    for (uint32_t i = 0; i < len[rr]; ++i) {
                        const uint32_t k = ap_bucket(hashes[c.offsets[r0 + rr] + c0[rr] + i], base, plan.shift);
                        if (k >= (uint32_t)SM_BUCKETS) fail("bucket out of range", k, s);
                        ++cnt[k];
                    }
                for (int k = 0; k < SM_BUCKETS; ++k) start[k + 1] = start[k] + cnt[k];
                size_t at = 0;
                for (uint32_t rr = 0; rr < nr; ++rr)
                    for (uint32_t i = 0; i < len[rr]; ++i, ++at) {
                        const uint64_t h = hashes[c.offsets[r0 + rr] + c0[rr] + i];
                        const uint32_t k = ap_bucket(h, base, plan.shift);
                        uint32_t rank = 0;                  // entries of the bucket with a smaller (hash, row)
                        for (uint32_t o = 0; o < nr; ++o)
                            for (uint32_t j = 0; j < len[o]; ++j) {
                                const uint64_t hj = hashes[c.offsets[r0 + o] + c0[o] + j];
                                if (ap_bucket(hj, base, plan.shift) == k && (hj < h || (hj == h && o < rr))) ++rank;
                            }
                        if (out0 + start[k] + rank != place[at]) fail("the two branches of the slice merge disagree", out0 + start[k] + rank, place[at]);
                    }
            }
            size_t at = 0;
            for (uint32_t rr = 0; rr < nr; ++rr)
                for (uint32_t i = 0; i < len[rr]; ++i, ++at) {
                    const uint64_t src = c.offsets[r0 + rr] + c0[rr] + i, o = place[at];
                    if (o >= total || o < c.offsets[r0] || o >= c.offsets[std::min(r0 + (uint32_t)AP_T, n)]) fail("a list entry outside its block's list", o);
                    if (written[o]++) fail("a list position written twice", o);
                    l_hash[o] = hashes[src]; l_ab[o] = narrow ? (uint64_t)(uint32_t)c.abunds[src] : c.abunds[src]; l_row[o] = (uint8_t)rr;
                }
        }
    for (uint64_t o = 0; o < total; ++o)
        if (!written[o]) fail("a list position never written", o);
    for (uint32_t b = 0; b < nb; ++b)
        for (uint64_t o = c.offsets[b * AP_T] + 1; o < c.offsets[std::min((b + 1) * (uint32_t)AP_T, n)]; ++o)
            if (l_hash[o - 1] > l_hash[o] || (l_hash[o - 1] == l_hash[o] && l_row[o - 1] >= l_row[o])) fail("a block's list is not ordered by (hash, row)", o);
    // the join
    uint32_t Z = ap_slices_per_tile(tiles);
    if (z_forced >= 1 && z_forced <= (uint32_t)AP_ZMAX) Z = z_forced;
    if (Z < 1 || Z > (uint32_t)AP_ZMAX) fail("slices per tile out of range", Z);
    std::vector<uint32_t> a_taken(total), b_staged(total);
    V64 staged(AP_CHUNK);
    for (uint64_t tile = 0; tile < tiles; ++tile) {
        uint32_t bi, bj;
        ap_tile_of((uint32_t)tile, nb, &bi, &bj);
        if (!(bi <= bj && bj < nb)) fail("tile out of the triangle", bi, bj);
        const bool diag = bi == bj;
        const uint32_t row0 = bi * AP_T, col0 = bj * AP_T;
        const uint32_t ra_end = std::min(row0 + (uint32_t)AP_T, n), rb_end = std::min(col0 + (uint32_t)AP_T, n);
        const uint64_t A0 = c.offsets[row0], A1 = c.offsets[ra_end], B0 = c.offsets[col0], B1 = c.offsets[rb_end];
        std::fill(a_taken.begin() + A0, a_taken.begin() + A1, 0u);
        std::fill(b_staged.begin() + B0, b_staged.begin() + B1, 0u);
        std::vector<unsigned long long> s_prod(AP_T * AP_TS, 0);
        std::vector<uint32_t> s_cnt(AP_T * AP_TS, 0);
        for (uint32_t z = 0; z < Z; ++z) {
            uint64_t bound[4];
            ap_slice_bounds(l_hash.data(), A0, A1, B0, B1, z, Z, bound);
            uint64_t a_cur = bound[0], b_cur = bound[2];
            const uint64_t a_end = bound[1], b_end = bound[3];
            if (a_cur < A0 || a_end > A1 || a_cur > a_end || b_cur < B0 || b_end > B1 || b_cur > b_end) fail("slice bounds out of the lists", tile, z);
            auto add = [&](uint32_t row_a, unsigned long long aa, uint32_t j) {
                const uint32_t rb = l_row[b_cur + j];
                if (diag && rb <= row_a) return;
                s_prod[row_a * AP_TS + rb] += aa * (unsigned long long)l_ab[b_cur + j];
                s_cnt[row_a * AP_TS + rb] += 1u;
            };
            while (a_cur < a_end && b_cur < b_end) {
                uint64_t nb_stage = std::min(b_end - b_cur, (uint64_t)AP_CHUNK);
                for (uint64_t i = 0; i < (uint64_t)AP_CHUNK; ++i) staged[i] = b_cur + i < b_end ? l_hash[b_cur + i] : ~0ull;
                nb_stage = ap_trim_to_runs(staged.data(), nb_stage, b_cur + nb_stage < b_end);
                if (nb_stage == 0) fail("a chunk trimmed to nothing", tile, b_cur);
                for (uint64_t i = 0; i < nb_stage; ++i) ++b_staged[b_cur + i];
                const uint64_t hi = staged[nb_stage - 1];
                for (;;) {
                    std::vector<uint32_t> work;
                    std::vector<unsigned long long> wpay;
                    uint32_t took = 0;
                    for (uint32_t tid = 0; tid < (uint32_t)AP_THREADS; ++tid) {
                        const uint64_t idx = a_cur + tid;
                        const uint64_t h = idx < a_end ? l_hash[idx] : ~0ull;
                        const bool mine = h <= hi && idx < a_end;
                        const uint32_t lo = ap_find(staged.data(), h);
                        if (!mine) continue;
                        ++took;
                        ++a_taken[idx];
                        if (lo < (uint32_t)nb_stage && staged[lo] == h) {
                            const uint32_t cnt = ap_run_len(staged.data(), lo, (uint32_t)nb_stage, h);
                            if (cnt > (uint32_t)AP_T) fail("a run longer than a block", cnt);
                            if (cnt <= (uint32_t)AP_INLINE) {
                                for (uint32_t j = lo; j < lo + cnt; ++j) add(l_row[idx], l_ab[idx], j);
                            } else {
                                work.push_back(ap_work_pack(lo, cnt, l_row[idx]));
                                wpay.push_back(l_ab[idx]);
                            }
                        }
                    }
                    for (size_t w = 0; w < work.size(); ++w) {
                        uint32_t lo, cnt, row_a;
                        ap_work_unpack(work[w], &lo, &cnt, &row_a);
                        for (uint32_t o = 0; o < cnt; ++o) add(row_a, wpay[w], lo + o);
                    }
                    a_cur += took;
                    if (took < (uint32_t)AP_THREADS) break;
                }
                b_cur += nb_stage;
            }
        }
        // every list position that can meet a partner was visited once; none twice
        auto has = [&](uint64_t lo, uint64_t hi, uint64_t h) { const uint64_t p = lower_bound_u64(l_hash.data(), lo, hi, h); return p < hi && l_hash[p] == h; };
        for (uint64_t p = A0; p < A1; ++p) {
            if (a_taken[p] > 1) fail("list A: a position visited twice", p, tile);
            if (a_taken[p] == 0 && has(B0, B1, l_hash[p])) fail("list A: a position with a partner not visited at all", p, tile);
        }
        for (uint64_t p = B0; p < B1; ++p) {
            if (b_staged[p] > 1) fail("list B: a position visited twice", p, tile);
            if (b_staged[p] == 0 && has(A0, A1, l_hash[p])) fail("list B: a position with a partner not visited at all", p, tile);
        }
        for (int i = 0; i < AP_T * AP_T; ++i) {
            const uint32_t r = row0 + (uint32_t)i / AP_T, cc = col0 + (uint32_t)i % AP_T;
            if (r >= n || cc >= n || (diag && cc <= r)) continue;
            const unsigned long long p = s_prod[((uint32_t)i / AP_T) * AP_TS + (uint32_t)i % AP_T];
            const uint32_t k = s_cnt[((uint32_t)i / AP_T) * AP_TS + (uint32_t)i % AP_T];
            prod[(uint64_t)r * n + cc] += p; prod[(uint64_t)cc * n + r] += p;
            common[(uint64_t)r * n + cc] += k; common[(uint64_t)cc * n + r] += k;
        }
    }
}

V64 read_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) fail("cannot open the case file");
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    V64 w((size_t)bytes / 8);
    if (bytes % 8 || fread(w.data(), 8, w.size(), f) != w.size()) fail("short case file");
    fclose(f);
    return w;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) fail("usage: compare_core_emul CASE_FILE RESULT_FILE");
    const V64 w = read_file(argv[1]);
    if (w.size() < 13) fail("case file without a header");
    Case c;
    c.mode = w[0]; c.n = w[1]; c.total = w[2];
    const bool has_abund = w[3] != 0, has_nums = w[4] != 0;
    for (int i = 0; i < 8; ++i) c.par[i] = w[5 + i];
    size_t at = 13;
    auto take = [&](V64& dst, uint64_t count) {
        if (at + count > w.size()) fail("case file shorter than its header says");
        dst.assign(w.begin() + at, w.begin() + at + count);
        at += count;
    };
    V64 out;
    if (c.mode == 4) {
        take(c.hashes, c.n * 6);
        for (uint64_t i = 0; i < c.n; ++i) {
            const uint64_t* r = &c.hashes[i * 6];
            const ComparePathModel m = compare_path_model((uint32_t)r[0], r[1], (uint32_t)r[2], r[3] != 0);
            const CompareIndexAccept a = compare_index_accept((uint32_t)r[0], r[4], r[5], r[1], m.t_merge, r[2] != 0);
            uint64_t bits;
            memcpy(&bits, &m.t_merge, 8);
            for (uint64_t v : {(uint64_t)m.threshold, bits, (uint64_t)m.try_dict, (uint64_t)m.try_sort, (uint64_t)a.accept, (uint64_t)a.words}) out.push_back(v);
        }
    } else {
        take(c.offsets, c.n + 1);
        if (c.offsets[0] != 0 || c.offsets[c.n] != c.total) fail("offsets do not span the hashes");
        take(c.hashes, c.total);
        if (has_abund) take(c.abunds, c.total);
        if (has_nums) take(c.nums, c.n);
        const uint64_t n = c.n;
        if (c.mode == 0) {
            out = run_scaled(c);
        } else if (c.mode == 1) {
            if (!has_nums) fail("bottom-k needs nums");
            V64 common(n * n, 0), none;
            run_ext(c, 0, common, none);
            ext_rows(c, common, nullptr);
            out = common;
            V64 jac;
            for (uint64_t i = 0; i < n; ++i)
                for (uint64_t j = 0; j < n; ++j) {
                    const uint64_t cm = common[i * n + j];
                    const uint64_t u = num_union_size(c.offsets[i + 1] - c.offsets[i], c.offsets[j + 1] - c.offsets[j], cm, (uint32_t)c.nums[std::min(i, j)], i == j);
                    out.push_back(u);
                    const double v = i == j ? 1.0 : jaccard_of(cm, u);
                    uint64_t bits;
                    memcpy(&bits, &v, 8);
                    jac.push_back(bits);
                }
            out.insert(out.end(), jac.begin(), jac.end());
        } else if (c.mode == 2 || c.mode == 3) {
            if (!has_abund) fail("the abundance modes need abundances");
            V64 common(n * n, 0), prod(n * n, 0);
            if (c.mode == 2) run_ext(c, c.par[0] ? 1 : 2, common, prod);
            else run_join(c, c.par[0] != 0, (uint32_t)c.par[1], common, prod);
            ext_rows(c, common, &prod);
            out = common;
            out.insert(out.end(), prod.begin(), prod.end());
        } else fail("unknown mode", c.mode);
        if (c.mode == 0 && c.par[6]) {                   // ... and the Jaccard of the counts, as jaccard_from_counts_kernel (whole matrix only)
            V64 jac;
            for (uint64_t i = 0; i < n; ++i)
                for (uint64_t j = 0; j < n; ++j) {
                    const double v = i == j ? 1.0 : jaccard_scaled(out[i * n + j], c.offsets[i + 1] - c.offsets[i], c.offsets[j + 1] - c.offsets[j]);
                    uint64_t bits;
                    memcpy(&bits, &v, 8);
                    jac.push_back(bits);
                }
            out.insert(out.end(), jac.begin(), jac.end());
        }
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 8, out.size(), f) != out.size() || fclose(f) != 0) fail("cannot write the result file");
    printf("ok: mode %llu, %llu sketches, %llu result words\n", (unsigned long long)c.mode, (unsigned long long)c.n, (unsigned long long)out.size());
    return 0;
}
