// gather_many_core.hpp compiled for the host: the rules of the many-queries gather behind a C interface, and the whole pipeline as
// the kernels of gather_many.hip walk it -- the fill 64 hashes at a time with the places a ballot would give, the pairs of the
// inverted lists through one stable sort, the rounds with the packed key and the test-and-clear of the bitmap
// (tests/test_gather_many_core_cpu.py).  With -DGM_EMUL_MAIN it is a program of its own that runs a small case (sanitizer builds).
#include <algorithm>
#include <vector>
#include "../../sourmash_amd/csrc/gather_many_core.hpp"

using namespace smg;

extern "C" {

uint32_t emul_gm_block() { return GM_BLOCK; }
uint32_t emul_gm_max_query_hashes() { return GM_MAX_QUERY_HASHES; }
uint32_t emul_gm_max_candidates() { return GM_MAX_CANDIDATES; }
uint32_t emul_gm_lds_limit() { return GM_LDS_LIMIT; }
uint32_t emul_gm_lds_static() { return GM_LDS_STATIC; }
uint64_t emul_gm_batch_common() { return GM_BATCH_COMMON; }
uint64_t emul_gm_lds_bytes(uint32_t query_hashes, uint32_t candidates) { return gm_lds_bytes(query_hashes, candidates); }
uint32_t emul_gm_caps_fit(uint32_t mqh, uint32_t mc) { return gm_caps_fit(mqh, mc) ? 1u : 0u; }
uint32_t emul_gm_status(uint64_t nq, uint64_t nc, uint32_t mqh, uint32_t mc) { return gm_status(nq, nc, mqh, mc); }
uint32_t emul_gm_find(const uint64_t* Q, uint32_t n, uint64_t h) { return gm_find(Q, n, h); }
uint64_t emul_gm_pick_key(uint32_t count, uint32_t candidate) { return gm_pick_key(count, candidate); }
uint32_t emul_gm_key_count(uint64_t key) { return gm_key_count(key); }
uint32_t emul_gm_key_candidate(uint64_t key) { return gm_key_candidate(key); }
uint32_t emul_gm_stop(uint64_t key, uint64_t threshold_hashes) { return gm_stop(key, threshold_hashes) ? 1u : 0u; }
uint32_t emul_gm_bitmap_init_word(uint32_t word, uint32_t n) { return gm_bitmap_init_word(word, n); }
uint32_t emul_gm_test_and_clear(uint32_t* bitmap, uint32_t pos) { return gm_test_and_clear(bitmap, pos) ? 1u : 0u; }
uint32_t emul_gm_inv_start(const uint64_t* keys, uint32_t lo, uint32_t hi, uint64_t key) { return gm_inv_start(keys, lo, hi, key); }
int32_t emul_gm_key_bits(uint64_t q_span) { return gm_key_bits(q_span); }
uint64_t emul_gm_batch_end(const uint64_t* weight, uint64_t m, uint64_t q_lo, uint64_t budget) { return gm_batch_end(weight, m, q_lo, budget); }

// The raw entry on the host.  Hits ordered by (query, row); the picks of query q go to [its first hit, + out_rounds[q]) of out_rows /
// out_isect, status[q] = 1 and nothing else for a query beyond a cap.  fpos_out / inv_out (may be null; room for the sum of
// common): the forward CSR and the candidates of the inverted lists as the sort leaves them.  -> rounds of all queries, or
// UINT64_MAX when a hit's slice of the forward CSR did not come out `common` long.
uint64_t emul_gm_gather(const uint64_t* qhashes, const uint64_t* qoffsets, uint64_t m, const uint64_t* hashes, const uint64_t* offsets, uint64_t n_rows,
                        const uint32_t* hit_queries, const uint32_t* hit_rows, const uint32_t* hit_common, uint64_t n_hits, uint64_t cutoff,
                        uint64_t threshold_hashes, uint32_t max_query_hashes, uint32_t max_candidates, uint32_t* out_rows, uint32_t* out_isect,
                        uint32_t* out_rounds, uint32_t* status, uint32_t* fpos_out, uint32_t* inv_out) {
    const uint32_t mqh = max_query_hashes ? max_query_hashes : GM_MAX_QUERY_HASHES, mc = max_candidates ? max_candidates : GM_MAX_CANDIDATES;
    std::vector<uint32_t> qlo(m + 1), qn(m);
    for (uint64_t q = 0; q < m; ++q) {
        qlo[q] = (uint32_t)gm_lower_bound32(hit_queries, n_hits, q);
        qn[q] = (uint32_t)many_cut_len(qhashes + qoffsets[q], qoffsets[q + 1] - qoffsets[q], cutoff);
    }
    qlo[m] = (uint32_t)gm_lower_bound32(hit_queries, n_hits, m);
    for (uint64_t q = 0; q < m; ++q) {
        status[q] = gm_status(qn[q], qlo[q + 1] - qlo[q], mqh, mc);
        if (!status[q]) out_rounds[q] = 0;
    }
    // the slices of the forward CSR: an exclusive scan of the hits' common counts (0 for a query that does not run)
    std::vector<uint64_t> foff(n_hits + 1, 0);
    for (uint64_t h = 0; h < n_hits; ++h) foff[h + 1] = foff[h] + (status[hit_queries[h]] ? 0 : hit_common[h]);
    const uint64_t total = foff[n_hits];
    std::vector<uint32_t> fpos(total);
    std::vector<std::pair<uint64_t, uint64_t>> pairs(total);
    bool flag = false;
    for (uint64_t h = 0; h < n_hits; ++h) {
        const uint32_t q = hit_queries[h];
        if (status[q]) continue;
        const uint64_t row = hit_rows[h], start = foff[h], len = foff[h + 1] - start;
        if (row >= n_rows) { flag = true; continue; }
        const uint64_t* Q = qhashes + qoffsets[q];
        const uint64_t base_key = qoffsets[q] - qoffsets[0];
        uint64_t written = 0;
        bool bad = false, ended = false;
        for (uint64_t at0 = offsets[row]; at0 < offsets[row + 1] && !bad && !ended; at0 += 64) {
            uint32_t pos[64];
            uint64_t mask = 0;
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint64_t i = at0 + lane;
                const bool valid = i < offsets[row + 1];
                const bool inside = valid && hashes[i] <= cutoff;
                pos[lane] = inside ? gm_find(Q, qn[q], hashes[i]) : GM_NONE;
                if (pos[lane] != GM_NONE) mask |= 1ull << lane;
                if (valid && !inside) ended = true;
            }
            for (uint32_t lane = 0; lane < 64; ++lane) {
                if (!(mask >> lane & 1)) continue;
                const uint64_t at = written + (uint64_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
                if (at < len) {
                    fpos[start + at] = pos[lane];
                    pairs[start + at] = {gm_inv_key(base_key, pos[lane]), h - qlo[q]};
                }
            }
            written += (uint64_t)__builtin_popcountll(mask);
            if (written > len) bad = true;
        }
        if (bad || written != len) flag = true;
    }
    if (flag) return ~0ull;
    std::stable_sort(pairs.begin(), pairs.end(), [](const std::pair<uint64_t, uint64_t>& a, const std::pair<uint64_t, uint64_t>& b) { return a.first < b.first; });
    std::vector<uint64_t> keys(total);
    for (uint64_t i = 0; i < total; ++i) {
        keys[i] = pairs[i].first;
        if (fpos_out) fpos_out[i] = fpos[i];
        if (inv_out) inv_out[i] = (uint32_t)pairs[i].second;
    }
    uint64_t all_rounds = 0;
    for (uint64_t q = 0; q < m; ++q) {
        const uint32_t h0 = qlo[q], nc = qlo[q + 1] - h0, n = qn[q];
        if (status[q] || nc == 0) continue;
        std::vector<uint32_t> cnt(hit_common + h0, hit_common + h0 + nc), bits(gm_bitmap_words(n));
        for (uint32_t w = 0; w < bits.size(); ++w) bits[w] = gm_bitmap_init_word(w, n);
        const uint32_t seg_lo = (uint32_t)foff[h0], seg_hi = (uint32_t)foff[h0 + nc];
        const uint64_t base_key = qoffsets[q] - qoffsets[0];
        uint32_t rounds = 0;
        while (rounds < nc) {
            uint64_t best = 0;
            for (uint32_t i = 0; i < nc; ++i) best = std::max(best, gm_pick_key(cnt[i], i));
            if (gm_stop(best, threshold_hashes)) break;
            const uint32_t win = gm_key_candidate(best);
            out_rows[h0 + rounds] = hit_rows[h0 + win];
            out_isect[h0 + rounds] = gm_key_count(best);
            ++rounds;
            for (uint64_t i = foff[h0 + win]; i < foff[h0 + win + 1]; ++i) {
                const uint32_t pos = fpos[i];
                if (!gm_test_and_clear(bits.data(), pos)) continue;
                const uint64_t k = gm_inv_key(base_key, pos);
                for (uint32_t j = gm_inv_start(keys.data(), seg_lo, seg_hi, k); j < seg_hi && keys[j] == k; ++j) --cnt[pairs[j].second];
            }
        }
        out_rounds[q] = rounds;
        all_rounds += rounds;
    }
    return all_rounds;
}

}  // extern "C"

#ifdef GM_EMUL_MAIN
#include <stdio.h>
// the hand case of tests/gather_many_cases.py beside an empty query and a query with no candidate; 0 when the picks are the expected
int main() {
    const std::vector<std::vector<uint64_t>> queries = {{}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, {900, 901}};
    const std::vector<std::vector<uint64_t>> rows = {{1, 2, 3, 4, 100}, {3, 4, 5, 6, 7}, {3, 8, 9, 10, 11}, {1, 2}, {}, {500}, {12}};
    std::vector<uint64_t> qh, qoff{0}, h, off{0};
    for (const auto& q : queries) { qh.insert(qh.end(), q.begin(), q.end()); qoff.push_back(qh.size()); }
    for (const auto& r : rows) { h.insert(h.end(), r.begin(), r.end()); off.push_back(h.size()); }
    qh.push_back(0); h.push_back(0);
    std::vector<uint32_t> hq, hr, hc;
    for (uint32_t q = 0; q < queries.size(); ++q)
        for (uint32_t r = 0; r < rows.size(); ++r) {
            uint32_t c = 0;
            for (uint64_t v : rows[r]) c += (uint32_t)std::count(queries[q].begin(), queries[q].end(), v);
            if (c) { hq.push_back(q); hr.push_back(r); hc.push_back(c); }
        }
    std::vector<uint32_t> out_rows(hq.size(), 77), out_isect(hq.size(), 77), rounds(3, 77), status(3, 77);
    const uint64_t got = emul_gm_gather(qh.data(), qoff.data(), 3, h.data(), off.data(), rows.size(), hq.data(), hr.data(), hc.data(), hq.size(), ~0ull, 0, 0, 0,
                                        out_rows.data(), out_isect.data(), rounds.data(), status.data(), nullptr, nullptr);
    const uint32_t want_rows[4] = {1, 2, 0, 6}, want_isect[4] = {5, 4, 2, 1};
    bool ok = got == 4 && rounds[0] == 0 && rounds[1] == 4 && rounds[2] == 0;
    for (int i = 0; i < 4 && ok; ++i) ok = out_rows[i] == want_rows[i] && out_isect[i] == want_isect[i];
    printf("%s: %llu rounds\n", ok ? "ok" : "MISMATCH", (unsigned long long)got);
    return ok ? 0 : 1;
}
#endif
