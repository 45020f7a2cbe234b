// gather_rows_core.hpp compiled for the host: the rules of the gather-rows pass behind a C interface, and the whole pass as the kernels
// of gather_rows.hip walk it -- the owner pass a pick at a time, 64 hashes of the row at a time through gm_find, the tally a query
// hash at a time with the pairs emitted in an order no sort may rely on, and an UNSTABLE sort by the pair key
// (tests/test_gather_rows_core_cpu.py).  With -DGR_EMUL_MAIN it is a program of its own that runs the hand case (sanitizer builds).
#include <algorithm>
#include <vector>
#include "../../sourmash_amd/csrc/gather_rows_core.hpp"

using namespace smg;

extern "C" {

uint32_t emul_gr_block() { return GR_BLOCK; }
uint32_t emul_gr_none() { return GM_NONE; }
uint32_t emul_gr_owner_merge(uint32_t owner, uint32_t rank) { return gr_owner_merge(owner, rank); }
uint32_t emul_gr_owned(uint32_t owner) { return gr_owned(owner) ? 1u : 0u; }
uint32_t emul_gr_segment_of(const uint64_t* offsets, uint64_t m, uint64_t i) { return gr_segment_of(offsets, m, i); }
uint64_t emul_gr_pair_key(uint32_t pick, uint32_t pos) { return gr_pair_key(pick, pos); }
uint32_t emul_gr_key_pick(uint64_t key) { return gr_key_pick(key); }
uint32_t emul_gr_key_pos(uint64_t key) { return gr_key_pos(key); }
int32_t emul_gr_key_bits(uint64_t n_picks) { return gr_key_bits(n_picks); }
uint32_t emul_gr_sizes_fit(uint64_t m, uint64_t q_total, uint64_t n_rows, uint64_t n_picks) { return gr_sizes_fit(m, q_total, n_rows, n_picks) ? 1u : 0u; }
// out9: qn, scal, wide, scan, keys_a, vals_a, keys_b, sort, end
void emul_gr_layout(uint64_t m, uint64_t q_total, uint64_t n_picks, uint64_t scan_bytes, uint64_t sort_bytes, uint64_t* out9) {
    const GrLayout L = gr_layout(m, q_total, n_picks, scan_bytes, sort_bytes);
    const uint64_t v[9] = {L.qn, L.scal, L.wide, L.scan, L.keys_a, L.vals_a, L.keys_b, L.sort, L.end};
    for (int i = 0; i < 9; ++i) out9[i] = v[i];
}

// The raw entry on the host.  -> owned hashes, or UINT64_MAX - trouble bits when the offsets or a pick row are refused.
uint64_t emul_gr_rows(const uint64_t* qhashes, const uint64_t* qabunds, const uint64_t* qoffsets, uint64_t m, uint64_t q_total, const uint64_t* hashes,
                      const uint64_t* offsets, uint64_t n_rows, const uint64_t* pick_offsets, const uint32_t* pick_rows, uint64_t n_picks, uint64_t cutoff,
                      uint32_t* owner, uint32_t* orig_common, uint32_t* unique, uint64_t* weighted, uint64_t* abund_offsets, uint64_t* abund_values,
                      uint64_t* query_sizes, uint64_t* total_weighted) {
    uint32_t flag = 0;
    std::vector<uint32_t> qn(m, 0);
    for (uint64_t q = 0; q < m; ++q) {                                  // gr_prep_kernel
        const uint64_t a = qoffsets[q], b = qoffsets[q + 1];
        if (b < a || b > q_total) flag |= GR_BAD_QUERY_OFFSETS;
        else qn[q] = (uint32_t)many_cut_len(qhashes + a, b - a, cutoff);
        const uint64_t pa = pick_offsets[q], pb = pick_offsets[q + 1];
        if (pb < pa || pb > n_picks || (q == 0 && pa != 0) || (q + 1 == m && pb != n_picks)) flag |= GR_BAD_PICK_OFFSETS;
        query_sizes[q] = total_weighted[q] = 0;
    }
    for (uint64_t i = 0; i < q_total; ++i) owner[i] = GM_NONE;
    for (uint64_t p = 0; p < n_picks; ++p) unique[p] = 0, weighted[p] = 0;
    if (flag) return ~0ull - flag;
    for (uint64_t p = n_picks; p-- > 0;) {                              // gr_owner_kernel: picks in whatever order (here the last first)
        const uint32_t q = gr_segment_of(pick_offsets, m, p);
        const uint32_t rank = (uint32_t)(p - pick_offsets[q]);
        const uint64_t row = pick_rows[p];
        uint32_t count = 0;
        if (row >= n_rows) { flag |= GR_BAD_PICK_ROW; orig_common[p] = 0; continue; }
        const uint64_t* Q = qhashes + qoffsets[q];
        uint32_t* own = owner + qoffsets[q];
        if (offsets[row + 1] < offsets[row]) flag |= GR_BAD_ROW_OFFSETS;
        bool ended = false;
        for (uint64_t at0 = offsets[row]; at0 < offsets[row + 1] && !ended; at0 += 64) {
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint64_t i = at0 + lane;
                const bool valid = i < offsets[row + 1];
                const bool inside = valid && hashes[i] <= cutoff;
                if (valid && !inside) ended = true;
                const uint32_t pos = inside ? gm_find(Q, qn[q], hashes[i]) : GM_NONE;
                if (pos == GM_NONE) continue;
                own[pos] = gr_owner_merge(own[pos], rank);
                ++count;
            }
        }
        orig_common[p] = count;
    }
    if (flag) return ~0ull - flag;
    std::vector<std::pair<uint64_t, uint64_t>> pairs;                   // gr_tally_kernel: positions in whatever order (here the last first)
    const uint64_t q_begin = m ? qoffsets[0] : 0, q_end = m ? qoffsets[m] : 0;
    for (uint64_t i = q_end; i-- > q_begin;) {
        const uint32_t q = gr_segment_of(qoffsets, m, i);
        const uint32_t pos = (uint32_t)(i - qoffsets[q]);
        if (pos >= qn[q]) continue;
        const uint64_t a = qabunds ? qabunds[i] : 1;
        query_sizes[q] += 1;
        total_weighted[q] += a;
        if (!gr_owned(owner[i])) continue;
        const uint64_t pick = pick_offsets[q] + owner[i];
        if (pick >= n_picks) continue;
        unique[pick] += 1;
        weighted[pick] += a;
        pairs.push_back({gr_pair_key((uint32_t)pick, pos), a});
    }
    const uint64_t mask = gr_key_bits(n_picks) >= 64 ? ~0ull : (1ull << gr_key_bits(n_picks)) - 1ull;   // the bits the device sorts by
    std::sort(pairs.begin(), pairs.end(), [mask](const std::pair<uint64_t, uint64_t>& a, const std::pair<uint64_t, uint64_t>& b) {
        return (a.first & mask) < (b.first & mask);
    });
    for (size_t i = 0; i < pairs.size(); ++i) abund_values[i] = pairs[i].second;
    abund_offsets[0] = 0;
    for (uint64_t p = 0; p < n_picks; ++p) abund_offsets[p + 1] = abund_offsets[p] + unique[p];
    return pairs.size();
}

}  // extern "C"

#ifdef GR_EMUL_MAIN
#include <stdio.h>
// the hand case of tests/gather_rows_cases.py beside an empty query and a query with no picks; 0 when the outputs are the expected
int main() {
    const std::vector<std::vector<uint64_t>> queries = {{}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, {900, 901}};
    const std::vector<std::vector<uint64_t>> rows = {{1, 2, 3, 4, 100}, {3, 4, 5, 6, 7}, {3, 8, 9, 10, 11}, {1, 2}, {}, {500}, {12}};
    std::vector<uint64_t> qh, qoff{0}, h, off{0};
    for (const auto& q : queries) { qh.insert(qh.end(), q.begin(), q.end()); qoff.push_back(qh.size()); }
    for (const auto& r : rows) { h.insert(h.end(), r.begin(), r.end()); off.push_back(h.size()); }
    const uint64_t q_total = qh.size();
    const std::vector<uint64_t> ab = qh, pick_off = {0, 0, 4, 4};   // abundance[h] = h
    const std::vector<uint32_t> pick_rows = {1, 2, 0, 6};
    qh.push_back(0); h.push_back(0);
    std::vector<uint32_t> owner(q_total, 77), oc(4, 77), un(4, 77);
    std::vector<uint64_t> w(4, 77), aoff(5, 77), av(q_total, 77), qs(3, 77), tw(3, 77);
    const uint64_t got = emul_gr_rows(qh.data(), ab.data(), qoff.data(), 3, q_total, h.data(), off.data(), rows.size(), pick_off.data(), pick_rows.data(), 4, ~0ull,
                                      owner.data(), oc.data(), un.data(), w.data(), aoff.data(), av.data(), qs.data(), tw.data());
    const uint32_t want_oc[4] = {5, 5, 4, 1}, want_un[4] = {5, 4, 2, 1};
    const uint64_t want_w[4] = {25, 38, 3, 12}, want_av[12] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 1, 2, 12};
    bool ok = got == 12 && qs[0] == 0 && qs[1] == 12 && qs[2] == 2 && tw[1] == 78 && aoff[4] == 12;
    for (int i = 0; i < 4 && ok; ++i) ok = oc[i] == want_oc[i] && un[i] == want_un[i] && w[i] == want_w[i];
    for (int i = 0; i < 12 && ok; ++i) ok = av[i] == want_av[i];
    printf("%s: %llu owned\n", ok ? "ok" : "MISMATCH", (unsigned long long)got);
    return ok ? 0 : 1;
}
#endif
