// The value rules of setops_core.hpp compiled for the host: the filter that moves values and the merge that sums
// (sourmash_amd/csrc/setops.hip) behind a C interface (tests/test_abund_set_core_cpu.py).  Both are walked as the kernels walk
// them -- work items of a split row, chunks of a workgroup, ballots of a wave, the payload through the sorts, the split, the two
// scans, runs in chunks -- with the header's own functions at every step.
#include <algorithm>
#include <vector>
#include "../../sourmash_amd/csrc/qindex_core.hpp"
#include "../../sourmash_amd/csrc/setops_core.hpp"

using namespace smg;

namespace {

uint32_t chunk_place(const bool* keep, uint32_t* place) {
    uint64_t mask[SETOPS_WAVES];
    uint32_t wave_totals[SETOPS_WAVES];
    for (uint32_t w = 0; w < SETOPS_WAVES; ++w) {
        mask[w] = 0;
        for (uint32_t l = 0; l < 64; ++l)
            if (keep[w * 64 + l]) mask[w] |= 1ull << l;
        wave_totals[w] = setops_wave_total(mask[w]);
    }
    for (uint32_t t = 0; t < SETOPS_BLOCK; ++t) place[t] = setops_wave_base(wave_totals, t >> 6) + setops_lane_rank(mask[t >> 6], t & 63u);
    return setops_chunk_total(wave_totals);
}

struct QMemHost {
    const std::vector<uint64_t>* Q;
    mutable uint64_t* bad;
    void quad(uint64_t i, uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d) const {
        if (i + 3 >= Q->size()) { ++*bad; a = b = c = d = 0; return; }
        a = (*Q)[i]; b = (*Q)[i + 1]; c = (*Q)[i + 2]; d = (*Q)[i + 3];
    }
    uint64_t at(uint32_t i) const {
        if (i >= Q->size()) { ++*bad; return 0; }
        return (*Q)[i];
    }
};

}  // namespace

extern "C" {

uint64_t emul_abund_not_found() { return SETOPS_NOT_FOUND; }
uint64_t emul_abund_find(const uint64_t* row, uint64_t n, uint64_t x) { return setops_find(row, n, x); }
uint32_t emul_abund_in_range(uint64_t a, uint64_t lo, uint64_t hi) { return setops_in_range(a, lo, hi) ? 1u : 0u; }
uint64_t emul_abund_payload(uint64_t group, uint64_t j) { return setops_payload(group, j); }
uint64_t emul_abund_payload_group(uint64_t p) { return setops_payload_group(p); }
uint64_t emul_abund_payload_pos(uint64_t p) { return setops_payload_pos(p); }
uint64_t emul_abund_run_sum(const uint64_t* scan, uint64_t start, uint64_t count) { return setops_run_sum(scan, start, count); }
void emul_abund_modes(uint32_t* out) {
    out[0] = SETOPS_VALUES_NONE; out[1] = SETOPS_VALUES_CARRY; out[2] = SETOPS_VALUES_TAKE; out[3] = SETOPS_VALUES_RANGE;
    out[4] = SETOPS_MERGE_FLAT; out[5] = SETOPS_MERGE_SUM; out[6] = SETOPS_MERGE_COUNT;
}

// The filter in a value mode as setops_filter_count / setops_filter_write run it.  other_offsets null: one sketch behind a query
// index with records (RANGE: no other sketch at all).  stats: [0] lookups made, [1] lookups the membership rule forbids, [2] work
// items whose write disagreed with their count, [3] reads of the index outside the padded sketch, [4] work items, [5] reads of the
// other side's abundances (TAKE: one per kept hash).  -> hashes of the result.
uint64_t emul_abund_filter(const uint64_t* hashes, const uint64_t* abunds, const uint64_t* offsets, uint64_t n, const uint64_t* other_hashes,
                           const uint64_t* other_abunds, const uint64_t* other_offsets, uint64_t other_len, uint32_t keep_present, uint32_t mode,
                           uint64_t range_lo, uint64_t range_hi, uint64_t* out_hashes, uint64_t* out_abunds, uint64_t* out_offsets, uint64_t* stats) {
    for (int i = 0; i < 6; ++i) stats[i] = 0;
    out_offsets[0] = 0;
    if (n == 0) return 0;
    std::vector<uint64_t> Q;
    std::vector<uint32_t> T;
    std::vector<QRec> rec;
    uint32_t shift = 0, buckets = 0;
    uint64_t q_max = 0;
    if (!other_offsets && other_len) {
        Q.assign(other_hashes, other_hashes + other_len);
        Q.resize(other_len + 4, 0);
        q_max = Q[other_len - 1];
        qindex_geometry(other_len, q_max, &shift, &buckets);
        T.assign(buckets + 1, 0);
        rec.resize(buckets);
        for (uint32_t b = 0; b <= buckets; ++b) qindex_fill_bucket(Q.data(), other_len, shift, buckets, T.data(), b);
        for (uint32_t b = 0; b < buckets; ++b) qindex_fill_record(Q.data(), T.data(), buckets, rec.data(), b);
    }
    const QMemHost mem{&Q, &stats[3]};
    std::vector<uint64_t> piece_start(n + 1, 0);
    for (uint64_t r = 0; r < n; ++r) piece_start[r + 1] = piece_start[r] + setops_pieces(offsets[r + 1] - offsets[r]);
    const uint64_t n_items = piece_start[n];
    stats[4] = n_items;
    std::vector<uint64_t> piece_count(n_items + 1, 0), piece_base(n_items + 1, 0);
    for (int write = 0; write < 2; ++write) {
        for (uint64_t t = 0; t < n_items; ++t) {
            const uint64_t r = setops_row_of(piece_start.data(), n, t);
            const uint64_t lo = offsets[r], hi = offsets[r + 1];
            const uint64_t i0 = lo + (t - piece_start[r]) * SETOPS_SPLIT;
            const uint64_t i1 = hi - i0 > SETOPS_SPLIT ? i0 + SETOPS_SPLIT : hi;
            uint64_t o_n = other_len, o_max = q_max, plo = 0;
            const uint64_t* partner = nullptr;
            if (other_offsets) {
                plo = other_offsets[r];
                partner = other_hashes + plo;
                o_n = other_offsets[r + 1] - plo;
                o_max = o_n ? partner[o_n - 1] : 0;
            }
            uint64_t running = 0;
            for (uint64_t c = i0; c < i1; c += SETOPS_BLOCK) {
                bool keep[SETOPS_BLOCK];
                uint32_t place[SETOPS_BLOCK];
                uint64_t where[SETOPS_BLOCK];
                for (uint32_t lane = 0; lane < SETOPS_BLOCK; ++lane) {
                    const uint64_t i = c + lane;
                    keep[lane] = false;
                    where[lane] = SETOPS_NOT_FOUND;
                    if (i >= i1) continue;
                    const uint64_t x = hashes[i];
                    if (mode == SETOPS_VALUES_RANGE) {
                        keep[lane] = setops_in_range(abunds[i], range_lo, range_hi);
                        continue;
                    }
                    auto counted = [&](uint64_t v) {
                        ++stats[0];
                        if (o_n == 0 || v > o_max) ++stats[1];
                    };
                    if (mode == SETOPS_VALUES_TAKE) {
                        uint64_t w = setops_member_at(x, o_n, o_max, [&](uint64_t v) -> uint64_t {
                            counted(v);
                            if (other_offsets) return setops_find(partner, o_n, v);
                            const QRec& q = rec[v >> shift];
                            const uint32_t p = q_rec_match_core(mem, v, q.pos, q.cnt, q.h[0], q.h[1], q.h[2]);
                            return p == NONE32 ? SETOPS_NOT_FOUND : (uint64_t)p;
                        });
                        if (w != SETOPS_NOT_FOUND && other_offsets) w += plo;
                        where[lane] = w;
                        keep[lane] = w != SETOPS_NOT_FOUND;
                    } else {
                        const bool present = setops_member(x, o_n, o_max, [&](uint64_t v) {
                            counted(v);
                            if (other_offsets) return setops_search(partner, o_n, v);
                            const QRec& q = rec[v >> shift];
                            return q_rec_match_core(mem, v, q.pos, q.cnt, q.h[0], q.h[1], q.h[2]) != NONE32;
                        });
                        keep[lane] = setops_filter_keeps(present, keep_present != 0);
                    }
                }
                const uint32_t chunk_total = chunk_place(keep, place);
                if (write)
                    for (uint32_t lane = 0; lane < SETOPS_BLOCK; ++lane)
                        if (keep[lane] && running + place[lane] < piece_count[t]) {
                            const uint64_t pos = setops_out_pos(piece_base[t], running, place[lane], 0);
                            out_hashes[pos] = hashes[c + lane];
                            uint64_t taken = 0;
                            if (mode == SETOPS_VALUES_TAKE) { taken = other_abunds[where[lane]]; ++stats[5]; }
                            if (mode != SETOPS_VALUES_NONE)
                                out_abunds[pos] = setops_filter_value(mode, mode == SETOPS_VALUES_TAKE ? 0 : abunds[c + lane], taken);
                        }
                running += chunk_total;
            }
            if (!write) piece_count[t] = running;
            else if (running != piece_count[t]) ++stats[2];
        }
        if (!write)
            for (uint64_t t = 0; t < n_items; ++t) piece_base[t + 1] = piece_base[t] + piece_count[t];
    }
    for (uint64_t r = 0; r <= n; ++r) out_offsets[r] = piece_base[piece_start[r]];
    return out_offsets[n];
}

// The merge with values as setops_merge_run runs it: SUM carries (group, position) through the sorts as the payload, splits it into
// the group and the gathered abundance, and takes every run's sum from ONE inclusive scan; COUNT writes the run's length.
// force_form: 0 the core's form, 2 wide.  -> hashes of the result.
uint64_t emul_abund_merge(const uint64_t* hashes, const uint64_t* abunds, const uint64_t* offsets, uint64_t n, const uint32_t* groups, uint64_t n_groups,
                          const uint32_t* need, uint32_t need_all, uint64_t max_hash, uint64_t num, uint32_t mode, uint32_t force_form,
                          uint64_t* out_hashes, uint64_t* out_abunds, uint64_t* out_offsets) {
    for (uint64_t g = 0; g <= n_groups; ++g) out_offsets[g] = 0;
    if (n == 0 || n_groups == 0) return 0;
    const uint64_t base = offsets[0], total = offsets[n] - base;
    if (total == 0) return 0;
    const bool sum = mode == SETOPS_MERGE_SUM;
    SetopsKeyForm form = setops_key_form(max_hash, n_groups);
    if (force_form == 2) form.packed = false;
    std::vector<uint32_t> group_rows(n_groups, 0);
    for (uint64_t r = 0; r < n; ++r) ++group_rows[groups ? groups[r] : 0];
    std::vector<uint64_t> keys(total), vals(total);
    for (uint64_t j = 0; j < total; ++j) {
        const uint64_t r = setops_row_of(offsets, n, base + j);
        const uint64_t g = groups ? groups[r] : 0, h = hashes[base + j];
        keys[j] = form.packed ? setops_pack(form, g, h) : h;
        vals[j] = sum ? setops_payload(g, j) : g;
    }
    // the sorts: the packed key alone; or by hash and then, stably, by the group (of the payload: its bits above 32)
    std::vector<uint64_t> idx(total);
    for (uint64_t j = 0; j < total; ++j) idx[j] = j;
    std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return keys[a] < keys[b]; });
    if (!form.packed)
        std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) {
            const uint64_t ga = sum ? setops_payload_group(vals[a]) : vals[a], gb = sum ? setops_payload_group(vals[b]) : vals[b];
            return ga < gb;
        });
    // the split: every sorted pair's group, and its abundance gathered through the payload's position
    std::vector<uint64_t> sorted_group(total), sorted_abund(total, 0);
    for (uint64_t i = 0; i < total; ++i) {
        const uint64_t p = vals[idx[i]];
        sorted_group[i] = sum ? setops_payload_group(p) : p;
        if (sum) sorted_abund[i] = abunds[base + setops_payload_pos(p)];
    }
    std::vector<uint64_t> run_key, run_group, run_count;
    for (uint64_t i = 0; i < total; ++i) {
        const uint64_t k = keys[idx[i]], g = sorted_group[i];
        if (!run_key.empty() && run_key.back() == k && run_group.back() == g) ++run_count.back();
        else { run_key.push_back(k); run_group.push_back(g); run_count.push_back(1); }
    }
    // the two scans: inclusive over the sorted abundances (wrapping u64), exclusive over the runs' counts
    std::vector<uint64_t> scan(total), run_start(run_key.size());
    uint64_t acc = 0;
    for (uint64_t i = 0; i < total; ++i) { acc += sorted_abund[i]; scan[i] = acc; }
    acc = 0;
    for (uint64_t i = 0; i < run_key.size(); ++i) { run_start[i] = acc; acc += run_count[i]; }
    const uint64_t n_runs = run_key.size(), n_chunks = (total + SETOPS_BLOCK - 1) / SETOPS_BLOCK;
    std::vector<uint64_t> chunk_count(n_chunks + 1, 0), chunk_base(n_chunks + 1, 0), kept_hash(total), kept_abund(total);
    std::vector<uint32_t> kept_group(total);
    for (int write = 0; write < 2; ++write) {
        for (uint64_t c = 0; c < n_chunks; ++c) {
            bool keep[SETOPS_BLOCK];
            uint32_t place[SETOPS_BLOCK];
            for (uint32_t t = 0; t < SETOPS_BLOCK; ++t) {
                const uint64_t i = c * SETOPS_BLOCK + t;
                keep[t] = i < n_runs && setops_keep(run_count[i], setops_need(need, need_all, group_rows.data(), run_group[i]));
            }
            const uint32_t chunk_total = chunk_place(keep, place);
            if (!write) { chunk_count[c] = chunk_total; continue; }
            for (uint32_t t = 0; t < SETOPS_BLOCK; ++t) {
                if (!keep[t]) continue;
                const uint64_t i = c * SETOPS_BLOCK + t, pos = setops_out_pos(chunk_base[c], 0, place[t], 0);
                kept_hash[pos] = form.packed ? setops_packed_hash(form, run_key[i]) : run_key[i];
                kept_group[pos] = (uint32_t)run_group[i];
                kept_abund[pos] = setops_merge_value(mode, run_count[i], sum ? setops_run_sum(scan.data(), run_start[i], run_count[i]) : 0);
            }
        }
        if (!write)
            for (uint64_t c = 0; c < n_chunks; ++c) chunk_base[c + 1] = chunk_base[c] + chunk_count[c];
    }
    const uint64_t n_kept = chunk_base[n_chunks];
    std::vector<uint64_t> off(n_groups + 1);
    for (uint64_t g = 0; g <= n_groups; ++g) off[g] = g == n_groups ? n_kept : setops_group_start(kept_group.data(), n_kept, g);
    uint64_t at = 0;
    for (uint64_t g = 0; g < n_groups; ++g) {
        const uint64_t len = setops_num_cut(off[g + 1] - off[g], num);
        out_offsets[g] = at;
        for (uint64_t i = 0; i < len; ++i) { out_hashes[at + i] = kept_hash[off[g] + i]; out_abunds[at + i] = kept_abund[off[g] + i]; }
        at += len;
    }
    out_offsets[n_groups] = at;
    return at;
}

}  // extern "C"
