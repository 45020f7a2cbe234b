// setops_core.hpp compiled for the host: the rules of the set algebra kernels (sourmash_amd/csrc/setops.hip) behind a C interface
// (tests/test_setops_core_cpu.py).  The merge and the filter are walked as the kernels walk them -- pairs, sorts, runs, chunks of a
// workgroup, ballots of a wave, work items of a split row -- with the header's own functions at every step.
#include <algorithm>
#include <vector>
#include "../../sourmash_amd/csrc/qindex_core.hpp"
#include "../../sourmash_amd/csrc/setops_core.hpp"

using namespace smg;

namespace {

// the ordered compaction of one chunk: keep[0, SETOPS_BLOCK) -> place[i] of the kept lanes, -> the chunk's total
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

// the other sketch as the match logic reads it: a padded copy, bounds checked
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

uint32_t emul_setops_block() { return SETOPS_BLOCK; }
uint32_t emul_setops_lds_partner() { return SETOPS_LDS_PARTNER; }
uint64_t emul_setops_split() { return SETOPS_SPLIT; }
uint32_t emul_setops_bits(uint64_t x) { return setops_bits(x); }
uint64_t emul_setops_pieces(uint64_t len) { return setops_pieces(len); }
uint64_t emul_setops_num_cut(uint64_t len, uint64_t num) { return setops_num_cut(len, num); }
uint64_t emul_setops_row_of(const uint64_t* offsets, uint64_t n, uint64_t i) { return setops_row_of(offsets, n, i); }

// out: hbits, gbits, packed
void emul_setops_key_form(uint64_t max_hash, uint64_t n_groups, uint32_t* out) {
    const SetopsKeyForm f = setops_key_form(max_hash, n_groups);
    out[0] = f.hbits; out[1] = f.gbits; out[2] = f.packed ? 1u : 0u;
}

// The merge as setops_merge_run runs it.  force_form: 0 the core's form, 2 wide whatever the core says.  out_hashes: room for
// the input's hashes; out_offsets: n_groups + 1.  -> hashes of the result.
uint64_t emul_setops_merge(const uint64_t* hashes, const uint64_t* offsets, uint64_t n, const uint32_t* groups, uint64_t n_groups, const uint32_t* need,
                           uint32_t need_all, uint64_t max_hash, uint64_t num, uint32_t force_form, uint64_t* out_hashes, uint64_t* out_offsets) {
    for (uint64_t g = 0; g <= n_groups; ++g) out_offsets[g] = 0;
    if (n == 0 || n_groups == 0) return 0;
    const uint64_t base = offsets[0], total = offsets[n] - base;
    if (total == 0) return 0;
    SetopsKeyForm form = setops_key_form(max_hash, n_groups);
    if (force_form == 2) form.packed = false;
    std::vector<uint32_t> group_rows(n_groups, 0);
    for (uint64_t r = 0; r < n; ++r) ++group_rows[groups ? groups[r] : 0];
    // assign: a pair per input hash, its row found in the offsets
    std::vector<uint64_t> keys(total), vals(total);
    for (uint64_t j = 0; j < total; ++j) {
        const uint64_t r = setops_row_of(offsets, n, base + j);
        const uint64_t g = groups ? groups[r] : 0, h = hashes[base + j];
        keys[j] = form.packed ? setops_pack(form, g, h) : h;
        vals[j] = g;
    }
    // order by (group, hash): one sort of the packed key, or two stable ones, by hash and then by group
    std::vector<uint64_t> idx(total);
    for (uint64_t j = 0; j < total; ++j) idx[j] = j;
    std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return keys[a] < keys[b]; });
    if (!form.packed) std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return vals[a] < vals[b]; });
    // runs of equal pairs
    std::vector<uint64_t> run_key, run_group, run_count;
    for (uint64_t j = 0; j < total; ++j) {
        const uint64_t k = keys[idx[j]], g = vals[idx[j]];
        if (!run_key.empty() && run_key.back() == k && run_group.back() == g) ++run_count.back();
        else { run_key.push_back(k); run_group.push_back(g); run_count.push_back(1); }
    }
    // keep by ordered compaction, a chunk at a time: count, scan, write
    const uint64_t n_runs = run_key.size(), n_chunks = (total + SETOPS_BLOCK - 1) / SETOPS_BLOCK;
    std::vector<uint64_t> chunk_count(n_chunks + 1, 0), chunk_base(n_chunks + 1, 0), kept_hash(total);
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
            }
        }
        if (!write)
            for (uint64_t c = 0; c < n_chunks; ++c) chunk_base[c + 1] = chunk_base[c] + chunk_count[c];
    }
    const uint64_t n_kept = chunk_base[n_chunks];
    std::vector<uint64_t> off(n_groups + 1);
    for (uint64_t g = 0; g <= n_groups; ++g) off[g] = g == n_groups ? n_kept : setops_group_start(kept_group.data(), n_kept, g);
    // the num cut: the first num of every row
    uint64_t at = 0;
    for (uint64_t g = 0; g < n_groups; ++g) {
        const uint64_t len = setops_num_cut(off[g + 1] - off[g], num);
        out_offsets[g] = at;
        for (uint64_t i = 0; i < len; ++i) out_hashes[at + i] = kept_hash[off[g] + i];
        at += len;
    }
    out_offsets[n_groups] = at;
    return at;
}

// The filter as setops_filter_count / setops_filter_write run it.  other_offsets null: one sketch other_hashes[0, other_len) behind a
// query index with records; otherwise row r against row r of the second set.  stats: [0] lookups made, [1] lookups made for a hash
// above the other sketch's largest or in an empty one (the rule forbids them), [2] work items whose write disagreed with their
// count, [3] reads of the index outside the padded sketch, [4] work items.  -> hashes of the result.
uint64_t emul_setops_filter(const uint64_t* hashes, const uint64_t* offsets, uint64_t n, const uint64_t* other_hashes, const uint64_t* other_offsets,
                            uint64_t other_len, uint32_t keep_present, uint64_t* out_hashes, uint64_t* out_offsets, uint64_t* stats) {
    for (int i = 0; i < 5; ++i) stats[i] = 0;
    out_offsets[0] = 0;
    if (n == 0) return 0;
    // the one sketch's index
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
    // work items
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
            uint64_t o_n = other_len, o_max = q_max;
            const uint64_t* partner = nullptr;
            if (other_offsets) {
                partner = other_hashes + other_offsets[r];
                o_n = other_offsets[r + 1] - other_offsets[r];
                o_max = o_n ? partner[o_n - 1] : 0;
            }
            uint64_t running = 0;
            for (uint64_t c = i0; c < i1; c += SETOPS_BLOCK) {
                bool keep[SETOPS_BLOCK];
                uint32_t place[SETOPS_BLOCK];
                for (uint32_t lane = 0; lane < SETOPS_BLOCK; ++lane) {
                    const uint64_t i = c + lane;
                    keep[lane] = false;
                    if (i >= i1) continue;
                    const uint64_t x = hashes[i];
                    const bool present = setops_member(x, o_n, o_max, [&](uint64_t v) {
                        ++stats[0];
                        if (o_n == 0 || v > o_max) ++stats[1];
                        if (other_offsets) return setops_search(partner, o_n, v);
                        const QRec& q = rec[v >> shift];
                        return q_rec_match_core(mem, v, q.pos, q.cnt, q.h[0], q.h[1], q.h[2]) != NONE32;
                    });
                    keep[lane] = setops_filter_keeps(present, keep_present != 0);
                }
                const uint32_t chunk_total = chunk_place(keep, place);
                if (write)
                    for (uint32_t lane = 0; lane < SETOPS_BLOCK; ++lane)
                        if (keep[lane] && running + place[lane] < piece_count[t]) out_hashes[setops_out_pos(piece_base[t], running, place[lane], 0)] = hashes[c + lane];
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

}  // extern "C"
