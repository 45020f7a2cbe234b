// Host build of the query index (sourmash_amd/csrc/qindex_core.hpp: table geometry, table and record fill, the match logic of both
// lookup forms) with a lane being a loop index and the device's loads being bounds-checked indexing (test-only artefact).
// tests/test_qindex_core_cpu.py compares it with np.searchsorted; tests/test_gpu_qindex.py compares the GPU with it.
//
// -DQINDEX_EMUL_OLD_GEOMETRY swaps the geometry for a copy of the one this header had before its shift was bounded, so that a test
// can show that the cases catch it (a shift of 64 for one hash >= 2^63).  That copy lives here only.
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../sourmash_amd/csrc/qindex_core.hpp"

namespace {

#if defined(QINDEX_EMUL_OLD_GEOMETRY)
void geometry(uint64_t nq, uint64_t q_max, uint32_t* shift, uint32_t* buckets) {
    uint32_t bucket_bits = 0;
    while (bucket_bits < 26 && (1ull << bucket_bits) < nq) ++bucket_bits;
    uint32_t value_bits = 0;
    while (value_bits < 64 && (q_max >> value_bits)) ++value_bits;
    *shift = value_bits > bucket_bits ? value_bits - bucket_bits : 0;
    // (a shift by 64 is undefined; what x86 and gfx950 make of it is a shift by 0, spelled out here so that the copy is defined)
    *buckets = (uint32_t)(*shift > 63 ? q_max : q_max >> *shift) + 1;
    if (*buckets < nq && *shift > 0 && bucket_bits < 26) {
        --*shift;
        *buckets = (uint32_t)(q_max >> *shift) + 1;
    }
}
#else
void geometry(uint64_t nq, uint64_t q_max, uint32_t* shift, uint32_t* buckets) { smg::qindex_geometry(nq, q_max, shift, buckets); }
#endif

// the query as the match logic sees it: Q[0 .. nq + 4) is readable, nothing else
struct QMemHost {
    const uint64_t* Q;
    uint64_t readable;
    uint64_t* violations;
    uint64_t at(uint64_t i) const {
        if (i >= readable) { ++*violations; return 0; }
        return Q[i];
    }
    void quad(uint64_t i, uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d) const {
        a = at(i); b = at(i + 1); c = at(i + 2); d = at(i + 3);
    }
};

}  // namespace

extern "C" void emul_qindex_geometry(uint64_t nq, uint64_t q_max, uint32_t* shift, uint32_t* buckets) { geometry(nq, q_max, shift, buckets); }

extern "C" void emul_qindex_geometry_many(const uint64_t* nq, const uint64_t* q_max, uint64_t n, uint32_t* shift, uint32_t* buckets) {
    for (uint64_t i = 0; i < n; ++i) geometry(nq[i], q_max[i], shift + i, buckets + i);
}

// T[0 .. buckets] and rec[0 .. buckets) (rec as 4 u64 a record: pos | cnt << 32, h0, h1, h2) for the given geometry
extern "C" void emul_qindex_build(const uint64_t* Q_padded, uint64_t nq, uint32_t shift, uint32_t buckets, uint32_t* T, uint64_t* rec) {
    // one lane per b, as many as the fill grids start: past buckets they must write nothing
    for (uint32_t b = 0; b < buckets + 300u; ++b) smg::qindex_fill_bucket(Q_padded, nq, shift, buckets, T, b);
    if (!rec) return;
    std::vector<smg::QRec> r(buckets);
    for (uint32_t b = 0; b < buckets + 300u; ++b) smg::qindex_fill_record(Q_padded, T, buckets, r.data(), b);
    for (uint32_t b = 0; b < buckets; ++b) {
        rec[4 * (uint64_t)b] = (uint64_t)r[b].pos | ((uint64_t)r[b].cnt << 32);
        for (int i = 0; i < 3; ++i) rec[4 * (uint64_t)b + 1 + i] = r[b].h[i];
    }
}

// out_pos[i] = position of probes[i] in Q, or NONE32.  form 0: the table form of q_find; 1: its record form; 2: the split record
// form with its callers' rule (the record of min(x, qmax) is loaded, the match runs with x itself, lanes with x > qmax are
// discarded).  Returns the number of reads outside Q[0 .. nq + 4), T[0 .. buckets] and rec[0 .. buckets), which must be 0;
// -1 for a geometry that no table can be built for (shift > 63 or more than 2 nq + 1 buckets) and -2 for an unknown form.
extern "C" int64_t emul_qindex_find(const uint64_t* Q_padded, uint64_t nq, const uint64_t* probes, uint64_t n, int form, uint32_t* out_pos) {
    if (form < 0 || form > 2) return -2;
    const uint64_t qmax = Q_padded[nq - 1];
    uint32_t shift = 0, buckets = 0;
    geometry(nq, qmax, &shift, &buckets);
    if (shift > 63 || (uint64_t)buckets > 2 * nq + 1 || (uint64_t)buckets != (qmax >> shift) + 1) return -1;
    std::vector<uint32_t> T((size_t)buckets + 1);
    std::vector<smg::QRec> rec(buckets);
    for (uint32_t b = 0; b <= buckets; ++b) smg::qindex_fill_bucket(Q_padded, nq, shift, buckets, T.data(), b);
    for (uint32_t b = 0; b < buckets; ++b) smg::qindex_fill_record(Q_padded, T.data(), buckets, rec.data(), b);
    uint64_t violations = 0;
    const QMemHost mem{Q_padded, nq + 4, &violations};
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t x = probes[i];
        uint32_t j = smg::NONE32;
        if (form == 0) {
            if (x <= qmax) {
                const uint64_t b = x >> shift;
                if (b + 1 > buckets) { ++violations; out_pos[i] = j; continue; }
                j = smg::q_table_match_core(mem, (uint32_t)nq, x, T[b], T[b + 1]);
            }
        } else {
            if (form == 1 && x > qmax) { out_pos[i] = j; continue; }
            const uint64_t b = (x <= qmax ? x : qmax) >> shift;
            if (b >= buckets) { ++violations; out_pos[i] = j; continue; }
            const smg::QRec& r = rec[b];
            j = smg::q_rec_match_core(mem, x, r.pos, r.cnt, r.h[0], r.h[1], r.h[2]);
            if (x > qmax) j = smg::NONE32;
        }
        out_pos[i] = j;
    }
    return (int64_t)violations;
}

#if defined(QINDEX_EMUL_MAIN)
// A program of its own, for a build with -fsanitize=address,undefined: the geometry over one hash at every bit length and over
// nq = 1 .. 5000 x every bit length of q_max (a shift by the operand's width would stop it), then tables, records and every lookup form
// over small queries with the shapes the lookups branch on, against a linear scan, with the vectors sized exactly.
#include <stdio.h>
static int check_query(const std::vector<uint64_t>& q, uint64_t* lookups) {
    std::vector<uint64_t> padded(q);
    for (int i = 0; i < 4; ++i) padded.push_back(q.back());
    std::vector<uint64_t> probes;
    for (uint64_t v : q) {
        probes.push_back(v);
        if (v > 0) probes.push_back(v - 1);
        if (v < UINT64_MAX) probes.push_back(v + 1);
    }
    for (uint64_t v : {(uint64_t)0, (uint64_t)1, (uint64_t)1 << 63, ((uint64_t)1 << 63) - 1, UINT64_MAX}) probes.push_back(v);
    std::vector<uint32_t> out(probes.size());
    for (int form = 0; form < 3; ++form) {
        if (emul_qindex_find(padded.data(), q.size(), probes.data(), probes.size(), form, out.data()) != 0) return 1;
        for (size_t i = 0; i < probes.size(); ++i) {
            uint32_t want = smg::NONE32;
            for (size_t j = 0; j < q.size(); ++j) if (q[j] == probes[i]) want = (uint32_t)j;
            if (out[i] != want) return 2;
        }
        *lookups += probes.size();
    }
    return 0;
}

int main() {
    uint64_t geometries = 0, lookups = 0;
    for (uint64_t nq = 1; nq <= 5000; ++nq)
        for (int bits = 0; bits <= 64; ++bits) {
            const uint64_t top = bits ? (uint64_t)1 << (bits - 1) : 0;
            for (uint64_t q_max : {top, top + top / 3, bits == 64 ? UINT64_MAX : (top << 1) - (bits ? 1 : 0)}) {
                if (q_max < nq - 1) continue;
                uint32_t shift = 0, buckets = 0;
                geometry(nq, q_max, &shift, &buckets);
                if (shift > 63 || (uint64_t)buckets != (q_max >> shift) + 1 || (uint64_t)buckets > 2 * nq + 1 || (shift > 0 && buckets < nq)) {
                    printf("geometry(%llu, %#llx) = shift %u, %u buckets\n", (unsigned long long)nq, (unsigned long long)q_max, shift, buckets);
                    return 1;
                }
                ++geometries;
            }
        }
    std::vector<std::vector<uint64_t>> queries;
    for (int b = 0; b < 64; ++b) queries.push_back({(uint64_t)1 << b});                         // one hash at every bit length
    queries.push_back({0});
    queries.push_back({0xAAAAAAAAAAAAAAAAull});
    queries.push_back({UINT64_MAX});
    queries.push_back({0, UINT64_MAX});
    queries.push_back({UINT64_MAX - 1, UINT64_MAX});
    for (uint64_t base : {(uint64_t)0, (uint64_t)1 << 40, UINT64_MAX - 299})                    // dense runs: shift 0, full buckets up to q_max
        for (uint64_t n : {4, 5, 7, 8, 9, 300}) {
            std::vector<uint64_t> q;
            for (uint64_t i = 0; i < n; ++i) q.push_back(base + i);
            queries.push_back(q);
        }
    for (uint64_t step : {(uint64_t)1, (uint64_t)1 << 40}) {                                       // one crowded bucket under a large shift
        std::vector<uint64_t> q;
        for (uint64_t i = 0; i < 10; ++i) q.push_back(((uint64_t)1 << 63) + i * step);
        queries.push_back(q);
    }
    for (const auto& q : queries) {
        const int bad = check_query(q, &lookups);
        if (bad) { printf("query of %zu hashes from %#llx: %s\n", q.size(), (unsigned long long)q[0], bad == 1 ? "a read out of bounds" : "a wrong position"); return 1; }
    }
    printf("ok: %llu geometries, %zu queries, %llu lookups\n", (unsigned long long)geometries, queries.size(), (unsigned long long)lookups);
    return 0;
}
#endif
