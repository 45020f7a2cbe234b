// qindex_core.hpp -- the arithmetic and the comparisons of the query index (qindex.hpp): table geometry, the fill of the table and
// of the bucket records, and the match logic of both lookup forms, over values that are already loaded.  The host and the device
// share it.  Plain C++ on the host (tests/native/qindex_emul.cpp compiles it with g++); qindex.hpp adds the device loads.
//
// The match functions read the query through a small view type `Mem`:
//     void     quad(uint64_t i, uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d) const;    // Q[i .. i + 3]
//     uint64_t at(uint32_t i) const;                                                           // Q[i]
// On the device quad() is two spelled-out 16-byte loads (qindex.hpp: QMemDev); on the host it is plain indexing with bounds checks.
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

constexpr uint32_t NONE32 = 0xffffffffu;
constexpr uint32_t QINDEX_MAX_BUCKET_BITS = 26;       // queries of more than 2^26 hashes share buckets: the table stops growing

// first-level table over the sorted query: bucket b = x >> shift covers Q[T[b], T[b+1]).  Q must be followed by 4
// readable entries (owners keep a padded copy), T has buckets + 1 entries, buckets = (qmax >> shift) + 1.
// One 32-byte record per bucket: where the bucket starts in Q, how many query hashes it holds, and the first three of
// them inline.  With about one hash per bucket a lookup is then ONE dependent step -- two independent 16-byte loads from
// the same record -- instead of table entry -> query entries; fuller buckets (2 % at one hash per bucket on average)
// finish with a binary search in Q.
struct __attribute__((aligned(32))) QRec {
    uint32_t pos, cnt;
    uint64_t h[3];
};

struct QIndex {
    const uint64_t* Q;
    uint64_t nq;
    const uint32_t* T;
    uint32_t shift;
    uint64_t qmax;
    const QRec* rec = nullptr;       // optional (owners that look up many times build it); q_find prefers it
};

// Table geometry for nq >= 1 sorted distinct hashes whose largest is q_max (so q_max >= nq - 1).  It keeps, for every such pair:
//   shift <= 63                               (x >> shift is defined for every x, a one-hash query above 2^63 included);
//   buckets == (q_max >> shift) + 1           in 64 bits, and it fits 32;
//   buckets <= 2 * nq + 1                     (callers size the table and its fill grid by 2 * nq + 2);
//   buckets >= nq  for nq <= 2^26             (between half a hash and one hash per bucket).
SMG_HD void qindex_geometry(uint64_t nq, uint64_t q_max, uint32_t* shift, uint32_t* buckets) {
    uint32_t bucket_bits = 0;
    while (bucket_bits < QINDEX_MAX_BUCKET_BITS && (1ull << bucket_bits) < nq) ++bucket_bits;
    uint32_t value_bits = 0;
    while (value_bits < 64 && (q_max >> value_bits)) ++value_bits;
    uint32_t s = value_bits > bucket_bits ? value_bits - bucket_bits : 0;
    if (s > 63) s = 63;                                   // nq == 1, q_max >= 2^63: two buckets, not a shift by the operand's width
    uint64_t n = (q_max >> s) + 1;
    // between half a hash and one hash per bucket: with up to two, one bucket in eight held more than the three hashes a
    // record carries inline (Poisson, mean 1.9) and sent its lookups into a second dependent load.  Above 2^26 hashes the table
    // has its largest size and stays there.
    if (n < nq && s > 0 && nq <= (1ull << QINDEX_MAX_BUCKET_BITS)) {
        --s;
        n = (q_max >> s) + 1;
    }
    *shift = s;
    *buckets = (uint32_t)n;
}

// T[b] = first position of Q with Q[pos] >= b << shift, for b = 0 .. n_buckets (T[n_buckets] = nq)
SMG_HD void qindex_fill_bucket(const uint64_t* __restrict__ Q, uint64_t nq, uint32_t shift, uint32_t n_buckets,
                               uint32_t* __restrict__ T, uint32_t b) {
    if (b > n_buckets) return;
    if (b == n_buckets) { T[b] = (uint32_t)nq; return; }
    const uint64_t x = (uint64_t)b << shift;
    uint64_t lo = 0, hi = nq;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (Q[mid] < x) lo = mid + 1; else hi = mid;
    }
    T[b] = (uint32_t)lo;
}

// rec[b] from the finished table: bucket b covers Q[T[b], T[b+1])
SMG_HD void qindex_fill_record(const uint64_t* __restrict__ Q, const uint32_t* __restrict__ T, uint32_t n_buckets,
                               QRec* __restrict__ rec, uint32_t b) {
    if (b >= n_buckets) return;
    const uint32_t pos = T[b], cnt = T[b + 1] - pos;
    QRec r;
    r.pos = pos;
    r.cnt = cnt;
    for (int i = 0; i < 3; ++i) r.h[i] = (uint32_t)i < cnt ? Q[pos + i] : 0ull;
    rec[b] = r;
}

// Record form: position of x in Q given the fields of x's bucket record, or NONE32.  x <= qmax.
template <class Mem>
SMG_HD uint32_t q_rec_match_core(const Mem& m, uint64_t x, uint32_t pos, uint32_t cnt, uint64_t h0, uint64_t h1, uint64_t h2) {
    uint32_t j = NONE32;
    if (cnt > 2 && h2 == x) j = pos + 2;
    if (cnt > 1 && h1 == x) j = pos + 1;
    if (cnt > 0 && h0 == x) j = pos;
    if (__builtin_expect(cnt > 3 && j == NONE32 && x > h2, 0)) {         // rare (1.5 % of the buckets hold more than three)
        uint64_t q3, q4, q5, q6;
        m.quad((uint64_t)pos + 3, q3, q4, q5, q6);                       // one more step covers buckets of up to seven
        if (q3 == x) j = pos + 3;
        else if (cnt > 4 && q4 == x) j = pos + 4;
        else if (cnt > 5 && q5 == x) j = pos + 5;
        else if (cnt > 6 && q6 == x) j = pos + 6;
        else if (cnt > 7 && x > q6) {
            uint32_t l = pos + 7, h = pos + cnt;
            const uint32_t end = h;
            while (l < h) {
                const uint32_t mid = (l + h) >> 1;
                if (m.at(mid) < x) l = mid + 1; else h = mid;
            }
            if (l < end && m.at(l) == x) j = l;
        }
    }
    return j;
}

// Table form: position of x in Q given x's bucket [lo, hi) = [T[b], T[b + 1]), or NONE32.  x <= qmax.
template <class Mem>
SMG_HD uint32_t q_table_match_core(const Mem& m, uint32_t nq, uint64_t x, uint32_t lo, uint32_t hi) {
    if (lo == hi) return NONE32;
    uint64_t q0, q1, q2, q3;
    m.quad(lo, q0, q1, q2, q3);                                      // padded: lo + 3 is always readable
    if (q0 == x) return lo;
    if (q1 == x) return lo + 1 < nq ? lo + 1 : NONE32;
    if (q2 == x) return lo + 2 < nq ? lo + 2 : NONE32;
    if (q3 == x) return lo + 3 < nq ? lo + 3 : NONE32;
    if (hi - lo <= 4) return NONE32;
    uint32_t l = lo + 4, h = hi;
    while (l < h) {
        const uint32_t mid = (l + h) >> 1;
        if (m.at(mid) < x) l = mid + 1; else h = mid;
    }
    return (l < hi && m.at(l) == x) ? l : NONE32;
}

}  // namespace smg
