// qindex.hpp -- lookup of a u64 in a sorted query through a first-level table (device side).
// Shared by gather.hip (postings build, apply) and pair_ops.hip (overlaps of a query with every row of a CSR).
// The geometry, the fills and the match logic are qindex_core.hpp's (host and device); this header adds the device's loads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qindex_core.hpp"

namespace smg {

// Wide loads from addresses that are only 4- / 8-byte aligned.  The hardware takes them (global memory, dword
// alignment); hipcc splits them into narrower instructions unless they are spelled out.
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void load_u32_pair(const uint32_t* p, uint32_t& a, uint32_t& b) {
    u32x2_t v;
    asm volatile("global_load_dwordx2 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
    a = v.x; b = v.y;
}

__device__ __forceinline__ void load_u64_quad(const uint64_t* p, uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d) {
    u32x4_t v0, v1;
    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:16\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v0), "=&v"(v1) : "v"(p) : "memory");
    a = (uint64_t)v0.x | ((uint64_t)v0.y << 32); b = (uint64_t)v0.z | ((uint64_t)v0.w << 32);
    c = (uint64_t)v1.x | ((uint64_t)v1.y << 32); d = (uint64_t)v1.z | ((uint64_t)v1.w << 32);
}

// the query as qindex_core.hpp's match logic reads it: four entries by the two spelled-out loads, single ones plainly
struct QMemDev {
    const uint64_t* Q;
    __device__ __forceinline__ void quad(uint64_t i, uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d) const { load_u64_quad(Q + i, a, b, c, d); }
    __device__ __forceinline__ uint64_t at(uint32_t i) const { return Q[i]; }
};

// The same lookup in two steps, for callers that keep several lookups in flight: q_rec_load issues the two 16-byte loads
// of the record (plain loads: the compiler schedules the loads of independent lookups back to back and places the waits),
// q_rec_match compares.  `x` must be <= qi.qmax (callers clamp, then discard the result of clamped lanes); qi.rec != null.
struct QRecVal {
    uint4 a, b;
};
__device__ __forceinline__ QRecVal q_rec_load(const QIndex& qi, uint64_t x) {
    const uint4* p = reinterpret_cast<const uint4*>(qi.rec + (x >> qi.shift));
    QRecVal v;
    v.a = p[0];
    v.b = p[1];
    return v;
}
__device__ __forceinline__ uint32_t q_rec_match(const QIndex& qi, uint64_t x, const QRecVal& v) {
    const uint32_t pos = v.a.x, cnt = v.a.y;
    const uint64_t h0 = (uint64_t)v.a.z | ((uint64_t)v.a.w << 32), h1 = (uint64_t)v.b.x | ((uint64_t)v.b.y << 32),
                   h2 = (uint64_t)v.b.z | ((uint64_t)v.b.w << 32);
    return q_rec_match_core(QMemDev{qi.Q}, x, pos, cnt, h0, h1, h2);
}

__device__ __forceinline__ uint32_t q_find_rec(const QIndex& qi, uint64_t x) {
    return q_rec_match(qi, x, q_rec_load(qi, x));
}

// Position of x in Q, or NONE32.  The table is sized for about one query hash per bucket, so a bucket almost always
// holds <= 4: those are fetched with two 16-byte loads and compared in registers.  Three load instructions per lookup
// (table pair, two halves of the bucket): every lane of a lookup goes to a different cache line, and a CU serves such
// loads at about one line per cycle, so the number of load INSTRUCTIONS is what a lookup costs.
// Fuller buckets finish with a binary search.
__device__ __forceinline__ uint32_t q_find(const QIndex& qi, uint64_t x) {
    if (x > qi.qmax) return NONE32;
    if (qi.rec) return q_find_rec(qi, x);
    uint32_t lo, hi;
    load_u32_pair(qi.T + (x >> qi.shift), lo, hi);
    return q_table_match_core(QMemDev{qi.Q}, (uint32_t)qi.nq, x, lo, hi);
}

}  // namespace smg
