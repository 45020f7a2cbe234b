// gather_rows.hip -- from the picks of gather to the integers of its result rows, for many queries at once.
//
// GPU counterpart of what the reference's GatherDatabases evaluates per round on MinHash objects and dictionaries
// (src/sourmash/search.py:877-949, GatherResult.build_gather_result :480-505): |original query ∩ match|, |remaining query ∩ match|,
// the sum of the query's abundances over the latter, and the abundances themselves in hash order.  Given the picks of every query
// in rank order (gather.hip or gather_many.hip found them) three steps over data that is already resident:
//   owner   a wave per pick walks the picked row and looks its hashes up in the pick's query (gm_find_group: the loads of a step
//           are independent); a found position takes the pick's rank with an atomicMin that returns nothing, and a popcount of the
//           matches is the pick's overlap with the ORIGINAL query.  The lowest rank that holds a hash owns it: that is "remaining
//           query ∩ match", because the whole match leaves the query each round.
//   tally   a lane per query hash: an owned hash counts for its pick (u32 and u64 atomic adds) and emits the pair (pick, position in
//           the query) -> abundance; the query's abundance sum at the cutoff is reduced per workgroup (its size at the cutoff is
//           known since the preparation).
//   sort    the pairs by their key: the abundances of a pick's hashes stand together in ascending hash order.
// No LDS tables, so no cap on the size of a query.  gather_rows_core.hpp holds the rules.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include "device_api.hpp"
#include "gather_rows_core.hpp"
#include "wavemask.hpp"

namespace smg {

namespace {

// Per query: its hashes <= cutoff (kept for the passes and written as query_sizes), its abundance sum zeroed, and whether its offsets (query and picks) can be walked at all.
__global__ __launch_bounds__(256) void gr_prep_kernel(const uint64_t* __restrict__ qhashes, const uint64_t* __restrict__ qoffsets, uint64_t m, uint64_t q_total,
                                                      const uint64_t* __restrict__ pick_offsets, uint64_t n_picks, uint64_t cutoff,
                                                      uint32_t* __restrict__ qn, uint64_t* __restrict__ query_sizes,
                                                      uint64_t* __restrict__ total_weighted, uint32_t* __restrict__ flag) {
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < m; q += (uint64_t)gridDim.x * 256u) {
        const uint64_t a = qoffsets[q], b = qoffsets[q + 1];
        uint32_t bad = 0, n = 0;
        if (b < a || b > q_total) bad |= GR_BAD_QUERY_OFFSETS;
        else n = (uint32_t)many_cut_len(qhashes + a, b - a, cutoff);
        const uint64_t pa = pick_offsets[q], pb = pick_offsets[q + 1];
        if (pb < pa || pb > n_picks || (q == 0 && pa != 0) || (q + 1 == m && pb != n_picks)) bad |= GR_BAD_PICK_OFFSETS;
        qn[q] = n;
        query_sizes[q] = n;
        total_weighted[q] = 0;
        if (bad) atomicOr(flag, bad);
    }
}

// The owner pass.  A wave takes a pick by ticket and walks its row's hashes <= cutoff in groups of 64, GM_FILL_UNROLL groups side by
// side, as gm_fill_kernel does; a match lowers the owner of its query hash to the pick's rank and is counted by a ballot.
__global__ __launch_bounds__(GR_BLOCK) void gr_owner_kernel(const uint64_t* __restrict__ qhashes, const uint64_t* __restrict__ qoffsets, uint64_t m,
                                                            const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ offsets, uint64_t n_rows,
                                                            const uint64_t* __restrict__ pick_offsets, const uint32_t* __restrict__ pick_rows,
                                                            uint64_t n_picks, uint64_t cutoff, const uint32_t* __restrict__ qn,
                                                            uint32_t* __restrict__ owner, uint32_t* __restrict__ orig_common,
                                                            unsigned long long* __restrict__ ticket, uint32_t* __restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    if (*flag) return;                                                 // offsets that cannot be walked: nothing runs
    for (;;) {
        unsigned long long t = 0;
        if (lane == 0) t = atomicAdd(ticket, 1ull);
        const uint64_t p = uniform64(t);
        if (p >= n_picks) break;
        const uint32_t q = gr_segment_of(pick_offsets, m, p);
        const uint32_t rank = (uint32_t)(p - pick_offsets[q]);
        const uint64_t row = pick_rows[p];
        uint32_t count = 0;
        if (row >= n_rows) {
            if (lane == 0) atomicOr(flag, GR_BAD_PICK_ROW);
        } else {
            const uint64_t q_lo = qoffsets[q];
            const uint64_t* Q = qhashes + q_lo;
            uint32_t* own = owner + q_lo;
            const uint32_t n = qn[q];
            const uint64_t lo = offsets[row], hi = offsets[row + 1];
            if (hi < lo && lane == 0) atomicOr(flag, GR_BAD_ROW_OFFSETS);
            for (uint64_t at0 = lo; at0 < hi; at0 += 64u * GM_FILL_UNROLL) {
                uint64_t v[GM_FILL_UNROLL];
                uint32_t pos[GM_FILL_UNROLL];
                bool inside[GM_FILL_UNROLL], past = false;
                GM_UNROLL for (int k = 0; k < GM_FILL_UNROLL; ++k) {
                    const uint64_t i = at0 + 64u * (uint32_t)k + lane;
                    const bool valid = i < hi;
                    v[k] = valid ? hashes[i] : 0;
                    inside[k] = valid && v[k] <= cutoff;
                    past = past || (valid && !inside[k]);
                }
                gm_find_group<GM_FILL_UNROLL>(Q, n, v, pos);
                GM_UNROLL for (int k = 0; k < GM_FILL_UNROLL; ++k) {
                    const bool match = inside[k] && pos[k] != GM_NONE;
                    if (match) atomicMin(&own[pos[k]], rank);          // (gr_owner_merge; the old value is not asked for)
                    count += (uint32_t)__popcll(mask_of(match));
                }
                if (mask_of(past)) break;                              // ascending: the row ends here at the common scaled
            }
        }
        if (lane == 0) orig_common[p] = count;
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// The tally pass.  A lane per query hash, a workgroup per 256 consecutive positions of the flat query array.  What the lanes of the
// workgroup's FIRST query add to its abundance sum goes through LDS and leaves as one atomic; a lane of a later query (queries
// shorter than a workgroup) adds for itself.  The pairs of a wave take their slots with one returning atomic.
__global__ __launch_bounds__(GR_BLOCK) void gr_tally_kernel(const uint64_t* __restrict__ qabunds, const uint64_t* __restrict__ qoffsets, uint64_t m,
                                                            const uint64_t* __restrict__ pick_offsets, uint64_t n_picks,
                                                            const uint32_t* __restrict__ qn, const uint32_t* __restrict__ owner,
                                                            uint32_t* __restrict__ unique, unsigned long long* __restrict__ weighted,
                                                            unsigned long long* __restrict__ total_weighted,
                                                            uint64_t* __restrict__ keys, uint64_t* __restrict__ vals,
                                                            unsigned long long* __restrict__ emitted, const uint32_t* __restrict__ flag) {
    __shared__ uint32_t s_q;
    __shared__ unsigned long long s_sum;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    if (*flag) return;
    const uint64_t q_begin = qoffsets[0], q_end = qoffsets[m];
    for (uint64_t base = (uint64_t)blockIdx.x * GR_BLOCK; base < q_end; base += (uint64_t)gridDim.x * GR_BLOCK) {
        if (tid == 0) { s_q = GM_NONE; s_sum = 0; }
        __syncthreads();
        const uint64_t i = base + tid;
        const bool valid = i >= q_begin && i < q_end;
        uint32_t q = GM_NONE, pos = 0;
        bool inside = false;
        unsigned long long a = 0;
        if (valid) {
            q = gr_segment_of(qoffsets, m, i);
            pos = (uint32_t)(i - qoffsets[q]);
            inside = pos < qn[q];
            a = qabunds ? qabunds[i] : 1ull;
            if (tid == 0 || i == q_begin) s_q = q;                     // the one first valid lane of the workgroup
        }
        __syncthreads();
        const uint32_t q0 = s_q;
        const bool first = inside && q == q0;
        const unsigned long long s = wave_sum(first ? a : 0ull);
        if (lane == 0 && s) atomicAdd(&s_sum, s);
        if (inside && !first) atomicAdd(&total_weighted[q], a);
        // the owned hashes: counted for their pick, and emitted
        const uint32_t o = inside ? owner[i] : GM_NONE;
        const uint64_t pick = inside && gr_owned(o) ? pick_offsets[q] + o : n_picks;
        const bool owned = pick < n_picks;
        const uint64_t mask = mask_of(owned);
        if (mask) {
            unsigned long long t = 0;
            if (lane == 0) t = atomicAdd(emitted, (unsigned long long)__popcll(mask));
            const uint64_t slot = uniform64(t) + (uint64_t)__popcll(mask & below);
            if (owned) {
                atomicAdd(&unique[pick], 1u);
                atomicAdd(&weighted[pick], a);
                keys[slot] = gr_pair_key((uint32_t)pick, pos);
                vals[slot] = a;
            }
        }
        __syncthreads();
        if (tid == 0 && q0 != GM_NONE && s_sum) atomicAdd(&total_weighted[q0], s_sum);
        __syncthreads();                                               // the LDS words are free for the next 256 positions
    }
}

// wide[p] = unique[p] as u64 for the scan that places the picks' abundances; wide[n_picks] = 0
__global__ __launch_bounds__(256) void gr_widen_kernel(const uint32_t* __restrict__ unique, uint64_t n_picks, uint64_t* __restrict__ wide) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p <= n_picks; p += (uint64_t)gridDim.x * 256u) wide[p] = p < n_picks ? unique[p] : 0;
}

unsigned blocks_for(uint64_t n, unsigned cap = 2048) {
    const uint64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

size_t scan_bytes(uint64_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)(n ? n : 1), rocprim::plus<uint64_t>(),
                                  (hipStream_t)0);
    return bytes;
}

GrLayout layout(uint64_t m, uint64_t q_total, uint64_t n_picks) {
    return gr_layout(m, q_total, n_picks, scan_bytes(n_picks + 1), sort_pairs_temp_bytes(q_total ? q_total : 1));
}

struct Stamp {
    hipEvent_t ev = nullptr;
    ~Stamp() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t mark(bool on, hipStream_t st) {
        if (!on) return hipSuccess;
        hipError_t e = hipEventCreate(&ev);
        return e != hipSuccess ? e : hipEventRecord(ev, st);
    }
};

}  // namespace

size_t gather_rows_workspace_bytes(uint64_t m, uint64_t q_total, uint64_t n_picks) { return layout(m, q_total, n_picks).end; }

hipError_t gather_rows_run(const GatherRowsArgs& a, uint64_t* n_owned, uint32_t* trouble, float* ms3, hipStream_t st) {
    if (!n_owned || !trouble) return hipErrorInvalidValue;
    *n_owned = 0;
    *trouble = 0;
    if (ms3) ms3[0] = ms3[1] = ms3[2] = 0.f;
    if (!gr_sizes_fit(a.m, a.q_total, a.n_rows, a.n_picks) || a.grid > (1u << 20)) return hipErrorInvalidValue;
    const GrLayout L = layout(a.m, a.q_total, a.n_picks);
    if (!a.d_workspace || a.workspace_bytes < L.end) return hipErrorInvalidValue;
    char* ws = static_cast<char*>(a.d_workspace);
    uint32_t* qn = (uint32_t*)(ws + L.qn);
    unsigned long long *ticket = (unsigned long long*)(ws + L.scal), *emitted = ticket + 1;
    uint32_t* flag = (uint32_t*)(ticket + 2);
    uint64_t *wide = (uint64_t*)(ws + L.wide), *keys_a = (uint64_t*)(ws + L.keys_a), *vals_a = (uint64_t*)(ws + L.vals_a), *keys_b = (uint64_t*)(ws + L.keys_b);
    const bool timed = ms3 != nullptr;
    Stamp t0, t1, t2, t3;
    hipError_t e;

    // ---- the owner pass
    if ((e = t0.mark(timed, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(ws + L.scal, 0, 256, st)) != hipSuccess) return e;
    if (a.q_total && (e = hipMemsetAsync(a.d_owner, 0xff, a.q_total * 4, st)) != hipSuccess) return e;   // GM_NONE
    if (a.n_picks) {
        if ((e = hipMemsetAsync(a.d_unique, 0, a.n_picks * 4, st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(a.d_weighted, 0, a.n_picks * 8, st)) != hipSuccess) return e;
    }
    if (a.m) {
        hipLaunchKernelGGL(gr_prep_kernel, dim3(blocks_for(a.m)), dim3(256), 0, st, a.d_qhashes, a.d_qoffsets, a.m, a.q_total, a.d_pick_offsets, a.n_picks,
                           a.cutoff, qn, a.d_query_sizes, a.d_total_weighted, flag);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.m && a.n_picks) {
        const unsigned grid = a.grid ? a.grid : blocks_for(a.n_picks * 64u);         // a wave a pick, four waves a workgroup
        hipLaunchKernelGGL(gr_owner_kernel, dim3(grid), dim3(GR_BLOCK), 0, st, a.d_qhashes, a.d_qoffsets, a.m, a.d_hashes, a.d_offsets, a.n_rows,
                           a.d_pick_offsets, a.d_pick_rows, a.n_picks, a.cutoff, qn, a.d_owner, a.d_orig_common, ticket, flag);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = t1.mark(timed, st)) != hipSuccess) return e;

    // ---- the tally pass, and where the abundances of every pick will stand
    if (a.m && a.q_total) {
        const unsigned grid = a.grid ? a.grid : blocks_for(a.q_total, 4096);
        hipLaunchKernelGGL(gr_tally_kernel, dim3(grid), dim3(GR_BLOCK), 0, st, a.d_qabunds, a.d_qoffsets, a.m, a.d_pick_offsets, a.n_picks, qn, a.d_owner,
                           a.d_unique, (unsigned long long*)a.d_weighted, (unsigned long long*)a.d_total_weighted,
                           keys_a, vals_a, emitted, flag);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gr_widen_kernel, dim3(blocks_for(a.n_picks + 1)), dim3(256), 0, st, a.d_unique, a.n_picks, wide);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t sb = scan_bytes(a.n_picks + 1);
    if ((e = rocprim::exclusive_scan(ws + L.scan, sb, (const uint64_t*)wide, a.d_abund_offsets, (uint64_t)0, (size_t)(a.n_picks + 1), rocprim::plus<uint64_t>(),
                                     st)) != hipSuccess)
        return e;
    if ((e = t2.mark(timed, st)) != hipSuccess) return e;
    uint64_t head[3] = {0, 0, 0};                                      // (ticket), pairs emitted, trouble
    if ((e = hipMemcpyAsync(head, ws + L.scal, 24, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if ((uint32_t)head[2]) { *trouble = (uint32_t)head[2]; return hipSuccess; }
    const uint64_t pairs = head[1];
    if (pairs > a.q_total) return hipErrorUnknown;                     // (a hash is owned at most once)

    // ---- the pair sort: the abundances of a pick stand together, in ascending hash order.  The workspace holds what a sort of
    // q_total pairs asks for; what this sort of `pairs` <= q_total asks for is looked up again and has to fit into that.
    const size_t sort_bytes = sort_pairs_temp_bytes(pairs ? pairs : 1);
    if (sort_bytes > sort_pairs_temp_bytes(a.q_total ? a.q_total : 1)) return hipErrorUnknown;
    if ((e = sort_pairs(keys_a, keys_b, vals_a, a.d_abund_values, pairs, gr_key_bits(a.n_picks), ws + L.sort, sort_bytes, st)) != hipSuccess) return e;
    if ((e = t3.mark(timed, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    *n_owned = pairs;
    if (timed) {
        (void)hipEventElapsedTime(&ms3[0], t0.ev, t1.ev);
        (void)hipEventElapsedTime(&ms3[1], t1.ev, t2.ev);
        (void)hipEventElapsedTime(&ms3[2], t2.ev, t3.ev);
    }
    return hipSuccess;
}

}  // namespace smg
