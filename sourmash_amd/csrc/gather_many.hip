// gather_many.hip -- the min-set-cover loop of gather for MANY small queries at once, one workgroup per query, its state in LDS.
//
// GPU counterpart of the reference's loop of GatherDatabases over many queries (src/sourmash/search.py:877-949 around
// CounterGather, src/sourmash/index/__init__.py:735-909).  In front of it stand the hits of the many-queries pass
// (overlap_many.hip): (query, row, common) of every pair that can ever be picked, ordered by (query, row).  A query's hits are its
// CANDIDATES, numbered in row order.  From them:
//   fpos   a forward CSR: per hit, the positions in the query of the hashes the row holds, ascending (gm_fill_kernel; the slice
//          of a hit is `common` long, so an exclusive scan of `common` places it),
//   inv    the inverted lists: per query hash, the candidates that hold it -- one stable pair sort of (position among all query
//          hashes, candidate), read through a binary search for the first pair of a position,
// and then the rounds (gm_rounds_kernel): a workgroup takes a query, keeps a counter per candidate and the uncovered hashes as a
// bitmap in LDS, and per round picks the largest counter (ties: lowest row), walks the winner's fpos slice, clears every bit that
// was still set and lowers the counter of every candidate holding that hash.  Work per query: sum of common + rounds x candidates.
// gather_many_core.hpp holds the rules.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include "device_api.hpp"
#include "gather_many_core.hpp"
#include "gather_parts.hpp"
#include "wavemask.hpp"

namespace smg {

namespace {

// Per query q of [0, m): its hits [qlo[q], qlo[q + 1]) among the hits ordered by query (query numbers start at q_base), its hashes
// <= cutoff, whether the LDS form takes it; for those it takes, rounds = 0 and the launch's largest sizes in maxes[0 .. 1].
// sums (may be null): the sum of common over its hits.
__global__ __launch_bounds__(256) void gm_prep_kernel(const uint64_t* __restrict__ qhashes, const uint64_t* __restrict__ qoffsets, uint64_t m,
                                                      uint32_t q_base, const uint32_t* __restrict__ hit_queries,
                                                      const uint32_t* __restrict__ hit_common, uint64_t n_hits, uint64_t cutoff,
                                                      uint32_t max_query_hashes, uint32_t max_candidates, uint32_t* __restrict__ qlo,
                                                      uint32_t* __restrict__ qn, uint32_t* __restrict__ status, uint32_t* __restrict__ out_rounds,
                                                      unsigned long long* __restrict__ sums, uint32_t* __restrict__ maxes) {
    __shared__ unsigned long long s_sum;
    const uint32_t tid = threadIdx.x;
    for (uint64_t q = blockIdx.x; q < m; q += gridDim.x) {
        if (tid == 0) s_sum = 0;
        __syncthreads();
        const uint64_t lo = gm_lower_bound32(hit_queries, n_hits, (uint64_t)q_base + q);
        const uint64_t hi = gm_lower_bound32(hit_queries, n_hits, (uint64_t)q_base + q + 1);
        if (sums) {
            unsigned long long local = 0;
            for (uint64_t i = lo + tid; i < hi; i += 256u) local += hit_common[i];
            if (local) atomicAdd(&s_sum, local);
        }
        __syncthreads();
        if (tid == 0) {
            const uint64_t a = qoffsets[q], b = qoffsets[q + 1];
            const uint64_t n = many_cut_len(qhashes + a, b - a, cutoff);
            const uint32_t st = gm_status(n, hi - lo, max_query_hashes, max_candidates);
            qlo[q] = (uint32_t)lo;
            if (q + 1 == m) qlo[m] = (uint32_t)hi;
            qn[q] = n < 0xffffffffull ? (uint32_t)n : 0xffffffffu;
            status[q] = st;
            if (!st) {
                if (out_rounds) out_rounds[q] = 0;
                if (maxes) { atomicMax(&maxes[0], (uint32_t)n); atomicMax(&maxes[1], (uint32_t)(hi - lo)); }
            }
            if (sums) sums[q] = s_sum;
        }
        __syncthreads();
    }
}

// w[h] = entries the forward CSR holds for hit h: its common count, 0 where its query is left to the one-query path; w[n_hits] = 0
__global__ __launch_bounds__(256) void gm_weights_kernel(const uint32_t* __restrict__ hit_queries, const uint32_t* __restrict__ hit_common,
                                                         uint64_t n_hits, uint32_t q_base, uint64_t m, const uint32_t* __restrict__ status,
                                                         uint64_t* __restrict__ w) {
    for (uint64_t h = (uint64_t)blockIdx.x * 256u + threadIdx.x; h <= n_hits; h += (uint64_t)gridDim.x * 256u) {
        uint64_t v = 0;
        if (h < n_hits) {
            const uint64_t q = (uint64_t)hit_queries[h] - q_base;      // (a hit of a query outside [q_base, q_base + m) holds nothing)
            if (hit_queries[h] >= q_base && q < m && !status[q]) v = hit_common[h];
        }
        w[h] = v;
    }
}

// The forward CSR and the pairs of the inverted lists.  A wave takes a hit by ticket and walks the row's hashes <= cutoff in groups
// of 64, GM_FILL_UNROLL groups side by side: a lane looks its hashes up in the query's ascending prefix in step (gm_find_group),
// so that a step of the search is that many independent loads.  The positions of the matches are written in ascending order: a
// ballot gives every matching lane its place, so the content does not depend on timing.  The hit's slice is foff[h + 1] - foff[h]
// = common long; a wave that would write past it, or ends short of it, writes nothing more and raises *flag.
__global__ __launch_bounds__(GM_BLOCK) void gm_fill_kernel(const uint64_t* __restrict__ qhashes, const uint64_t* __restrict__ qoffsets, uint64_t m,
                                                           uint32_t q_base, const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ offsets,
                                                           uint64_t n_rows, const uint32_t* __restrict__ hit_queries,
                                                           const uint32_t* __restrict__ hit_rows, uint64_t n_hits, uint64_t cutoff,
                                                           const uint32_t* __restrict__ qlo, const uint32_t* __restrict__ qn,
                                                           const uint32_t* __restrict__ status, const uint64_t* __restrict__ foff,
                                                           uint32_t* __restrict__ fpos, uint64_t* __restrict__ keys, uint64_t* __restrict__ vals,
                                                           unsigned long long* __restrict__ ticket, uint32_t* __restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t q_first = qoffsets[0];
    for (;;) {
        unsigned long long t = 0;
        if (lane == 0) t = atomicAdd(ticket, 1ull);
        const uint64_t h = uniform64(t);
        if (h >= n_hits) break;
        const uint64_t q = (uint64_t)hit_queries[h] - q_base;
        if (hit_queries[h] < q_base || q >= m || status[q]) continue;
        const uint64_t row = hit_rows[h];
        const uint64_t start = foff[h], len = foff[h + 1] - start;
        if (row >= n_rows) {
            if (lane == 0) atomicOr(flag, 1u);
            continue;
        }
        const uint64_t q_lo = qoffsets[q];
        const uint64_t* Q = qhashes + q_lo;
        const uint32_t n = qn[q], cand = (uint32_t)(h - qlo[q]);
        const uint64_t base_key = q_lo - q_first;
        const uint64_t lo = offsets[row], hi = offsets[row + 1];
        uint64_t written = 0;
        bool bad = false;
        for (uint64_t at0 = lo; at0 < hi && !bad; at0 += 64u * GM_FILL_UNROLL) {
            // GM_FILL_UNROLL groups of 64 consecutive hashes; the lane's lookups go side by side (gm_find_group)
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
                const uint64_t mask = mask_of(match);
                const uint64_t at = written + (uint64_t)__popcll(mask & below);
                if (match && at < len) {
                    fpos[start + at] = pos[k];
                    keys[start + at] = gm_inv_key(base_key, pos[k]);
                    vals[start + at] = cand;
                }
                written += (uint64_t)__popcll(mask);
            }
            if (written > len) bad = true;
            if (mask_of(past)) break;                                  // ascending: the row ends here at the common scaled
        }
        if ((bad || written != len) && lane == 0) atomicOr(flag, 1u);
    }
}

// The rounds.  A workgroup takes one query at a time by ticket from `ticket`, this launch's own zeroed counter.  Dynamic LDS:
// cnt_cap counters, then the bitmap.  It waits on its own barriers only, and the ticket is its one device-scope atomic.  A query has
// at most as many rounds as candidates, so the picks of query q go to the slots [qlo[q], + rounds) of its own hits.
__global__ __launch_bounds__(GM_BLOCK) void gm_rounds_kernel(const uint64_t* __restrict__ qoffsets, uint64_t m, const uint32_t* __restrict__ hit_rows,
                                                             const uint32_t* __restrict__ hit_common, const uint32_t* __restrict__ qlo,
                                                             const uint32_t* __restrict__ qn, const uint32_t* __restrict__ status,
                                                             const uint64_t* __restrict__ foff, const uint32_t* __restrict__ fpos,
                                                             const uint64_t* __restrict__ inv_keys, const uint64_t* __restrict__ inv_cands,
                                                             uint64_t threshold_hashes, uint32_t cnt_cap, uint32_t word_cap,
                                                             uint32_t* __restrict__ out_rows, uint32_t* __restrict__ out_isect,
                                                             uint32_t* __restrict__ out_rounds, unsigned long long* __restrict__ ticket,
                                                             const uint32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
    __shared__ unsigned long long s_red[GM_BLOCK / 64];
    __shared__ unsigned long long s_query;
    uint32_t* s_cnt = s_dyn;
    uint32_t* s_bits = s_dyn + cnt_cap;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (*flag) return;                                                 // the forward CSR is not what the hits promised: nothing runs
    const uint64_t q_first = qoffsets[0];
    for (;;) {
        if (tid == 0) s_query = atomicAdd(ticket, 1ull);
        __syncthreads();
        const uint64_t q = s_query;
        if (q >= m) break;
        const uint32_t h0 = qlo[q], nc = qlo[q + 1] - h0, n = qn[q], words = gm_bitmap_words(n);
        // (what the prep kernel accepted fits; the test keeps a launch with other caps from leaving its LDS)
        const bool runs = !status[q] && nc != 0 && nc <= cnt_cap && words <= word_cap;
        if (runs) {
            for (uint32_t i = tid; i < nc; i += GM_BLOCK) s_cnt[i] = hit_common[h0 + i];
            for (uint32_t w = tid; w < words; w += GM_BLOCK) s_bits[w] = gm_bitmap_init_word(w, n);
            __syncthreads();
            const uint32_t seg_lo = (uint32_t)foff[h0], seg_hi = (uint32_t)foff[h0 + nc];
            const uint64_t base_key = qoffsets[q] - q_first;
            uint32_t rounds = 0;
            while (rounds < nc) {
                unsigned long long key = 0;
                for (uint32_t i = tid; i < nc; i += GM_BLOCK) {
                    const unsigned long long k = gm_pick_key(s_cnt[i], i);
                    key = k > key ? k : key;
                }
                key = wave_max(key);
                if (lane == 0) s_red[wave] = key;
                __syncthreads();
                unsigned long long best = s_red[0];
                for (uint32_t w = 1; w < GM_BLOCK / 64; ++w) best = s_red[w] > best ? s_red[w] : best;
                if (gm_stop(best, threshold_hashes)) break;            // (the same words for every lane: the whole workgroup leaves)
                const uint32_t win = gm_key_candidate(best);
                if (win >= nc) break;
                if (tid == 0) {
                    out_rows[h0 + rounds] = hit_rows[h0 + win];
                    out_isect[h0 + rounds] = gm_key_count(best);
                }
                ++rounds;
                const uint32_t a = (uint32_t)foff[h0 + win], b = (uint32_t)foff[h0 + win + 1];
                for (uint32_t i = a + tid; i < b; i += GM_BLOCK) {
                    const uint32_t pos = fpos[i];
                    if (pos >= n) continue;
                    const uint32_t bit = gm_bit(pos);
                    const uint32_t old = atomicAnd(&s_bits[pos >> 5], ~bit);
                    if (!(old & bit)) continue;                        // covered in an earlier round
                    const uint64_t k = gm_inv_key(base_key, pos);
                    for (uint32_t j = gm_inv_start(inv_keys, seg_lo, seg_hi, k); j < seg_hi && inv_keys[j] == k; ++j) {
                        const uint64_t c = inv_cands[j];
                        if (c < nc) atomicSub(&s_cnt[c], 1u);
                    }
                }
                __syncthreads();                                       // the round ends: counters and bitmap stand, s_red is free
            }
            if (tid == 0) out_rounds[q] = rounds;
        }
        __syncthreads();                                               // s_query and the LDS state are free for the next query
    }
}

// *total = rounds of the queries that ran
__global__ __launch_bounds__(256) void gm_total_kernel(const uint32_t* __restrict__ out_rounds, const uint32_t* __restrict__ status, uint64_t m,
                                                       unsigned long long* __restrict__ total) {
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    unsigned long long local = 0;
    for (uint64_t q = threadIdx.x; q < m; q += 256u)
        if (!status[q]) local += out_rounds[q];
    if (local) atomicAdd(&s_sum, local);
    __syncthreads();
    if (threadIdx.x == 0) *total = s_sum;
}

unsigned blocks_for(uint64_t n, unsigned cap = 2048) {
    const uint64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

size_t scan_bytes(uint64_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(),
                                  (hipStream_t)0);
    return bytes;
}

// the workspace, carved in 256-byte granules: what depends on the entries of the forward CSR comes last
struct GmLayout {
    size_t qlo, qn, w, foff, scal, scan, scan_bytes_, fixed_end, fpos, keys_a, vals_a, keys_b, vals_b, sort, sort_bytes, end;
    GmLayout(uint64_t m, uint64_t n_hits, uint64_t total) {
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t p = at; at += al256(bytes); return p; };
        qlo = take((m + 2) * 4); qn = take((m + 1) * 4); w = take((n_hits + 2) * 8); foff = take((n_hits + 2) * 8); scal = take(256);
        scan_bytes_ = scan_bytes(n_hits + 1);
        scan = take(scan_bytes_);
        fixed_end = at;
        fpos = take((total + 1) * 4);
        keys_a = take((total + 1) * 8); vals_a = take((total + 1) * 8); keys_b = take((total + 1) * 8); vals_b = take((total + 1) * 8);
        sort_bytes = sort_pairs_temp_bytes(total ? total : 1);
        sort = take(sort_bytes);
        end = at + 256;
    }
};

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

size_t gather_many_workspace_bytes(uint64_t m, uint64_t n_hits, uint64_t total_common) { return GmLayout(m, n_hits, total_common).end; }

hipError_t gather_many_plan(const uint64_t* d_qhashes, const uint64_t* d_qoffsets, uint64_t m, const uint32_t* d_hit_queries,
                            const uint32_t* d_hit_common, uint64_t n_hits, uint64_t cutoff, uint32_t max_query_hashes, uint32_t max_candidates,
                            uint32_t* d_qlo, uint32_t* d_qn, uint32_t* d_status, uint64_t* d_sums, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(gm_prep_kernel, dim3((unsigned)(m < 4096 ? m : 4096)), dim3(256), 0, stream, d_qhashes, d_qoffsets, m, 0u, d_hit_queries, d_hit_common,
                       n_hits, cutoff, max_query_hashes, max_candidates, d_qlo, d_qn, d_status, (uint32_t*)nullptr, (unsigned long long*)d_sums,
                       (uint32_t*)nullptr);
    return hipGetLastError();
}

hipError_t gather_many_run(const GatherManyArgs& a, uint64_t* total_rounds, uint32_t* trouble, float* ms3, hipStream_t st) {
    if (!total_rounds || !trouble) return hipErrorInvalidValue;
    *total_rounds = 0;
    *trouble = GM_OK;
    if (ms3) ms3[0] = ms3[1] = ms3[2] = 0.f;
    const uint32_t mqh = a.max_query_hashes ? a.max_query_hashes : GM_MAX_QUERY_HASHES;
    const uint32_t mc = a.max_candidates ? a.max_candidates : GM_MAX_CANDIDATES;
    if (!gm_caps_fit(mqh, mc) || a.m >= GM_INDEX_LIMIT || a.n_rows >= GM_INDEX_LIMIT || a.n_hits >= GM_INDEX_LIMIT || a.grid > (1u << 20) ||
        (uint64_t)a.q_base + a.m >= GM_INDEX_LIMIT)
        return hipErrorInvalidValue;
    const GmLayout L0(a.m, a.n_hits, 0);
    if (a.workspace_bytes < L0.end || !a.d_workspace) return hipErrorInvalidValue;
    if (a.m == 0) return hipSuccess;
    char* ws = static_cast<char*>(a.d_workspace);
    uint32_t *qlo = (uint32_t*)(ws + L0.qlo), *qn = (uint32_t*)(ws + L0.qn);
    uint64_t *w = (uint64_t*)(ws + L0.w), *foff = (uint64_t*)(ws + L0.foff), *scal = (uint64_t*)(ws + L0.scal);
    unsigned long long *fill_ticket = (unsigned long long*)scal, *rounds_ticket = fill_ticket + 1, *d_total = fill_ticket + 4;
    uint32_t *flag = (uint32_t*)(scal + 2), *maxes = (uint32_t*)(scal + 3);
    const bool timed = ms3 != nullptr;
    Stamp t0, t1, t2, t3;
    hipError_t e;

    // ---- which queries run, where their hits stand, and the slices of the forward CSR
    if ((e = t0.mark(timed, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(scal, 0, 256, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(gm_prep_kernel, dim3((unsigned)(a.m < 4096 ? a.m : 4096)), dim3(256), 0, st, a.d_qhashes, a.d_qoffsets, a.m, a.q_base,
                       a.d_hit_queries, a.d_hit_common, a.n_hits, a.cutoff, mqh, mc, qlo, qn, a.d_status, a.d_out_rounds, (unsigned long long*)nullptr,
                       maxes);
    hipLaunchKernelGGL(gm_weights_kernel, dim3(blocks_for(a.n_hits + 1)), dim3(256), 0, st, a.d_hit_queries, a.d_hit_common, a.n_hits, a.q_base, a.m,
                       a.d_status, w);
    size_t pb = L0.scan_bytes_;
    if ((e = rocprim::exclusive_scan(ws + L0.scan, pb, (const uint64_t*)w, foff, (uint64_t)0, (size_t)(a.n_hits + 1), rocprim::plus<uint64_t>(), st)) !=
        hipSuccess)
        return e;
    uint64_t total = 0, span[2] = {0, 0};
    uint32_t mx[2] = {0, 0};
    if ((e = hipMemcpyAsync(&total, foff + a.n_hits, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(mx, maxes, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&span[0], a.d_qoffsets, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&span[1], a.d_qoffsets + a.m, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (total >= GM_INDEX_LIMIT) { *trouble = GM_TOO_MANY_ENTRIES; return hipSuccess; }
    const GmLayout L(a.m, a.n_hits, total);
    if (a.workspace_bytes < L.end) { *trouble = GM_WORKSPACE_TOO_SMALL; return hipSuccess; }
    if (total == 0 || a.n_hits == 0) {                                 // no query that runs has a candidate: every rounds[q] is 0 already
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        return hipSuccess;
    }
    uint32_t* fpos = (uint32_t*)(ws + L.fpos);
    uint64_t *keys_a = (uint64_t*)(ws + L.keys_a), *vals_a = (uint64_t*)(ws + L.vals_a), *keys_b = (uint64_t*)(ws + L.keys_b),
             *vals_b = (uint64_t*)(ws + L.vals_b);
    const unsigned fill_grid = a.grid ? a.grid : blocks_for(a.n_hits * 64u);   // a wave a hit, four waves a workgroup
    hipLaunchKernelGGL(gm_fill_kernel, dim3(fill_grid), dim3(GM_BLOCK), 0, st, a.d_qhashes, a.d_qoffsets, a.m, a.q_base, a.d_hashes, a.d_offsets, a.n_rows,
                       a.d_hit_queries, a.d_hit_rows, a.n_hits, a.cutoff, qlo, qn, a.d_status, foff, fpos, keys_a, vals_a, fill_ticket, flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = t1.mark(timed, st)) != hipSuccess) return e;

    // ---- the inverted lists: one stable sort by the position among all query hashes leaves a position's candidates ascending
    const uint64_t q_span = span[1] >= span[0] ? span[1] - span[0] : 0;
    if ((e = sort_pairs(keys_a, keys_b, vals_a, vals_b, total, gm_key_bits(q_span ? q_span : 1), ws + L.sort, L.sort_bytes, st)) != hipSuccess) return e;
    if ((e = t2.mark(timed, st)) != hipSuccess) return e;

    // ---- the rounds
    const uint32_t cnt_cap = mx[1] ? mx[1] : 1, word_cap = gm_bitmap_words(mx[0] ? mx[0] : 1);
    const size_t lds = 4u * (size_t)cnt_cap + 4u * (size_t)word_cap;
    if (lds + GM_LDS_STATIC > GM_LDS_LIMIT) return hipErrorInvalidValue;   // (gm_caps_fit said otherwise)
    size_t per_cu = (160u * 1024u) / (lds + GM_LDS_STATIC);
    per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;                 // eight workgroups of four waves fill a CU's 32 wave slots
    const uint64_t full = 256u * per_cu;
    const unsigned g = a.grid ? a.grid : (unsigned)(a.m < full ? a.m : full);
    hipLaunchKernelGGL(gm_rounds_kernel, dim3(g), dim3(GM_BLOCK), lds, st, a.d_qoffsets, a.m, a.d_hit_rows, a.d_hit_common, qlo, qn, a.d_status, foff, fpos,
                       keys_b, vals_b, a.threshold_hashes, cnt_cap, word_cap, a.d_out_rows, a.d_out_isect, a.d_out_rounds, rounds_ticket, flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = t3.mark(timed, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(gm_total_kernel, dim3(1), dim3(256), 0, st, a.d_out_rounds, a.d_status, a.m, d_total);
    uint64_t head[3] = {0, 0, 0};                                      // flag, (maxes), total rounds
    if ((e = hipMemcpyAsync(&head[0], scal + 2, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&head[2], d_total, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if ((uint32_t)head[0]) { *trouble = GM_FILL_MISMATCH; return hipSuccess; }
    *total_rounds = head[2];
    if (timed) {
        (void)hipEventElapsedTime(&ms3[0], t0.ev, t1.ev);
        (void)hipEventElapsedTime(&ms3[1], t1.ev, t2.ev);
        (void)hipEventElapsedTime(&ms3[2], t2.ev, t3.ev);
    }
    return hipSuccess;
}

}  // namespace smg
