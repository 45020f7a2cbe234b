// overlap_many.hip -- m queries against every row of a CSR collection in ONE pass over the collection.
//
// GPU counterpart of the reference's many-against-many loop: `for query in queries: index.search(query)` /
// `index.prefetch(query)` (src/sourmash/index/__init__.py:115-170, 202-256), which walks the collection once per query.  Here the
// queries are merged into one index --
//   U     the sorted distinct hashes of all queries (at the common scaled),
//   uoff  where the postings of U[j] start, |U| + 1 entries,
//   post  the numbers of the queries that hold U[j], ascending,
// -- built with one stable (hash, query) pair sort, and looked up through a QIndex with records (qindex.hpp).  The pass then reads
// every row of the collection once: a workgroup takes a row, its lanes look the row's hashes up in U and count, in LDS, one
// counter per query; the queries whose counter reaches their `need` leave as (query, row, count) triples.  Only those leave: the
// m x n matrix is never formed.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include "device_api.hpp"
#include "many_core.hpp"
#include "qindex.hpp"

namespace smg {

namespace {

// keys[j] / vals[j]: the hashes of the query rows back to back and the number of the row each came from
__global__ __launch_bounds__(256) void many_expand_kernel(const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ offsets, uint64_t m,
                                                          uint64_t total, uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
    const uint64_t base = offsets[0];
    for (uint64_t q = blockIdx.x; q < m; q += gridDim.x) {
        const uint64_t lo = offsets[q], hi = offsets[q + 1];
        for (uint64_t i = lo + threadIdx.x; i < hi; i += 256u) {
            const uint64_t j = i - base;
            if (j < total) { keys[j] = hashes[i]; vals[j] = q; }
        }
    }
}

// post[i] = the query number as u32
__global__ __launch_bounds__(256) void many_narrow_kernel(const uint64_t* __restrict__ vals, uint64_t n, uint32_t* __restrict__ post) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) post[i] = (uint32_t)vals[i];
}

// out[0] = distinct hashes <= cutoff (the part of U the pass uses), out[1] = the largest of them
__global__ void many_cut_kernel(const uint64_t* __restrict__ U, const uint64_t* __restrict__ n_u, uint64_t cutoff, uint64_t* __restrict__ out) {
    const uint64_t n = many_cut_len(U, *n_u, cutoff);
    out[0] = n;
    out[1] = n ? U[n - 1] : 0;
}

__global__ __launch_bounds__(256) void many_table_kernel(const uint64_t* __restrict__ U, uint64_t n, uint32_t shift, uint32_t buckets, uint32_t* __restrict__ T) {
    qindex_fill_bucket(U, n, shift, buckets, T, blockIdx.x * 256u + threadIdx.x);
}
__global__ __launch_bounds__(256) void many_record_kernel(const uint64_t* __restrict__ U, const uint32_t* __restrict__ T, uint32_t buckets, QRec* __restrict__ rec) {
    qindex_fill_record(U, T, buckets, rec, blockIdx.x * 256u + threadIdx.x);
}

// sizes[r] = hashes of row r that are <= cutoff
__global__ __launch_bounds__(256) void many_sizes_kernel(const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                         uint64_t cutoff, uint64_t* __restrict__ sizes) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256u) {
        const uint64_t lo = offsets[r];
        sizes[r] = many_cut_len(hashes + lo, offsets[r + 1] - lo, cutoff);
    }
}

// The pass, for the queries [q_lo, q_lo + qb) of the merged index.  Rows are handed out by tickets: a workgroup's first row is its
// own number, every later one gridDim.x + a ticket from `ticket` (this launch's own zeroed counter), taken while the row in front
// of it is counted.  s_cnt: qb counters, zero between rows.  A workgroup waits on its own barriers only.
__global__ __launch_bounds__(MANY_BLOCK) void many_overlap_kernel(QIndex qi, const uint32_t* __restrict__ uoff, const uint32_t* __restrict__ post,
                                                                  const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ offsets,
                                                                  uint64_t n_rows, uint64_t cutoff, const uint32_t* __restrict__ need, uint32_t q_lo,
                                                                  uint32_t qb, uint32_t* __restrict__ out_q, uint32_t* __restrict__ out_row,
                                                                  uint32_t* __restrict__ out_cnt, uint64_t capacity,
                                                                  unsigned long long* __restrict__ cursor, unsigned long long* __restrict__ ticket) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_cnt[];
    __shared__ unsigned long long s_next[2];                 // the row behind this one, by the parity of the workgroup's step
    const uint32_t tid = threadIdx.x, lane = tid & 63u, q_hi = q_lo + qb;
    for (uint32_t i = tid; i < qb; i += MANY_BLOCK) s_cnt[i] = 0;
    __syncthreads();
    uint64_t row = blockIdx.x;
    for (uint32_t step = 0; row < n_rows; ++step) {
        if (tid == 0) s_next[step & 1u] = (unsigned long long)gridDim.x + atomicAdd(ticket, 1ull);
        const uint64_t lo = offsets[row], hi = offsets[row + 1];
        for (uint64_t i = lo + tid; i < hi; i += MANY_BLOCK) {
            const uint64_t h = hashes[i];
            if (h > cutoff) break;                           // ascending: the row ends here at the common scaled
            const uint32_t j = q_find(qi, h);
            if (j == NONE32) continue;
            uint32_t a = uoff[j], b = uoff[j + 1];
            many_post_range(post, &a, &b, q_lo, q_hi);
            for (uint32_t p = a; p < b; ++p) atomicAdd(&s_cnt[post[p] - q_lo], 1u);
        }
        __syncthreads();
        // the counters, 64 at a time per wave: those that reach their query's need are compacted by a ballot and take their
        // places with one atomic on the cursor; every counter is zero again afterwards
        for (uint32_t base = 0; base < qb; base += MANY_BLOCK) {
            const uint32_t idx = base + tid;
            uint32_t c = 0;
            if (idx < qb) {
                c = s_cnt[idx];
                if (c) s_cnt[idx] = 0;
            }
            const bool hit = c != 0 && c >= need[q_lo + idx];
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                unsigned long long first = 0;
                if (lane == (uint32_t)__ffsll((long long)mask) - 1u) first = atomicAdd(cursor, (unsigned long long)__popcll(mask));
                first = __shfl(first, __ffsll((long long)mask) - 1);
                const unsigned long long at = first + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
                if (hit && at < capacity) {
                    out_q[at] = q_lo + idx;
                    out_row[at] = (uint32_t)row;
                    out_cnt[at] = c;
                }
            }
        }
        __syncthreads();
        row = s_next[step & 1u];
    }
}

__global__ __launch_bounds__(256) void many_keys_kernel(const uint32_t* __restrict__ q, const uint32_t* __restrict__ row, const uint32_t* __restrict__ cnt,
                                                        uint64_t n, uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        keys[i] = many_key(q[i], row[i]);
        vals[i] = cnt[i];
    }
}
__global__ __launch_bounds__(256) void many_unkeys_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, uint64_t n,
                                                          uint32_t* __restrict__ q, uint32_t* __restrict__ row, uint32_t* __restrict__ cnt) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        q[i] = many_key_query(keys[i]);
        row[i] = many_key_row(keys[i]);
        cnt[i] = (uint32_t)vals[i];
    }
}

unsigned blocks_for(uint64_t n, unsigned cap = 2048) {
    const uint64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

size_t rle_bytes(uint64_t n) {
    size_t bytes = 0;
    (void)rocprim::run_length_encode(nullptr, bytes, (const uint64_t*)nullptr, (unsigned int)(n ? n : 1), (uint64_t*)nullptr, (uint32_t*)nullptr,
                                     (uint64_t*)nullptr, (hipStream_t)0);
    return bytes;
}
size_t scan_bytes(uint64_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)(n + 1), rocprim::plus<uint32_t>(), (hipStream_t)0);
    return bytes;
}

// the workspace, carved in 256-byte granules
struct ManyLayout {
    size_t keys_a, vals_a, keys_b, vals_b, U, counts, uoff, post, T, rec, need, scal, prim, prim_bytes, end;
    ManyLayout(uint64_t m, uint64_t q_total, uint64_t capacity) {
        const uint64_t pairs = q_total > capacity ? q_total : capacity;      // the pair arrays serve the build, then the final sort
        const uint64_t max_buckets = 2 * q_total + 2;
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t p = at; at += al256(bytes); return p; };
        keys_a = take((pairs + 1) * 8); vals_a = take((pairs + 1) * 8); keys_b = take((pairs + 1) * 8); vals_b = take((pairs + 1) * 8);
        U = take((q_total + 8) * 8); counts = take((q_total + 2) * 4); uoff = take((q_total + 2) * 4); post = take((q_total + 1) * 4);
        T = take((max_buckets + 2) * 4); rec = take((max_buckets + 1) * sizeof(QRec)); need = take((m + 1) * 4); scal = take(256);
        prim_bytes = sort_pairs_temp_bytes(pairs);
        if (rle_bytes(q_total) > prim_bytes) prim_bytes = rle_bytes(q_total);
        if (scan_bytes(q_total) > prim_bytes) prim_bytes = scan_bytes(q_total);
        prim = take(prim_bytes);
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

size_t many_overlap_workspace_bytes(uint64_t m, uint64_t q_total, uint64_t capacity) { return ManyLayout(m, q_total, capacity).end; }

uint32_t many_overlap_passes(uint64_t m, uint32_t q_block) {
    const uint32_t qb = q_block ? q_block : MANY_Q_BLOCK;
    return (uint32_t)((m + qb - 1) / qb);
}

hipError_t many_sizes_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n, uint64_t cutoff, uint64_t* d_sizes, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(many_sizes_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, d_hashes, d_offsets, n, cutoff, d_sizes);
    return hipGetLastError();
}

hipError_t many_overlap_run(const ManyArgs& a, uint64_t* hits_out, float* ms3, hipStream_t st) {
    if (!hits_out) return hipErrorInvalidValue;
    *hits_out = 0;
    if (ms3) ms3[0] = ms3[1] = ms3[2] = 0.f;
    const uint32_t q_block = a.q_block ? a.q_block : MANY_Q_BLOCK;
    if (q_block > MANY_Q_BLOCK_MAX || a.m >= NONE32 || a.n_rows >= NONE32 || a.q_total >= 0x7fffffffull || a.capacity >= 0xffffffffull ||
        a.grid > (1u << 20))
        return hipErrorInvalidValue;
    const ManyLayout L(a.m, a.q_total, a.capacity);
    if (a.workspace_bytes < L.end || !a.d_result) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.d_result, 0, 32, st);
    if (e != hipSuccess) return e;
    if (a.m == 0 || a.n_rows == 0 || a.q_total == 0) return hipStreamSynchronize(st);
    char* ws = static_cast<char*>(a.d_workspace);
    uint64_t *keys_a = (uint64_t*)(ws + L.keys_a), *vals_a = (uint64_t*)(ws + L.vals_a), *keys_b = (uint64_t*)(ws + L.keys_b),
             *vals_b = (uint64_t*)(ws + L.vals_b), *U = (uint64_t*)(ws + L.U), *scal = (uint64_t*)(ws + L.scal);
    uint32_t *counts = (uint32_t*)(ws + L.counts), *uoff = (uint32_t*)(ws + L.uoff), *post = (uint32_t*)(ws + L.post), *T = (uint32_t*)(ws + L.T);
    QRec* rec = (QRec*)(ws + L.rec);
    void* prim = ws + L.prim;
    const uint64_t nq = a.q_total;
    Stamp t0, t1, t2, t3;
    const bool timed = ms3 != nullptr;

    // ---- the merged index: one stable pair sort by hash leaves the queries of a hash ascending
    if ((e = t0.mark(timed, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(many_expand_kernel, dim3((unsigned)(a.m < 4096 ? a.m : 4096)), dim3(256), 0, st, a.d_qhashes, a.d_qoffsets, a.m, nq, keys_a, vals_a);
    if ((e = sort_pairs(keys_a, keys_b, vals_a, vals_b, nq, 64, prim, L.prim_bytes, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(counts, 0, (nq + 2) * 4, st)) != hipSuccess) return e;
    size_t pb = L.prim_bytes;
    if ((e = rocprim::run_length_encode(prim, pb, (const uint64_t*)keys_b, (unsigned int)nq, U, counts, scal, st)) != hipSuccess) return e;
    pb = L.prim_bytes;
    // (over all nq + 1 entries: the counts behind the last distinct hash are zero, so uoff[|U|] = nq closes the offsets)
    if ((e = rocprim::exclusive_scan(prim, pb, (const uint32_t*)counts, uoff, 0u, (size_t)(nq + 1), rocprim::plus<uint32_t>(), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(many_narrow_kernel, dim3(blocks_for(nq)), dim3(256), 0, st, vals_b, nq, post);
    hipLaunchKernelGGL(many_cut_kernel, dim3(1), dim3(1), 0, st, U, scal, a.cutoff, scal + 1);
    uint64_t head[3] = {0, 0, 0};
    if ((e = hipMemcpyAsync(head, scal, 24, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    const uint64_t n_u = head[1], u_max = head[2];
    if ((e = hipMemcpyAsync(a.d_result + 1, &head[1], 8, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if (n_u == 0) return hipStreamSynchronize(st);           // no query hash at the common scaled: nothing can hit
    uint32_t shift = 0, buckets = 0;
    qindex_geometry(n_u, u_max, &shift, &buckets);
    if (shift > 63) { shift = 63; buckets = (uint32_t)(u_max >> 63) + 1; }   // (a single hash with the top bit set asks for a shift by 64)
    if ((uint64_t)buckets > 2 * nq + 2) return hipErrorInvalidValue;   // (qindex_geometry: never more than 2 n + 1)
    hipLaunchKernelGGL(many_table_kernel, dim3((buckets + 1 + 255) / 256), dim3(256), 0, st, U, n_u, shift, buckets, T);
    hipLaunchKernelGGL(many_record_kernel, dim3((buckets + 255) / 256), dim3(256), 0, st, U, T, buckets, rec);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    QIndex qi;
    qi.Q = U; qi.nq = n_u; qi.T = T; qi.shift = shift; qi.qmax = u_max; qi.rec = rec;
    if ((e = t1.mark(timed, st)) != hipSuccess) return e;

    // ---- the pass: once over the collection per block of queries
    const uint32_t passes = many_overlap_passes(a.m, q_block);
    unsigned long long* tickets = (unsigned long long*)(scal + 4);   // one counter, zeroed again in front of every pass
    unsigned long long* cursor = (unsigned long long*)a.d_result;
    const unsigned full = 256u * 8u;                          // eight workgroups of four waves fill a CU's 32 wave slots
    const unsigned g = a.grid ? a.grid : (unsigned)(a.n_rows < full ? a.n_rows : full);
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t q_lo = p * q_block, qb = (uint32_t)(a.m - q_lo < q_block ? a.m - q_lo : q_block);
        if ((e = hipMemsetAsync(tickets, 0, 8, st)) != hipSuccess) return e;   // in stream order: the pass in front has finished with it
        hipLaunchKernelGGL(many_overlap_kernel, dim3(g), dim3(MANY_BLOCK), (size_t)qb * 4, st, qi, uoff, post, a.d_hashes, a.d_offsets, a.n_rows,
                           a.cutoff, a.d_need, q_lo, qb, a.d_queries, a.d_rows, a.d_common, a.capacity, cursor, tickets);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = t2.mark(timed, st)) != hipSuccess) return e;
    uint64_t hits = 0;
    const uint64_t n_passes = passes;
    if ((e = hipMemcpyAsync(a.d_result + 2, &n_passes, 8, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&hits, a.d_result, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    *hits_out = hits;

    // ---- order by (query, row); a result that did not fit stays as it fell (the caller runs again with room for `hits`)
    if (hits && hits <= a.capacity) {
        hipLaunchKernelGGL(many_keys_kernel, dim3(blocks_for(hits)), dim3(256), 0, st, a.d_queries, a.d_rows, a.d_common, hits, keys_a, vals_a);
        if ((e = sort_pairs(keys_a, keys_b, vals_a, vals_b, hits, 64, prim, L.prim_bytes, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(many_unkeys_kernel, dim3(blocks_for(hits)), dim3(256), 0, st, keys_b, vals_b, hits, a.d_queries, a.d_rows, a.d_common);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = t3.mark(timed, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (timed) {
        (void)hipEventElapsedTime(&ms3[0], t0.ev, t1.ev);
        (void)hipEventElapsedTime(&ms3[1], t1.ev, t2.ev);
        (void)hipEventElapsedTime(&ms3[2], t2.ev, t3.ev);
    }
    return hipSuccess;
}

}  // namespace smg
