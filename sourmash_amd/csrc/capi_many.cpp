// capi_many.cpp -- the C-ABI (include/sourmash_amd.h): many queries against a collection in one pass over it (overlap_many.hip,
// many_core.hpp).  The raw entries work on the caller's device buffers; smgpu_sketchset_overlaps_many takes two resident sets,
// picks the capacity, runs again once when the hits did not fit, and leaves the result on the host.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include "capi_common.hpp"
#include "many_core.hpp"

using namespace smg;

namespace {

// what a call leaves on the host
struct ManyHits {
    std::vector<uint32_t> queries, rows, common;
    std::vector<uint64_t> query_sizes, row_sizes;             // at the common scaled
    uint64_t max_hash = 0, reruns = 0, passes = 0;
    double ms[4] = {0, 0, 0, 0};                              // index build, passes, sort (device), whole call (host)
};

std::atomic<uint64_t> g_first_capacity{0};                    // test support: smgpu_many_set_first_capacity

void check_raw(const void* p, const char* what) {
    if (!p) throw err_internal(std::string("smgpu_many_overlap_raw: null pointer (") + what + ")");
}

// (a set keeps its ksize in residues; the reference compares the sketches' own, three times that for the amino acid alphabets)
ManyParams params_of(const SketchSet& s) {
    if (s.ksize == 0) throw err_internal("the set's sketches do not share one set of parameters");
    return ManyParams{s.ksize * (s.hash_function == HF_DNA ? 1u : 3u), s.hash_function, s.seed, s.max_hash, s.num};
}

// the reference's order (check_compatible, minhash.rs:886-912): ksize, hash function, max_hash only when a side is num, seed
void check_params_compatible(const ManyParams& a, const ManyParams& b) {
    switch (many_compat_code(a, b)) {
    case 0: return;
    case E_MISMATCH_KSIZES: throw err_mismatch_ksizes();
    case E_MISMATCH_DNA_PROT: throw err_mismatch_dnaprot();
    case E_MISMATCH_SCALED: throw err_mismatch_scaled();
    case E_MISMATCH_SEED: throw err_mismatch_seed();
    default: throw Error(E_MISMATCH_NUM, "a search of many queries requires scaled signatures");
    }
}

}  // namespace

void smg::check_sets_compatible(const SketchSet& db, const SketchSet& q) {
    const ManyParams a = params_of(db), b = params_of(q);
    check_params_compatible(a, b);
}

void smg::check_sketch_compatible(const SketchSet& db, const KmerMinHash& mh) {
    check_params_compatible(params_of(db), ManyParams{mh.ksize, mh.hash_function, mh.seed, mh.max_hash, mh.num});
}

// Room for the hits: a few per query and row is what a thresholded search leaves; every pair at most.  A result that does not fit
// reports its size, and the second run has exactly that room.
void smg::many_hits_on_device(const SketchSet& db, const SketchSet& qs, const uint32_t* d_need, uint64_t cutoff, ManyDeviceHits& out, hipStream_t st) {
    const uint64_t m = qs.n, n = db.n;
    const uint64_t all_pairs = m * n;
    uint64_t cap = g_first_capacity.load();
    if (cap == 0) cap = std::max<uint64_t>(1u << 20, 8 * (m + n));
    cap = std::min<uint64_t>(cap, all_pairs);
    AsyncBuf d_result(64, st), ws;
    for (int attempt = 0;; ++attempt) {
        if (cap >= 0xffffffffull) throw err_internal("smgpu_sketchset_overlaps_many: 2^32 hits or more; raise the counts the hits need");
        out.queries.reset(cap * 4 + 16, st); out.rows.reset(cap * 4 + 16, st); out.common.reset(cap * 4 + 16, st);
        const uint64_t ws_bytes = many_overlap_workspace_bytes(m, qs.total, cap);
        ws.reset((size_t)ws_bytes, st);
        const ManyArgs a{qs.hashes.as<uint64_t>(), qs.offsets.as<uint64_t>(), m, qs.total, db.hashes.as<uint64_t>(), db.offsets.as<uint64_t>(), n,
                         d_need, cutoff, 0, 0, out.queries.as<uint32_t>(), out.rows.as<uint32_t>(), out.common.as<uint32_t>(), cap,
                         d_result.as<uint64_t>(), ws.p, ws_bytes};
        hip_check(many_overlap_run(a, &out.hits, out.ms3, st), "many_overlap");
        if (out.hits <= cap) break;
        if (attempt) throw err_internal("smgpu_sketchset_overlaps_many: the second run found more hits than the first");
        cap = out.hits;
        out.reruns = 1;
    }
}

extern "C" {

void smgpu_many_geometry(uint32_t* workgroup, uint32_t* q_block, uint32_t* q_block_max) {
    if (workgroup) *workgroup = MANY_BLOCK;
    if (q_block) *q_block = MANY_Q_BLOCK;
    if (q_block_max) *q_block_max = MANY_Q_BLOCK_MAX;
}

void smgpu_many_need(uint32_t mode, double threshold, const uint64_t* sizes, uint64_t m, uint32_t* need_out) {
    landing_void([&] {
        if (mode > MANY_MAX_CONTAINMENT) throw err_internal("smgpu_many_need: mode 0 (Jaccard), 1 (containment) or 2 (max containment)");
        if (m && (!sizes || !need_out)) throw err_internal("smgpu_many_need: null pointer");
        for (uint64_t q = 0; q < m; ++q) need_out[q] = many_need(mode, threshold, sizes[q]);
    });
}

uint64_t smgpu_many_overlap_workspace_bytes(uint64_t m, uint64_t q_total, uint64_t capacity) {
    return many_overlap_workspace_bytes(m, q_total, capacity);
}

uint64_t smgpu_many_overlap_raw(const uint64_t* d_qhashes, const uint64_t* d_qoffsets, uint64_t m, uint64_t q_total, const uint64_t* d_hashes,
                                const uint64_t* d_offsets, uint64_t n_rows, const uint32_t* d_need, uint64_t cutoff, uint32_t q_block, uint32_t grid,
                                uint32_t* d_queries, uint32_t* d_rows, uint32_t* d_common, uint64_t capacity, uint64_t* d_result, void* d_workspace,
                                uint64_t workspace_bytes, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        check_raw(d_result, "d_result");
        check_raw(d_workspace, "d_workspace");
        if (m && n_rows) { check_raw(d_qoffsets, "d_qoffsets"); check_raw(d_offsets, "d_offsets"); check_raw(d_need, "d_need"); }
        if (m && n_rows && q_total) { check_raw(d_qhashes, "d_qhashes"); check_raw(d_hashes, "d_hashes"); }
        if (capacity) { check_raw(d_queries, "d_queries"); check_raw(d_rows, "d_rows"); check_raw(d_common, "d_common"); }
        if (q_block > MANY_Q_BLOCK_MAX) throw err_internal("smgpu_many_overlap_raw: q_block above " + std::to_string(MANY_Q_BLOCK_MAX));
        if (grid > (1u << 20)) throw err_internal("smgpu_many_overlap_raw: grid above 1048576 workgroups");
        if (m >= 0xffffffffull || n_rows >= 0xffffffffull || q_total >= 0x7fffffffull || capacity >= 0xffffffffull)
            throw err_internal("smgpu_many_overlap_raw: 2^32 queries, rows or hits, or 2^31 query hashes, are not taken");
        if (workspace_bytes < many_overlap_workspace_bytes(m, q_total, capacity))
            throw err_internal("smgpu_many_overlap_raw: the workspace is smaller than smgpu_many_overlap_workspace_bytes says");
        (void)DeviceCtx::get();                                      // no device: say so, not "invalid device"
        const ManyArgs a{d_qhashes, d_qoffsets, m, q_total, d_hashes, d_offsets, n_rows, d_need, cutoff, q_block, grid,
                         d_queries, d_rows, d_common, capacity, d_result, d_workspace, workspace_bytes};
        uint64_t hits = 0;
        hip_check(many_overlap_run(a, &hits, nullptr, (hipStream_t)stream), "many_overlap");
        ret = hits;
    });
    return ret;
}

void smgpu_many_sizes_raw(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n, uint64_t cutoff, uint64_t* d_sizes, void* stream) {
    landing_void([&] {
        if (n && (!d_offsets || !d_sizes)) throw err_internal("smgpu_many_sizes_raw: null pointer");
        (void)DeviceCtx::get();
        hip_check(many_sizes_launch(d_hashes, d_offsets, n, cutoff, d_sizes, (hipStream_t)stream), "many_sizes");
    });
}

void smgpu_sketchset_sizes_at(const SmgpuSketchSet* p, uint64_t max_hash, uint64_t* out) {
    landing_void([&] {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (!s || (s->n && !out)) throw err_internal("smgpu_sketchset_sizes_at: null pointer");
        if (s->n == 0) return;
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        AsyncBuf d(s->n * 8, st);
        hip_check(many_sizes_launch(s->hashes.as<uint64_t>(), s->offsets.as<uint64_t>(), s->n, max_hash ? max_hash : ~0ull, d.as<uint64_t>(), st), "many_sizes");
        hip_check(hipMemcpyAsync(out, d.p, s->n * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
    });
}

void smgpu_many_set_first_capacity(uint64_t capacity) { g_first_capacity.store(capacity); }

SmgpuManyHits* smgpu_sketchset_overlaps_many(const SmgpuSketchSet* db_p, const SmgpuSketchSet* queries_p, const uint32_t* need, uint32_t need_all) {
    return landing<SmgpuManyHits*>([&]() -> SmgpuManyHits* {
        const SketchSet* db = reinterpret_cast<const SketchSet*>(db_p);
        const SketchSet* qs = reinterpret_cast<const SketchSet*>(queries_p);
        if (!db || !qs) throw err_internal("smgpu_sketchset_overlaps_many: null pointer");
        check_sets_compatible(*db, *qs);
        if (!need && need_all == 0) throw err_internal("smgpu_sketchset_overlaps_many: the count a hit needs is never 0");
        const uint64_t m = qs->n, n = db->n;
        for (uint64_t q = 0; need && q < m; ++q)
            if (need[q] == 0) throw err_internal("smgpu_sketchset_overlaps_many: the count a hit needs is never 0");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        const auto t_begin = std::chrono::steady_clock::now();
        std::unique_ptr<ManyHits> h(new ManyHits());
        h->max_hash = many_cutoff(qs->max_hash, db->max_hash);
        h->query_sizes.assign(m, 0);
        h->row_sizes.assign(n, 0);
        if (m == 0 || n == 0) return reinterpret_cast<SmgpuManyHits*>(h.release());
        AsyncBuf d_qsizes(m * 8, st), d_rsizes(n * 8, st), d_need(m * 4, st);
        hip_check(many_sizes_launch(qs->hashes.as<uint64_t>(), qs->offsets.as<uint64_t>(), m, h->max_hash, d_qsizes.as<uint64_t>(), st), "many_sizes");
        hip_check(many_sizes_launch(db->hashes.as<uint64_t>(), db->offsets.as<uint64_t>(), n, h->max_hash, d_rsizes.as<uint64_t>(), st), "many_sizes");
        hip_check(hipMemcpyAsync(h->query_sizes.data(), d_qsizes.p, m * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipMemcpyAsync(h->row_sizes.data(), d_rsizes.p, n * 8, hipMemcpyDeviceToHost, st), "D2H");
        std::vector<uint32_t> need_v(need ? need : nullptr, need ? need + m : nullptr);
        if (!need) need_v.assign(m, need_all);
        hip_check(hipMemcpyAsync(d_need.p, need_v.data(), m * 4, hipMemcpyHostToDevice, st), "H2D");
        ManyDeviceHits H;
        many_hits_on_device(*db, *qs, d_need.as<uint32_t>(), h->max_hash, H, st);
        for (int i = 0; i < 3; ++i) h->ms[i] = H.ms3[i];
        h->reruns = H.reruns;
        const uint64_t hits = H.hits;
        AsyncBuf &d_q = H.queries, &d_r = H.rows, &d_c = H.common;
        h->passes = many_overlap_passes(m, 0);
        h->queries.resize(hits); h->rows.resize(hits); h->common.resize(hits);
        if (hits) {
            hip_check(hipMemcpyAsync(h->queries.data(), d_q.p, hits * 4, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipMemcpyAsync(h->rows.data(), d_r.p, hits * 4, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipMemcpyAsync(h->common.data(), d_c.p, hits * 4, hipMemcpyDeviceToHost, st), "D2H");
        }
        hip_check(hipStreamSynchronize(st), "sync");
        h->ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        return reinterpret_cast<SmgpuManyHits*>(h.release());
    });
}

void smgpu_manyhits_free(SmgpuManyHits* p) { delete reinterpret_cast<ManyHits*>(p); }
uint64_t smgpu_manyhits_len(const SmgpuManyHits* p) { return reinterpret_cast<const ManyHits*>(p)->queries.size(); }
const uint32_t* smgpu_manyhits_queries(const SmgpuManyHits* p) { return reinterpret_cast<const ManyHits*>(p)->queries.data(); }
const uint32_t* smgpu_manyhits_rows(const SmgpuManyHits* p) { return reinterpret_cast<const ManyHits*>(p)->rows.data(); }
const uint32_t* smgpu_manyhits_common(const SmgpuManyHits* p) { return reinterpret_cast<const ManyHits*>(p)->common.data(); }
const uint64_t* smgpu_manyhits_query_sizes(const SmgpuManyHits* p) { return reinterpret_cast<const ManyHits*>(p)->query_sizes.data(); }
const uint64_t* smgpu_manyhits_row_sizes(const SmgpuManyHits* p) { return reinterpret_cast<const ManyHits*>(p)->row_sizes.data(); }
uint64_t smgpu_manyhits_scaled(const SmgpuManyHits* p) {
    const uint64_t mx = reinterpret_cast<const ManyHits*>(p)->max_hash;
    return mx ? scaled_for_max_hash(mx) : 0;
}
void smgpu_manyhits_stats(const SmgpuManyHits* p, double* out6) {
    const ManyHits* h = reinterpret_cast<const ManyHits*>(p);
    if (!out6) return;
    for (int i = 0; i < 4; ++i) out6[i] = h->ms[i];
    out6[4] = (double)h->reruns;
    out6[5] = (double)h->passes;
}

}  // extern "C"
