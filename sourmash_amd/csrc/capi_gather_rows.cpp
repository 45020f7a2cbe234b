// capi_gather_rows.cpp -- the C-ABI (include/sourmash_amd.h): the integers of gather's result rows for the picks of many queries
// (gather_rows.hip, gather_rows_core.hpp).  The raw entry works on the caller's device buffers and a pick list;
// smgpu_sketchset_gather_rows_many runs the many-queries gather (capi_gather_many.cpp) on two resident sets and then the pass on
// the same buffers, smgpu_sketchset_gather_rows does the same for one query through the one-query gather (capi_gather.cpp).
#include <algorithm>
#include <chrono>
#include <memory>
#include "capi_common.hpp"
#include "gather_rows_core.hpp"

using namespace smg;

namespace {

// what a call leaves on the host: the picks of query q are [offsets[q], offsets[q + 1]) of the per-pick arrays, in rank order
struct GatherRows {
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> rows, isect, orig_common;
    std::vector<uint64_t> weighted, abund_offsets, abund_values, query_sizes, row_sizes, total_weighted;
    uint64_t max_hash = 0;
    double stats[5] = {0, 0, 0, 0, 0};            // ms: gather (host), owner, tally, sort (device), whole call (host)
};

void check_raw(const void* p, const char* what) {
    if (!p) throw err_internal(std::string("smgpu_gather_rows_raw: null pointer (") + what + ")");
}

void check_trouble(uint32_t trouble, const char* who) {
    if (!trouble) return;
    if (trouble & GR_BAD_QUERY_OFFSETS) throw err_internal(std::string(who) + ": the query offsets descend or leave the query hashes");
    if (trouble & GR_BAD_PICK_OFFSETS) throw err_internal(std::string(who) + ": the pick offsets descend or do not span the picks");
    if (trouble & GR_BAD_PICK_ROW) throw err_internal(std::string(who) + ": a pick names a row the collection does not have");
    throw err_internal(std::string(who) + ": the offsets of a picked row descend");
}

double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// The pass on resident buffers: out->offsets / rows / isect hold the picks (host); h_abunds (may be null) is aligned with the m
// queries' q_total hashes on the device.  Fills the rest of *out and checks the pass against the gather: unique == isect.
// d_resident_abunds (may be null): the same column already on the device -- an abundance set's own; nothing is uploaded then.
void rows_pass(const SketchSet& db, const uint64_t* d_qhashes, const uint64_t* d_qoffsets, uint64_t m, uint64_t q_total, const uint64_t* h_abunds,
               GatherRows* out, const char* who, hipStream_t st, const uint64_t* d_resident_abunds = nullptr) {
    const uint64_t n = db.n, n_picks = out->rows.size(), cutoff = out->max_hash;
    if (!gr_sizes_fit(m, q_total, n, n_picks)) throw err_internal(std::string(who) + ": 2^32 queries, query hashes, rows or picks are not taken");
    out->orig_common.assign(n_picks, 0);
    out->weighted.assign(n_picks, 0);
    out->abund_offsets.assign(n_picks + 1, 0);
    out->query_sizes.assign(m, 0);
    out->total_weighted.assign(m, 0);
    out->row_sizes.assign(n, 0);
    if (n) {
        AsyncBuf d_rsizes(n * 8, st);
        hip_check(many_sizes_launch(db.hashes.as<uint64_t>(), db.offsets.as<uint64_t>(), n, cutoff, d_rsizes.as<uint64_t>(), st), "many_sizes");
        hip_check(hipMemcpyAsync(out->row_sizes.data(), d_rsizes.p, n * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
    }
    if (m == 0) return;
    AsyncBuf d_pick_off((m + 1) * 8, st), d_pick_rows(n_picks * 4 + 16, st), d_abunds, d_owner(q_total * 4 + 16, st), d_orig(n_picks * 4 + 16, st),
        d_unique(n_picks * 4 + 16, st), d_weighted(n_picks * 8 + 16, st), d_aoff((n_picks + 1) * 8, st), d_avals(q_total * 8 + 16, st), d_qsizes(m * 8, st),
        d_tw(m * 8, st);
    const uint64_t ws_bytes = gather_rows_workspace_bytes(m, q_total, n_picks);
    AsyncBuf ws((size_t)ws_bytes, st);
    hip_check(hipMemcpyAsync(d_pick_off.p, out->offsets.data(), (m + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
    if (n_picks) hip_check(hipMemcpyAsync(d_pick_rows.p, out->rows.data(), n_picks * 4, hipMemcpyHostToDevice, st), "H2D");
    if (h_abunds && q_total && !d_resident_abunds) {
        d_abunds.reset(q_total * 8, st);
        hip_check(hipMemcpyAsync(d_abunds.p, h_abunds, q_total * 8, hipMemcpyHostToDevice, st), "H2D");
    }
    const GatherRowsArgs a{d_qhashes, d_resident_abunds && q_total ? d_resident_abunds : d_abunds.as<uint64_t>(), d_qoffsets, m, q_total, db.hashes.as<uint64_t>(), db.offsets.as<uint64_t>(), n,
                           d_pick_off.as<uint64_t>(), d_pick_rows.as<uint32_t>(), n_picks, cutoff, 0, d_owner.as<uint32_t>(), d_orig.as<uint32_t>(),
                           d_unique.as<uint32_t>(), d_weighted.as<uint64_t>(), d_aoff.as<uint64_t>(), d_avals.as<uint64_t>(), d_qsizes.as<uint64_t>(),
                           d_tw.as<uint64_t>(), ws.p, ws_bytes};
    uint64_t owned = 0;
    uint32_t trouble = 0;
    float ms3[3];
    hip_check(gather_rows_run(a, &owned, &trouble, ms3, st), "gather_rows");
    check_trouble(trouble, who);
    for (int i = 0; i < 3; ++i) out->stats[1 + i] = ms3[i];
    std::vector<uint32_t> unique(n_picks);
    out->abund_values.assign(owned, 0);
    if (n_picks) {
        hip_check(hipMemcpyAsync(out->orig_common.data(), d_orig.p, n_picks * 4, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipMemcpyAsync(unique.data(), d_unique.p, n_picks * 4, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipMemcpyAsync(out->weighted.data(), d_weighted.p, n_picks * 8, hipMemcpyDeviceToHost, st), "D2H");
    }
    hip_check(hipMemcpyAsync(out->abund_offsets.data(), d_aoff.p, (n_picks + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipMemcpyAsync(out->query_sizes.data(), d_qsizes.p, m * 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipMemcpyAsync(out->total_weighted.data(), d_tw.p, m * 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    if (owned) HostXfer::get().device_to_host(out->abund_values.data(), d_avals.p, owned * 8, st);
    for (uint64_t p = 0; p < n_picks; ++p)
        if (unique[p] != out->isect[p])
            throw err_internal(std::string(who) + ": a pick owns another number of query hashes than the gather reported for it");
    if (out->abund_offsets[n_picks] != owned) throw err_internal(std::string(who) + ": the picks' hashes do not add up to the owned hashes");
}

const GatherRows* GR(const SmgpuGatherRows* p) { return reinterpret_cast<const GatherRows*>(p); }

}  // namespace

extern "C" {

uint64_t smgpu_gather_rows_workspace_bytes(uint64_t m, uint64_t q_total, uint64_t n_picks) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        if (!gr_sizes_fit(m, q_total, 0, n_picks)) throw err_internal("smgpu_gather_rows_workspace_bytes: 2^32 queries, query hashes or picks are not taken");
        ret = gather_rows_workspace_bytes(m, q_total, n_picks);
    });
    return ret;
}

uint64_t smgpu_gather_rows_raw(const uint64_t* d_qhashes, const uint64_t* d_qabunds, const uint64_t* d_qoffsets, uint64_t m, uint64_t q_total,
                               const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n_rows, const uint64_t* d_pick_offsets,
                               const uint32_t* d_pick_rows, uint64_t n_picks, uint64_t cutoff, uint32_t grid, uint32_t* d_owner, uint32_t* d_orig_common,
                               uint32_t* d_unique, uint64_t* d_weighted, uint64_t* d_abund_offsets, uint64_t* d_abund_values, uint64_t* d_query_sizes,
                               uint64_t* d_total_weighted, void* d_workspace, uint64_t workspace_bytes, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        check_raw(d_workspace, "d_workspace");
        check_raw(d_abund_offsets, "d_abund_offsets");
        if (m) {
            check_raw(d_qoffsets, "d_qoffsets"); check_raw(d_pick_offsets, "d_pick_offsets");
            check_raw(d_query_sizes, "d_query_sizes"); check_raw(d_total_weighted, "d_total_weighted");
        }
        if (q_total) { check_raw(d_qhashes, "d_qhashes"); check_raw(d_owner, "d_owner"); check_raw(d_abund_values, "d_abund_values"); }
        if (n_picks) {
            check_raw(d_hashes, "d_hashes"); check_raw(d_offsets, "d_offsets"); check_raw(d_pick_rows, "d_pick_rows");
            check_raw(d_orig_common, "d_orig_common"); check_raw(d_unique, "d_unique"); check_raw(d_weighted, "d_weighted");
        }
        if (grid > (1u << 20)) throw err_internal("smgpu_gather_rows_raw: grid above 1048576 workgroups");
        if (!gr_sizes_fit(m, q_total, n_rows, n_picks)) throw err_internal("smgpu_gather_rows_raw: 2^32 queries, query hashes, rows or picks are not taken");
        if (m == 0 && n_picks) throw err_internal("smgpu_gather_rows_raw: picks without a query");
        if (workspace_bytes < gather_rows_workspace_bytes(m, q_total, n_picks))
            throw err_internal("smgpu_gather_rows_raw: the workspace is smaller than smgpu_gather_rows_workspace_bytes says");
        (void)DeviceCtx::get();                                      // no device: say so, not "invalid device"
        const GatherRowsArgs a{d_qhashes, d_qabunds, d_qoffsets, m, q_total, d_hashes, d_offsets, n_rows, d_pick_offsets, d_pick_rows, n_picks, cutoff, grid,
                               d_owner, d_orig_common, d_unique, d_weighted, d_abund_offsets, d_abund_values, d_query_sizes, d_total_weighted, d_workspace,
                               workspace_bytes};
        uint64_t owned = 0;
        uint32_t trouble = 0;
        hip_check(gather_rows_run(a, &owned, &trouble, nullptr, (hipStream_t)stream), "gather_rows");
        check_trouble(trouble, "smgpu_gather_rows_raw");
        ret = owned;
    });
    return ret;
}

SmgpuGatherRows* smgpu_sketchset_gather_rows_many(const SmgpuSketchSet* db_p, const SmgpuSketchSet* queries_p, const uint64_t* abunds,
                                                  uint64_t threshold_hashes) {
    return smgpu_sketchset_gather_rows_many_resident(db_p, queries_p, abunds, threshold_hashes, 0);
}

SmgpuGatherRows* smgpu_sketchset_gather_rows_many_resident(const SmgpuSketchSet* db_p, const SmgpuSketchSet* queries_p, const uint64_t* abunds,
                                                           uint64_t threshold_hashes, uint32_t use_resident) {
    return landing<SmgpuGatherRows*>([&]() -> SmgpuGatherRows* {
        const SketchSet* db = reinterpret_cast<const SketchSet*>(db_p);
        const SketchSet* qs = reinterpret_cast<const SketchSet*>(queries_p);
        if (!db || !qs) throw err_internal("smgpu_sketchset_gather_rows_many: null pointer");
        if (use_resident && abunds) throw err_internal("smgpu_sketchset_gather_rows_many_resident: the set's own abundances, or an array, not both");
        if (use_resident && !qs->has_abunds()) throw err_internal("smgpu_sketchset_gather_rows_many_resident: the queries are a flat set");
        check_sets_compatible(*db, *qs);
        const auto t_begin = std::chrono::steady_clock::now();
        // ---- the picks: the many-queries gather itself (its error, if any, stands in the thread's slot)
        SmgpuManyGather* picks = smgpu_sketchset_gather_many(db_p, queries_p, threshold_hashes);
        if (!picks) return nullptr;
        std::unique_ptr<SmgpuManyGather, void (*)(SmgpuManyGather*)> hold(picks, smgpu_manygather_free);
        const uint64_t m = qs->n;
        std::unique_ptr<GatherRows> out(new GatherRows());
        out->max_hash = many_cutoff(qs->max_hash, db->max_hash);
        const uint64_t* off = smgpu_manygather_offsets(picks);
        out->offsets.assign(off, off + m + 1);
        const uint64_t n_picks = out->offsets[m];
        out->rows.assign(smgpu_manygather_rows(picks), smgpu_manygather_rows(picks) + n_picks);
        out->isect.assign(smgpu_manygather_isect(picks), smgpu_manygather_isect(picks) + n_picks);
        out->stats[0] = ms_since(t_begin);
        // ---- the pass, on the buffers the gather worked on
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        // (use_resident: the queries' own abundance column is the pass's d_qabunds -- no host array, no upload)
        rows_pass(*db, qs->hashes.as<uint64_t>(), qs->offsets.as<uint64_t>(), m, qs->total, abunds, out.get(), "smgpu_sketchset_gather_rows_many", ctx.stream(),
                  use_resident ? qs->abunds.as<uint64_t>() : nullptr);
        out->stats[4] = ms_since(t_begin);
        return reinterpret_cast<SmgpuGatherRows*>(out.release());
    });
}

SmgpuGatherRows* smgpu_sketchset_gather_rows(const SmgpuSketchSet* db_p, const SourmashKmerMinHash* query, uint64_t threshold_hashes) {
    return landing<SmgpuGatherRows*>([&]() -> SmgpuGatherRows* {
        const SketchSet* db = reinterpret_cast<const SketchSet*>(db_p);
        if (!db || !query) throw err_internal("smgpu_sketchset_gather_rows: null pointer");
        const KmerMinHash* mh = MH(query);                           // queued records are hashed before the context is taken
        check_sketch_compatible(*db, *mh);
        const auto t_begin = std::chrono::steady_clock::now();
        std::unique_ptr<GatherRows> out(new GatherRows());
        out->max_hash = many_cutoff(mh->max_hash, db->max_hash);
        out->offsets.assign(2, 0);
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        const uint64_t nq = mh->mins.size();
        const uint64_t nq_cut = many_cut_len(mh->mins.data(), nq, out->max_hash);
        AsyncBuf d_q(nq * 8 + 16, st), d_qoff(16, st);
        const uint64_t qoff[2] = {0, nq};
        if (nq) hip_check(hipMemcpyAsync(d_q.p, mh->mins.data(), nq * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipMemcpyAsync(d_qoff.p, qoff, 16, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipStreamSynchronize(st), "sync");                  // (qoff leaves the stack)
        // ---- the picks: the one-query gather on the query's hashes <= cutoff (a row's hashes above it meet nothing there)
        if (nq_cut && db->n) {
            std::vector<uint64_t> idx, isect;
            gather_one_on_device(d_q.as<uint64_t>(), nq_cut, *db, threshold_hashes, idx, isect, st);
            for (size_t i = 0; i < idx.size(); ++i) {
                out->rows.push_back((uint32_t)idx[i]);
                out->isect.push_back((uint32_t)isect[i]);
            }
        }
        out->offsets[1] = out->rows.size();
        out->stats[0] = ms_since(t_begin);
        const bool with_abunds = mh->track_abundance && mh->abunds.size() == nq;
        rows_pass(*db, d_q.as<uint64_t>(), d_qoff.as<uint64_t>(), 1, nq, with_abunds ? mh->abunds.data() : nullptr, out.get(), "smgpu_sketchset_gather_rows", st);
        out->stats[4] = ms_since(t_begin);
        return reinterpret_cast<SmgpuGatherRows*>(out.release());
    });
}

void smgpu_gatherrows_free(SmgpuGatherRows* p) { delete reinterpret_cast<GatherRows*>(p); }
uint64_t smgpu_gatherrows_queries(const SmgpuGatherRows* p) { return GR(p)->offsets.size() - 1; }
uint64_t smgpu_gatherrows_n_rows(const SmgpuGatherRows* p) { return GR(p)->row_sizes.size(); }
const uint64_t* smgpu_gatherrows_offsets(const SmgpuGatherRows* p) { return GR(p)->offsets.data(); }
const uint32_t* smgpu_gatherrows_rows(const SmgpuGatherRows* p) { return GR(p)->rows.data(); }
const uint32_t* smgpu_gatherrows_isect(const SmgpuGatherRows* p) { return GR(p)->isect.data(); }
const uint32_t* smgpu_gatherrows_orig_common(const SmgpuGatherRows* p) { return GR(p)->orig_common.data(); }
const uint64_t* smgpu_gatherrows_weighted(const SmgpuGatherRows* p) { return GR(p)->weighted.data(); }
const uint64_t* smgpu_gatherrows_abund_offsets(const SmgpuGatherRows* p) { return GR(p)->abund_offsets.data(); }
const uint64_t* smgpu_gatherrows_abund_values(const SmgpuGatherRows* p) { return GR(p)->abund_values.data(); }
const uint64_t* smgpu_gatherrows_query_sizes(const SmgpuGatherRows* p) { return GR(p)->query_sizes.data(); }
const uint64_t* smgpu_gatherrows_row_sizes(const SmgpuGatherRows* p) { return GR(p)->row_sizes.data(); }
const uint64_t* smgpu_gatherrows_total_weighted(const SmgpuGatherRows* p) { return GR(p)->total_weighted.data(); }
uint64_t smgpu_gatherrows_scaled(const SmgpuGatherRows* p) {
    const uint64_t mx = GR(p)->max_hash;
    return mx ? scaled_for_max_hash(mx) : 0;
}
void smgpu_gatherrows_stats(const SmgpuGatherRows* p, double* out5) {
    if (!out5) return;
    for (int i = 0; i < 5; ++i) out5[i] = GR(p)->stats[i];
}

}  // extern "C"
