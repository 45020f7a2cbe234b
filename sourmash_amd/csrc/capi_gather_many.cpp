// capi_gather_many.cpp -- the C-ABI (include/sourmash_amd.h): gather of many queries against a collection in one call
// (gather_many.hip, gather_many_core.hpp).  The raw entry works on the caller's device buffers and the hits of
// smgpu_many_overlap_raw; smgpu_sketchset_gather_many takes two resident sets, finds the candidates with the many-queries pass,
// cuts the queries into batches, runs the queries beyond the caps of the LDS form through the one-query path (capi_gather.cpp),
// and leaves the picks on the host.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include "capi_common.hpp"
#include "gather_many_core.hpp"

using namespace smg;

namespace {

// what a call leaves on the host: the picks of query q are [offsets[q], offsets[q + 1]) of rows / isect, in rank order
struct ManyGather {
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> rows, isect;
    uint64_t max_hash = 0;
    double stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // ms: candidates, fill, sort, rounds (device), way out, whole call (host); way-out queries; batches
};

// test support: smgpu_gather_many_set_limits (0: the default)
std::atomic<uint32_t> g_max_query_hashes{0}, g_max_candidates{0};
std::atomic<uint64_t> g_batch_common{0};

void check_raw(const void* p, const char* what) {
    if (!p) throw err_internal(std::string("smgpu_gather_many_raw: null pointer (") + what + ")");
}

void check_trouble(uint32_t trouble, const char* who) {
    switch (trouble) {
    case GM_OK: return;
    case GM_FILL_MISMATCH:
        throw err_internal(std::string(who) + ": a row shares another number of hashes with its query than its hit says (the hits are not those of these sets)");
    case GM_TOO_MANY_ENTRIES: throw err_internal(std::string(who) + ": the hits' common counts sum to 2^32 or more");
    default: throw err_internal(std::string(who) + ": the workspace is smaller than smgpu_gather_many_workspace_bytes says for these hits");
    }
}

double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

}  // namespace

extern "C" {

void smgpu_gather_many_geometry(uint32_t* workgroup, uint32_t* max_query_hashes, uint32_t* max_candidates) {
    if (workgroup) *workgroup = GM_BLOCK;
    if (max_query_hashes) *max_query_hashes = GM_MAX_QUERY_HASHES;
    if (max_candidates) *max_candidates = GM_MAX_CANDIDATES;
}

uint64_t smgpu_gather_many_workspace_bytes(uint64_t m, uint64_t n_hits, uint64_t total_common) {
    return gather_many_workspace_bytes(m, n_hits, total_common);
}

void smgpu_gather_many_set_limits(uint32_t max_query_hashes, uint32_t max_candidates, uint64_t batch_common) {
    g_max_query_hashes.store(max_query_hashes);
    g_max_candidates.store(max_candidates);
    g_batch_common.store(batch_common);
}

uint64_t smgpu_gather_many_raw(const uint64_t* d_qhashes, const uint64_t* d_qoffsets, uint64_t m, const uint64_t* d_hashes, const uint64_t* d_offsets,
                               uint64_t n_rows, const uint32_t* d_hit_queries, const uint32_t* d_hit_rows, const uint32_t* d_hit_common, uint64_t n_hits,
                               uint64_t cutoff, uint64_t threshold_hashes, uint32_t max_query_hashes, uint32_t max_candidates, uint32_t grid,
                               uint32_t* d_out_rows, uint32_t* d_out_isect, uint32_t* d_out_rounds, uint32_t* d_status, void* d_workspace,
                               uint64_t workspace_bytes, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        check_raw(d_workspace, "d_workspace");
        if (m) { check_raw(d_qoffsets, "d_qoffsets"); check_raw(d_qhashes, "d_qhashes"); check_raw(d_out_rounds, "d_out_rounds"); check_raw(d_status, "d_status"); }
        if (n_hits) {
            check_raw(d_hashes, "d_hashes"); check_raw(d_offsets, "d_offsets");
            check_raw(d_hit_queries, "d_hit_queries"); check_raw(d_hit_rows, "d_hit_rows"); check_raw(d_hit_common, "d_hit_common");
            check_raw(d_out_rows, "d_out_rows"); check_raw(d_out_isect, "d_out_isect");
        }
        const uint32_t mqh = max_query_hashes ? max_query_hashes : GM_MAX_QUERY_HASHES, mc = max_candidates ? max_candidates : GM_MAX_CANDIDATES;
        if (!gm_caps_fit(mqh, mc))
            throw err_internal("smgpu_gather_many_raw: the caps ask for more than " + std::to_string(GM_LDS_LIMIT) + " bytes of LDS a workgroup");
        if (grid > (1u << 20)) throw err_internal("smgpu_gather_many_raw: grid above 1048576 workgroups");
        if (m >= GM_INDEX_LIMIT || n_rows >= GM_INDEX_LIMIT || n_hits >= GM_INDEX_LIMIT)
            throw err_internal("smgpu_gather_many_raw: 2^32 queries, rows or hits are not taken");
        if (workspace_bytes < gather_many_workspace_bytes(m, n_hits, 0))
            throw err_internal("smgpu_gather_many_raw: the workspace is smaller than smgpu_gather_many_workspace_bytes says");
        (void)DeviceCtx::get();                                      // no device: say so, not "invalid device"
        const GatherManyArgs a{d_qhashes, d_qoffsets, m, 0, d_hashes, d_offsets, n_rows, d_hit_queries, d_hit_rows, d_hit_common, n_hits, cutoff,
                               threshold_hashes, mqh, mc, grid, d_out_rows, d_out_isect, d_out_rounds, d_status, d_workspace, workspace_bytes};
        uint64_t total = 0;
        uint32_t trouble = GM_OK;
        hip_check(gather_many_run(a, &total, &trouble, nullptr, (hipStream_t)stream), "gather_many");
        check_trouble(trouble, "smgpu_gather_many_raw");
        ret = total;
    });
    return ret;
}

SmgpuManyGather* smgpu_sketchset_gather_many(const SmgpuSketchSet* db_p, const SmgpuSketchSet* queries_p, uint64_t threshold_hashes) {
    return landing<SmgpuManyGather*>([&]() -> SmgpuManyGather* {
        const SketchSet* db = reinterpret_cast<const SketchSet*>(db_p);
        const SketchSet* qs = reinterpret_cast<const SketchSet*>(queries_p);
        if (!db || !qs) throw err_internal("smgpu_sketchset_gather_many: null pointer");
        check_sets_compatible(*db, *qs);
        const uint64_t m = qs->n, n = db->n;
        std::unique_ptr<ManyGather> out(new ManyGather());
        out->max_hash = many_cutoff(qs->max_hash, db->max_hash);
        out->offsets.assign(m + 1, 0);
        if (m == 0 || n == 0) return reinterpret_cast<SmgpuManyGather*>(out.release());
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        const auto t_begin = std::chrono::steady_clock::now();
        const uint64_t cutoff = out->max_hash;

        // ---- the candidates: a row whose overlap is below the threshold can never be picked (counters only fall), and leaving it
        // out changes no other counter.  The hits stay on the device.
        const uint32_t need = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, threshold_hashes), 0xffffffffull);
        const std::vector<uint32_t> need_v(m, need);
        AsyncBuf d_need(m * 4, st);
        hip_check(hipMemcpyAsync(d_need.p, need_v.data(), m * 4, hipMemcpyHostToDevice, st), "H2D");
        ManyDeviceHits H;
        many_hits_on_device(*db, *qs, d_need.as<uint32_t>(), cutoff, H, st);
        out->stats[0] = (double)H.ms3[0] + H.ms3[1] + H.ms3[2];
        const uint64_t hits = H.hits;
        if (hits == 0) {
            out->stats[5] = ms_since(t_begin);
            return reinterpret_cast<SmgpuManyGather*>(out.release());
        }

        // ---- per query: its hits, its size at the common scaled, whether the LDS form takes it, the entries it needs
        const uint32_t mqh = g_max_query_hashes.load() ? g_max_query_hashes.load() : GM_MAX_QUERY_HASHES;
        const uint32_t mc = g_max_candidates.load() ? g_max_candidates.load() : GM_MAX_CANDIDATES;
        const uint64_t budget = g_batch_common.load() ? g_batch_common.load() : GM_BATCH_COMMON;
        if (!gm_caps_fit(mqh, mc)) throw err_internal("smgpu_gather_many_set_limits: the caps ask for more LDS than a workgroup may take");
        AsyncBuf d_qlo((m + 2) * 4, st), d_qn((m + 1) * 4, st), d_status((m + 1) * 4, st), d_sums((m + 1) * 8, st), d_rounds((m + 1) * 4, st);
        AsyncBuf d_out_rows(hits * 4 + 16, st), d_out_isect(hits * 4 + 16, st);
        hip_check(gather_many_plan(qs->hashes.as<uint64_t>(), qs->offsets.as<uint64_t>(), m, H.queries.as<uint32_t>(), H.common.as<uint32_t>(), hits, cutoff,
                                   mqh, mc, d_qlo.as<uint32_t>(), d_qn.as<uint32_t>(), d_status.as<uint32_t>(), d_sums.as<uint64_t>(), st), "gather_many plan");
        hip_check(hipMemsetAsync(d_rounds.p, 0, (m + 1) * 4, st), "memset");
        std::vector<uint32_t> qlo(m + 1), qn(m), status(m), rounds(m);
        std::vector<uint64_t> sums(m), qoff(m + 1);
        hip_check(hipMemcpyAsync(qlo.data(), d_qlo.p, (m + 1) * 4, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipMemcpyAsync(qn.data(), d_qn.p, m * 4, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipMemcpyAsync(status.data(), d_status.p, m * 4, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipMemcpyAsync(sums.data(), d_sums.p, m * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipMemcpyAsync(qoff.data(), qs->offsets.p, (m + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");

        // ---- batches: contiguous ranges of queries whose entries stay under the budget; a query that alone would reach 2^32
        // entries stands in no range and takes the way out
        std::vector<uint64_t> weight(m);
        std::vector<uint8_t> alone(m, 0);
        for (uint64_t q = 0; q < m; ++q) {
            weight[q] = status[q] ? 0 : sums[q];
            if (weight[q] >= GM_INDEX_LIMIT) { alone[q] = 1; status[q] = 1; }
        }
        struct Range { uint64_t q0, q1, entries; };
        std::vector<Range> ranges;
        uint64_t ws_bytes = 0;
        for (uint64_t q = 0; q < m;) {
            if (alone[q]) { ++q; continue; }
            uint64_t lim = q;
            while (lim < m && !alone[lim]) ++lim;
            const uint64_t q1 = gm_batch_end(weight.data(), lim, q, budget);
            uint64_t entries = 0;
            for (uint64_t i = q; i < q1; ++i) entries += weight[i];
            if (entries) {
                ranges.push_back({q, q1, entries});
                ws_bytes = std::max<uint64_t>(ws_bytes, gather_many_workspace_bytes(q1 - q, qlo[q1] - qlo[q], entries));
            }
            q = q1;
        }
        AsyncBuf ws;
        if (ws_bytes) ws.reset((size_t)ws_bytes, st);
        for (const Range& r : ranges) {
            const uint64_t h0 = qlo[r.q0], hb = qlo[r.q1] - h0;
            const GatherManyArgs a{qs->hashes.as<uint64_t>(), qs->offsets.as<uint64_t>() + r.q0, r.q1 - r.q0, (uint32_t)r.q0, db->hashes.as<uint64_t>(),
                                   db->offsets.as<uint64_t>(), n, H.queries.as<uint32_t>() + h0, H.rows.as<uint32_t>() + h0, H.common.as<uint32_t>() + h0,
                                   hb, cutoff, threshold_hashes, mqh, mc, 0, d_out_rows.as<uint32_t>() + h0, d_out_isect.as<uint32_t>() + h0,
                                   d_rounds.as<uint32_t>() + r.q0, d_status.as<uint32_t>() + r.q0, ws.p, ws_bytes};
            uint64_t total = 0;
            uint32_t trouble = GM_OK;
            float ms3[3];
            hip_check(gather_many_run(a, &total, &trouble, ms3, st), "gather_many");
            check_trouble(trouble, "smgpu_sketchset_gather_many");
            for (int i = 0; i < 3; ++i) out->stats[1 + i] += ms3[i];
        }
        out->stats[7] = (double)ranges.size();
        std::vector<uint32_t> pick_rows(hits), pick_isect(hits);
        if (!ranges.empty()) {
            hip_check(hipMemcpyAsync(pick_rows.data(), d_out_rows.p, hits * 4, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipMemcpyAsync(pick_isect.data(), d_out_isect.p, hits * 4, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipMemcpyAsync(rounds.data(), d_rounds.p, m * 4, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
        }

        // ---- the answer, query by query; the queries beyond a cap run through the one-query path on the resident buffers,
        // restricted to their hashes <= cutoff (the rows' hashes above it meet nothing in such a query)
        std::vector<uint64_t> one_idx, one_isect;
        for (uint64_t q = 0; q < m; ++q) {
            const uint64_t nc = qlo[q + 1] - qlo[q];
            if (status[q] && nc) {
                const auto t_one = std::chrono::steady_clock::now();
                gather_one_on_device(qs->hashes.as<uint64_t>() + qoff[q], qn[q], *db, threshold_hashes, one_idx, one_isect, st);
                for (size_t i = 0; i < one_idx.size(); ++i) {
                    out->rows.push_back((uint32_t)one_idx[i]);
                    out->isect.push_back((uint32_t)one_isect[i]);
                }
                out->stats[4] += ms_since(t_one);
                out->stats[6] += 1;
            } else if (!status[q]) {
                const uint32_t k = rounds[q];
                if (k > nc) throw err_internal("smgpu_sketchset_gather_many: a query has more rounds than candidates");
                out->rows.insert(out->rows.end(), pick_rows.begin() + qlo[q], pick_rows.begin() + qlo[q] + k);
                out->isect.insert(out->isect.end(), pick_isect.begin() + qlo[q], pick_isect.begin() + qlo[q] + k);
            }
            out->offsets[q + 1] = out->rows.size();
        }
        out->stats[5] = ms_since(t_begin);
        return reinterpret_cast<SmgpuManyGather*>(out.release());
    });
}

void smgpu_manygather_free(SmgpuManyGather* p) { delete reinterpret_cast<ManyGather*>(p); }
const uint64_t* smgpu_manygather_offsets(const SmgpuManyGather* p) { return reinterpret_cast<const ManyGather*>(p)->offsets.data(); }
const uint32_t* smgpu_manygather_rows(const SmgpuManyGather* p) { return reinterpret_cast<const ManyGather*>(p)->rows.data(); }
const uint32_t* smgpu_manygather_isect(const SmgpuManyGather* p) { return reinterpret_cast<const ManyGather*>(p)->isect.data(); }
uint64_t smgpu_manygather_scaled(const SmgpuManyGather* p) {
    const uint64_t mx = reinterpret_cast<const ManyGather*>(p)->max_hash;
    return mx ? scaled_for_max_hash(mx) : 0;
}
void smgpu_manygather_stats(const SmgpuManyGather* p, double* out8) {
    if (!out8) return;
    for (int i = 0; i < 8; ++i) out8[i] = reinterpret_cast<const ManyGather*>(p)->stats[i];
}

}  // extern "C"
