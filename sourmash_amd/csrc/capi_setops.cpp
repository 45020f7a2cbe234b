// capi_setops.cpp -- the C-ABI (include/sourmash_amd.h): set algebra on resident collections (setops.hip, setops_core.hpp).  The raw
// entries work on the caller's device buffers; the set-level entries take resident sets and return a new one -- merged by group,
// intersected with or reduced by another sketch or set, or downsampled -- with host offsets and manifest rows like a loaded set.
#include <algorithm>
#include <memory>
#include "capi_common.hpp"
#include "setops_core.hpp"

using namespace smg;

namespace {

void check_raw(const void* p, const char* entry, const char* what) {
    if (!p) throw err_internal(std::string(entry) + ": null pointer (" + what + ")");
}

void need_params(const SketchSet& s) {
    if (s.ksize == 0) throw err_internal("the set's sketches do not share one set of parameters");
}

// The filter of a resident set against one sketch on the device (d_other[0, other_len)) or a second set row by row.  An abundance
// receiver carries its column: the kept hashes keep their own abundances (the other side's stay ignored).
SketchSet* filter_set(const SketchSet& s, const uint64_t* d_other_hashes, const uint64_t* d_other_offsets, uint64_t other_len, uint32_t keep_present,
                      hipStream_t st) {
    return sketchset_filter_values(s, d_other_hashes, d_other_offsets, other_len, keep_present,
                                   s.has_abunds() ? SETOPS_VALUES_CARRY : SETOPS_VALUES_NONE, nullptr, 0, ~0ull, st);
}

}  // namespace

namespace smg {

// the reference's order (check_compatible, minhash.rs:886-912) with max_hash always compared: sig subtract / sig intersect refuse
// sketches of different scaled (is_compatible), and the caller downsamples first
void check_filter_compatible(const SketchSet& s, uint32_t ksize, uint32_t hash_function, uint64_t max_hash, uint64_t seed) {
    if (s.ksize * (s.hash_function == HF_DNA ? 1u : 3u) != ksize) throw err_mismatch_ksizes();
    if (s.hash_function != hash_function) throw err_mismatch_dnaprot();
    if (s.max_hash != max_hash) throw err_mismatch_scaled();
    if (s.seed != seed) throw err_mismatch_seed();
}

std::unique_ptr<SketchSet> sketchset_like(const SketchSet& s, uint64_t n) {
    std::unique_ptr<SketchSet> out(new SketchSet());
    out->n = n;
    out->ksize = s.ksize; out->hash_function = s.hash_function; out->seed = s.seed; out->max_hash = s.max_hash; out->num = s.num;
    return out;
}

// (a row's md5 is that of other hashes and is dropped)
void sketchset_finish_rows(SketchSet& out, const SketchSet* from) {
    out.rows.assign(out.n, ManifestRow());
    for (uint64_t r = 0; r < out.n; ++r) {
        ManifestRow& m = out.rows[r];
        if (from && from->rows.size() == out.n) m = from->rows[r];
        m.md5.clear();
        m.internal_location.clear();
        m.ksize = out.ksize; m.moltype = molecule_name(out.hash_function); m.num = out.num;
        m.scaled = out.max_hash ? scaled_for_max_hash(out.max_hash) : 0;
        m.with_abundance = out.has_abunds();
        m.n_hashes = out.host_offsets[r + 1] - out.host_offsets[r];
    }
}

void sketchset_fetch_offsets(SketchSet& out, hipStream_t st) {
    out.host_offsets.assign(out.n + 1, 0);
    hip_check(hipMemcpyAsync(out.host_offsets.data(), out.offsets.p, (out.n + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    out.total = out.host_offsets[out.n];
}

// One filter for every value mode (setops_core.hpp: SetopsValueMode): count, room, write; the result carries an abundance column
// whenever the mode moves values.  abund_max of the result: the source's (a bound is all the angular kernels need).
SketchSet* sketchset_filter_values(const SketchSet& s, const uint64_t* d_other_hashes, const uint64_t* d_other_offsets, uint64_t other_len,
                                   uint32_t keep_present, uint32_t values, const uint64_t* d_other_abunds, uint64_t range_lo, uint64_t range_hi,
                                   hipStream_t st, uint64_t abund_max) {
    std::unique_ptr<SketchSet> out = sketchset_like(s, s.n);
    out->offsets.reserve((s.n + 1) * 8, st);
    const uint64_t ws_bytes = setops_filter_workspace_bytes(s.n, s.total, d_other_offsets ? 0 : other_len);
    AsyncBuf ws((size_t)ws_bytes, st), d_result(64, st);
    SetopsFilterArgs a{s.hashes.as<uint64_t>(), s.offsets.as<uint64_t>(), s.n, s.total, d_other_hashes, d_other_offsets, other_len,
                       keep_present, 0, out->offsets.as<uint64_t>(), d_result.as<uint64_t>(), ws.p, ws_bytes};
    a.values = values; a.d_abunds = s.abunds.as<uint64_t>(); a.d_other_abunds = d_other_abunds; a.range_lo = range_lo; a.range_hi = range_hi;
    SetopsFilterState state;
    uint64_t total = 0;
    hip_check(setops_filter_count(a, state, &total, st), "setops_filter (count)");
    out->hashes.reserve(total * 8 + 16, st);
    if (values != SETOPS_VALUES_NONE) {
        out->abunds.reserve(total * 8 + 16, st);
        out->abund_max = values == SETOPS_VALUES_TAKE ? abund_max : s.abund_max;
    }
    uint32_t trouble = 0;
    hip_check(setops_filter_write(a, state, out->hashes.as<uint64_t>(), total, &trouble, st, out->abunds.as<uint64_t>()), "setops_filter (write)");
    if (trouble) throw err_internal("the filter wrote another number of hashes than it had counted");
    sketchset_fetch_offsets(*out, st);
    if (out->total != total) throw err_internal("the filter's offsets do not end at its total");
    sketchset_finish_rows(*out, &s);
    return out.release();
}

}  // namespace smg

extern "C" {

void smgpu_setops_geometry(uint32_t* workgroup, uint32_t* lds_partner, uint64_t* split) {
    if (workgroup) *workgroup = SETOPS_BLOCK;
    if (lds_partner) *lds_partner = SETOPS_LDS_PARTNER;
    if (split) *split = SETOPS_SPLIT;
}

void smgpu_setops_key_form(uint64_t max_hash, uint64_t n_groups, uint32_t* hbits, uint32_t* gbits, uint32_t* packed) {
    const SetopsKeyForm f = setops_key_form(max_hash, n_groups);
    if (hbits) *hbits = f.hbits;
    if (gbits) *gbits = f.gbits;
    if (packed) *packed = f.packed ? 1u : 0u;
}

uint64_t smgpu_setops_merge_workspace_bytes(uint64_t total, uint64_t n_groups) { return setops_merge_workspace_bytes(total, n_groups); }

uint64_t smgpu_setops_merge_values_workspace_bytes(uint64_t total, uint64_t n_groups) { return setops_merge_values_workspace_bytes(total, n_groups); }

uint64_t smgpu_setops_merge_raw(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n, uint64_t total, const uint32_t* d_groups, uint64_t n_groups,
                                const uint32_t* d_need, uint32_t need_all, uint64_t max_hash, uint64_t num, uint64_t* d_out_hashes,
                                uint64_t* d_out_offsets, uint64_t* d_result, void* d_workspace, uint64_t workspace_bytes, void* stream) {
    return smgpu_setops_merge_values_raw(d_hashes, nullptr, d_offsets, n, total, d_groups, n_groups, d_need, need_all, max_hash, num, SETOPS_MERGE_FLAT,
                                         d_out_hashes, nullptr, d_out_offsets, d_result, d_workspace, workspace_bytes, stream);
}

uint64_t smgpu_setops_merge_values_raw(const uint64_t* d_hashes, const uint64_t* d_abunds, const uint64_t* d_offsets, uint64_t n, uint64_t total,
                                       const uint32_t* d_groups, uint64_t n_groups, const uint32_t* d_need, uint32_t need_all, uint64_t max_hash,
                                       uint64_t num, uint32_t values, uint64_t* d_out_hashes, uint64_t* d_out_abunds, uint64_t* d_out_offsets,
                                       uint64_t* d_result, void* d_workspace, uint64_t workspace_bytes, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        const char* me = values ? "smgpu_setops_merge_values_raw" : "smgpu_setops_merge_raw";
        if (values > SETOPS_MERGE_COUNT) throw err_internal(std::string(me) + ": values is 0 (flat), 1 (sum) or 2 (count)");
        if (values == SETOPS_MERGE_SUM && total) check_raw(d_abunds, me, "d_abunds");
        if (values && total) check_raw(d_out_abunds, me, "d_out_abunds");
        check_raw(d_result, me, "d_result");
        check_raw(d_workspace, me, "d_workspace");
        check_raw(d_out_offsets, me, "d_out_offsets");
        if (n) check_raw(d_offsets, me, "d_offsets");
        if (total) { check_raw(d_hashes, me, "d_hashes"); check_raw(d_out_hashes, me, "d_out_hashes"); }
        if (total > SETOPS_MERGE_MAX_HASHES || n >= 0xffffffffull || n_groups > 0xfffffffeull)
            throw err_internal(std::string(me) + ": 2^32 hashes, rows or groups are not taken");
        if (n && n_groups == 0) throw err_internal(std::string(me) + ": rows without a group");
        if (num && (need_all || d_need)) throw err_internal(std::string(me) + ": a num cut goes with the union only");
        if (workspace_bytes < (values ? setops_merge_values_workspace_bytes(total, n_groups) : setops_merge_workspace_bytes(total, n_groups)))
            throw err_internal(std::string(me) + ": the workspace is smaller than smgpu_setops_merge_" + (values ? "values_" : "") + "workspace_bytes says");
        (void)DeviceCtx::get();                                      // no device: say so, not "invalid device"
        hipStream_t st = (hipStream_t)stream;
        if (n) {
            // what the kernels index with is checked first: the offsets' ends against `total`, every group against n_groups
            uint64_t ends[2] = {0, 0};
            hip_check(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipMemcpyAsync(&ends[1], d_offsets + n, 8, hipMemcpyDeviceToHost, st), "D2H");
            std::vector<uint32_t> groups(d_groups ? n : 0);
            if (d_groups) hip_check(hipMemcpyAsync(groups.data(), d_groups, n * 4, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
            if (ends[1] < ends[0] || ends[1] - ends[0] != total) throw err_internal(std::string(me) + ": the offsets do not span `total` hashes");
            for (uint32_t g : groups)
                if (g >= n_groups) throw err_internal(std::string(me) + ": a group number outside 0 .. n_groups - 1");
        }
        SetopsMergeArgs a{d_hashes, d_offsets, n, total, d_groups, n_groups, d_need, need_all, max_hash, num, d_out_hashes, d_out_offsets, d_result,
                          d_workspace, workspace_bytes};
        a.values = values; a.d_abunds = d_abunds; a.d_out_abunds = d_out_abunds;
        uint64_t out_total = 0;
        hip_check(setops_merge_run(a, &out_total, st), "setops_merge");
        ret = out_total;
    });
    return ret;
}

uint64_t smgpu_setops_filter_workspace_bytes(uint64_t n, uint64_t total, uint64_t other_len) { return setops_filter_workspace_bytes(n, total, other_len); }

uint64_t smgpu_setops_filter_raw(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n, uint64_t total, const uint64_t* d_other_hashes,
                                 const uint64_t* d_other_offsets, uint64_t other_len, uint32_t keep_present, uint32_t grid, uint64_t* d_out_hashes,
                                 uint64_t capacity, uint64_t* d_out_offsets, uint64_t* d_result, void* d_workspace, uint64_t workspace_bytes,
                                 void* stream) {
    return smgpu_setops_filter_values_raw(d_hashes, nullptr, d_offsets, n, total, d_other_hashes, nullptr, d_other_offsets, other_len, keep_present,
                                          SETOPS_VALUES_NONE, 0, ~0ull, grid, d_out_hashes, nullptr, capacity, d_out_offsets, d_result, d_workspace,
                                          workspace_bytes, stream);
}

uint64_t smgpu_setops_filter_values_raw(const uint64_t* d_hashes, const uint64_t* d_abunds, const uint64_t* d_offsets, uint64_t n, uint64_t total,
                                        const uint64_t* d_other_hashes, const uint64_t* d_other_abunds, const uint64_t* d_other_offsets,
                                        uint64_t other_len, uint32_t keep_present, uint32_t values, uint64_t range_lo, uint64_t range_hi, uint32_t grid,
                                        uint64_t* d_out_hashes, uint64_t* d_out_abunds, uint64_t capacity, uint64_t* d_out_offsets, uint64_t* d_result,
                                        void* d_workspace, uint64_t workspace_bytes, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        const char* me = values ? "smgpu_setops_filter_values_raw" : "smgpu_setops_filter_raw";
        if (values > SETOPS_VALUES_RANGE) throw err_internal(std::string(me) + ": values is 0 (flat), 1 (carry), 2 (take) or 3 (range)");
        if ((values == SETOPS_VALUES_CARRY || values == SETOPS_VALUES_RANGE) && total) check_raw(d_abunds, me, "d_abunds");
        if (values && capacity) check_raw(d_out_abunds, me, "d_out_abunds");
        if (values == SETOPS_VALUES_TAKE) {
            if (!keep_present) throw err_internal(std::string(me) + ": take keeps the hashes the other sketch holds (keep_present = 1)");
            if (d_other_offsets || other_len) check_raw(d_other_abunds, me, "d_other_abunds");
        }
        if (values == SETOPS_VALUES_RANGE) {                         // no other sketch: an empty one stands in, and nothing is looked up
            if (d_other_offsets || other_len) throw err_internal(std::string(me) + ": the range filter takes no other sketch");
        }
        check_raw(d_result, me, "d_result");
        check_raw(d_workspace, me, "d_workspace");
        check_raw(d_out_offsets, me, "d_out_offsets");
        if (n) check_raw(d_offsets, me, "d_offsets");
        if (total) check_raw(d_hashes, me, "d_hashes");
        if (capacity) check_raw(d_out_hashes, me, "d_out_hashes");
        if (!d_other_offsets && other_len) check_raw(d_other_hashes, me, "d_other_hashes");
        if (n >= 0xffffffffull) throw err_internal(std::string(me) + ": 2^32 rows are not taken");
        if (!d_other_offsets && other_len > SETOPS_OTHER_MAX_HASHES) throw err_internal(std::string(me) + ": another sketch of 2^32 hashes is not taken");
        if (grid > (1u << 20)) throw err_internal(std::string(me) + ": grid above 1048576 workgroups");
        if (workspace_bytes < setops_filter_workspace_bytes(n, total, d_other_offsets ? 0 : other_len))
            throw err_internal(std::string(me) + ": the workspace is smaller than smgpu_setops_filter_workspace_bytes says");
        (void)DeviceCtx::get();
        hipStream_t st = (hipStream_t)stream;
        if (n) {
            uint64_t ends[2] = {0, 0};
            hip_check(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipMemcpyAsync(&ends[1], d_offsets + n, 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
            if (ends[1] < ends[0] || ends[1] - ends[0] != total) throw err_internal(std::string(me) + ": the offsets do not span `total` hashes");
        }
        SetopsFilterArgs a{d_hashes, d_offsets, n, total, d_other_hashes, d_other_offsets, other_len, keep_present, grid, d_out_offsets, d_result,
                           d_workspace, workspace_bytes};
        a.values = values; a.d_abunds = d_abunds; a.d_other_abunds = d_other_abunds; a.range_lo = range_lo; a.range_hi = range_hi;
        SetopsFilterState state;
        uint64_t out_total = 0;
        hip_check(setops_filter_count(a, state, &out_total, st), "setops_filter (count)");
        ret = out_total;
        if (out_total > capacity) return;                            // the caller runs again with room
        uint32_t trouble = 0;
        hip_check(setops_filter_write(a, state, d_out_hashes, capacity, &trouble, st, d_out_abunds), "setops_filter (write)");
        if (trouble) {
            ret = ~0ull;
            throw err_internal(std::string(me) + ": the write kept another number of hashes than the count");
        }
    });
    return ret;
}

SmgpuSketchSet* smgpu_sketchset_merge_groups(const SmgpuSketchSet* p, const uint32_t* groups, uint64_t n_groups, const uint32_t* need, uint32_t need_all,
                                             const char* const* names) {
    return smgpu_sketchset_merge_groups_values(p, groups, n_groups, need, need_all, names, 0);
}

SmgpuSketchSet* smgpu_sketchset_merge_groups_values(const SmgpuSketchSet* p, const uint32_t* groups, uint64_t n_groups, const uint32_t* need,
                                                    uint32_t need_all, const char* const* names, uint32_t count_rows) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (!s) throw err_internal("smgpu_sketchset_merge_groups: null pointer");
        if (count_rows && s->has_abunds())
            throw err_internal("count_rows counts the rows of a flat set: this set carries abundance, and its merge sums them (flatten() first)");
        const uint32_t values = count_rows ? SETOPS_MERGE_COUNT : s->has_abunds() ? SETOPS_MERGE_SUM : SETOPS_MERGE_FLAT;
        if (s->n) need_params(*s);
        if (s->n && n_groups == 0) throw err_internal("smgpu_sketchset_merge_groups: rows without a group");
        if (n_groups > 0xfffffffeull || s->total > SETOPS_MERGE_MAX_HASHES) throw err_internal("smgpu_sketchset_merge_groups: 2^32 hashes or groups are not taken");
        for (uint64_t r = 0; groups && r < s->n; ++r)
            if (groups[r] >= n_groups) throw err_internal("smgpu_sketchset_merge_groups: a group number outside 0 .. n_groups - 1");
        if (s->num && (need_all || need))
            throw Error(E_MISMATCH_NUM, "a num set merges to the union of its rows only: the count a hash needs cannot be chosen");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::unique_ptr<SketchSet> out = sketchset_like(*s, n_groups);
        out->offsets.reserve((n_groups + 1) * 8, st);
        const uint64_t ws_bytes = values ? setops_merge_values_workspace_bytes(s->total, n_groups) : setops_merge_workspace_bytes(s->total, n_groups);
        AsyncBuf ws((size_t)ws_bytes, st), d_result(64, st), d_groups((s->n + 1) * 4, st), d_need((n_groups + 1) * 4, st), d_tmp((s->total + 2) * 8, st);
        AsyncBuf d_tmp_abunds(values ? (s->total + 2) * 8 : 8, st);
        if (groups && s->n) hip_check(hipMemcpyAsync(d_groups.p, groups, s->n * 4, hipMemcpyHostToDevice, st), "H2D");
        if (need && n_groups) hip_check(hipMemcpyAsync(d_need.p, need, n_groups * 4, hipMemcpyHostToDevice, st), "H2D");
        SetopsMergeArgs a{s->hashes.as<uint64_t>(), s->offsets.as<uint64_t>(), s->n, s->total, groups ? d_groups.as<uint32_t>() : nullptr, n_groups,
                          need ? d_need.as<uint32_t>() : nullptr, need_all, s->max_hash, s->num, d_tmp.as<uint64_t>(), out->offsets.as<uint64_t>(),
                          d_result.as<uint64_t>(), ws.p, ws_bytes};
        a.values = values; a.d_abunds = s->abunds.as<uint64_t>(); a.d_out_abunds = values ? d_tmp_abunds.as<uint64_t>() : nullptr;
        uint64_t total = 0;
        hip_check(setops_merge_run(a, &total, st), "setops_merge");
        out->hashes.reserve(total * 8 + 16, st);
        if (total) hip_check(hipMemcpyAsync(out->hashes.p, d_tmp.p, total * 8, hipMemcpyDeviceToDevice, st), "D2D");
        if (values) {
            out->abunds.reserve(total * 8 + 16, st);
            if (total) hip_check(hipMemcpyAsync(out->abunds.p, d_tmp_abunds.p, total * 8, hipMemcpyDeviceToDevice, st), "D2D");
            // (a sum is not bounded by its addends' bound: the wide angular form; a count is at most the set's rows)
            out->abund_max = count_rows ? s->n : ~0ull;
        }
        sketchset_fetch_offsets(*out, st);
        if (out->total != total) throw err_internal("the merge's offsets do not end at its total");
        sketchset_finish_rows(*out, nullptr);
        for (uint64_t gi = 0; names && gi < n_groups; ++gi)
            if (names[gi]) out->rows[gi].name = names[gi];
        return reinterpret_cast<SmgpuSketchSet*>(out.release());
    });
}

SmgpuSketchSet* smgpu_sketchset_filter(const SmgpuSketchSet* p, const SmgpuSketchSet* other_p, uint32_t keep_present) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        const SketchSet* o = reinterpret_cast<const SketchSet*>(other_p);
        if (!s || !o) throw err_internal("smgpu_sketchset_filter: null pointer");
        need_params(*s);
        need_params(*o);
        check_filter_compatible(*s, o->ksize * (o->hash_function == HF_DNA ? 1u : 3u), o->hash_function, o->max_hash, o->seed);
        if (o->n != 1 && o->n != s->n) throw err_internal("smgpu_sketchset_filter: the other set has one row, or as many as this one");
        if (o->n == 1 && o->total > SETOPS_OTHER_MAX_HASHES) throw err_internal("smgpu_sketchset_filter: another sketch of 2^32 hashes is not taken");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        if (o->n == 1) return reinterpret_cast<SmgpuSketchSet*>(filter_set(*s, o->hashes.as<uint64_t>(), nullptr, o->total, keep_present, st));
        return reinterpret_cast<SmgpuSketchSet*>(filter_set(*s, o->hashes.as<uint64_t>(), o->offsets.as<uint64_t>(), 0, keep_present, st));
    });
}

SmgpuSketchSet* smgpu_sketchset_filter_sketch(const SmgpuSketchSet* p, const SourmashKmerMinHash* mh_p, uint32_t keep_present) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        const KmerMinHash* mh = MH(mh_p);                            // (queued records are hashed before the context is taken)
        if (!s || !mh) throw err_internal("smgpu_sketchset_filter_sketch: null pointer");
        need_params(*s);
        check_filter_compatible(*s, mh->ksize, mh->hash_function, mh->max_hash, mh->seed);
        const uint64_t nq = mh->size();
        if (nq > SETOPS_OTHER_MAX_HASHES) throw err_internal("smgpu_sketchset_filter_sketch: a sketch of 2^32 hashes is not taken");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        AsyncBuf dq(nq * 8 + 16, st);
        if (nq) hip_check(hipMemcpyAsync(dq.p, mh->mins.data(), nq * 8, hipMemcpyHostToDevice, st), "H2D");
        return reinterpret_cast<SmgpuSketchSet*>(filter_set(*s, dq.as<uint64_t>(), nullptr, nq, keep_present, st));
    });
}

SmgpuSketchSet* smgpu_sketchset_downsample(const SmgpuSketchSet* p, uint64_t max_hash) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (!s) throw err_internal("smgpu_sketchset_downsample: null pointer");
        need_params(*s);
        if (s->num || s->max_hash == 0 || max_hash == 0) throw Error(E_MISMATCH_NUM, "cannot downsample a num MinHash using scaled");
        if (max_hash > s->max_hash) throw err_cannot_upsample();
        if (s->n >= 0xffffffffull) throw err_internal("smgpu_sketchset_downsample: 2^32 rows are not taken");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::unique_ptr<SketchSet> out = sketchset_like(*s, s->n);
        out->max_hash = max_hash;
        // every row ends where its hashes pass max_hash (rows ascend): sizes at the cutoff, their prefix sums, one prefix gather
        std::vector<uint64_t> sizes(s->n + 1, 0);
        AsyncBuf d_sizes((s->n + 1) * 8, st);
        if (s->n) {
            hip_check(many_sizes_launch(s->hashes.as<uint64_t>(), s->offsets.as<uint64_t>(), s->n, max_hash, d_sizes.as<uint64_t>(), st), "many_sizes");
            hip_check(hipMemcpyAsync(sizes.data(), d_sizes.p, s->n * 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
        }
        out->host_offsets.assign(s->n + 1, 0);
        for (uint64_t r = 0; r < s->n; ++r) out->host_offsets[r + 1] = out->host_offsets[r] + sizes[r];
        out->total = out->host_offsets[s->n];
        out->hashes.reserve(out->total * 8 + 16, st);
        out->offsets.reserve((s->n + 1) * 8, st);
        hip_check(hipMemcpyAsync(out->offsets.p, out->host_offsets.data(), (s->n + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(csr_prefix_gather_launch(s->hashes.as<uint64_t>(), s->offsets.as<uint64_t>(), out->offsets.as<uint64_t>(), (uint32_t)s->n,
                                           out->hashes.as<uint64_t>(), st), "csr_prefix_gather");
        if (s->has_abunds()) {                                       // the same prefix of every row, in the other column
            out->abunds.reserve(out->total * 8 + 16, st);
            out->abund_max = s->abund_max;
            hip_check(csr_prefix_gather_launch(s->abunds.as<uint64_t>(), s->offsets.as<uint64_t>(), out->offsets.as<uint64_t>(), (uint32_t)s->n,
                                               out->abunds.as<uint64_t>(), st), "csr_prefix_gather");
        }
        hip_check(hipStreamSynchronize(st), "sync");
        sketchset_finish_rows(*out, s);
        return reinterpret_cast<SmgpuSketchSet*>(out.release());
    });
}

}  // extern "C"
