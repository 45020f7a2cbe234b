// capi_sketchset.cpp -- the C-ABI (include/sourmash_amd.h): collections of sketches loaded from signature files
// (collection.hpp, sigload.hpp, sigjson.hip), held as one CSR in device memory (SketchSet, capi_common.hpp), and written back as
// .sig / .sig.gz / .zip from the device (sigwrite.hpp, sigwrite.hip).
#include <algorithm>
#include <memory>
#include "capi_common.hpp"
#include "sigload.hpp"
#include "sigwrite.hpp"

using namespace smg;

namespace {

// files -> host CSR (collection.hpp); no device needed
static LoadedCollection load_collection(const char* const* paths, uintptr_t n_paths, uint32_t ksize, const char* moltype,
                                        uint64_t scaled, uint32_t n_threads) {
    LoadSelect sel;
    sel.ksize = ksize;
    sel.hash_function = (moltype && *moltype) ? (int)molecule_from_name(moltype) : -1;
    sel.scaled = scaled;
    CollectionLoader loader(sel, n_threads);
    for (uintptr_t i = 0; i < n_paths; ++i) loader.add_path(paths[i]);
    return loader.run();
}

static SketchSet* upload_collection(LoadedCollection&& col) {
    DeviceCtx& ctx = DeviceCtx::get();
    std::lock_guard<std::recursive_mutex> g(ctx.mutex());
    hipStream_t st = ctx.stream();
    std::unique_ptr<SketchSet> s(new SketchSet());
    s->n = col.rows.size();
    s->total = col.hashes.size();
    s->hashes.reserve(s->total * 8 + 16, st);
    s->offsets.reserve((s->n + 1) * 8, st);
    if (s->total) hip_check(hipMemcpyAsync(s->hashes.p, col.hashes.data(), s->total * 8, hipMemcpyHostToDevice, st), "H2D");
    hip_check(hipMemcpyAsync(s->offsets.p, col.offsets.data(), (s->n + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
    hip_check(hipStreamSynchronize(st), "sync");
    s->host_offsets = std::move(col.offsets);
    s->rows = std::move(col.rows);
    s->ksize = col.ksize; s->hash_function = col.hash_function; s->seed = col.seed;
    s->max_hash = col.max_hash; s->num = col.num; s->skipped = col.skipped;
    return s.release();
}

// ---- signature writer (sigwrite.hpp): a set's rows as .sig / .sig.gz / .zip, written from the device ---------------------------

// a set as the writer's source; `off`: room for the offsets of a set that keeps none on the host
void sw_source_of(const SketchSet* s, std::vector<uint64_t>& off, hipStream_t st, SwSource& src) {
    src.d_hashes = s->hashes.as<uint64_t>();
    src.d_offsets = s->offsets.as<uint64_t>();
    if (s->host_offsets.size() == s->n + 1) src.h_offsets = s->host_offsets.data();
    else {
        off.assign(s->n + 1, 0);
        hip_check(hipMemcpyAsync(off.data(), s->offsets.p, (s->n + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        src.h_offsets = off.data();
    }
    src.n = s->n;
    src.ksize = s->ksize; src.hash_function = s->hash_function; src.seed = s->seed; src.max_hash = s->max_hash; src.num = s->num;
    src.rows = &s->rows;
}

// every row's message length, for the MD5 hand-out
void sw_message_lengths(const SwSource& src, hipStream_t st, std::vector<uint64_t>& msg_len) {
    msg_len.assign(src.n, 0);
    if (src.n == 0) return;
    const uint64_t h0 = src.h_offsets[0], nh = src.h_offsets[src.n] - h0;
    const size_t tmp_bytes = sw_positions_temp_bytes(nh);
    AsyncBuf d_pos((nh + 2) * 8, st), d_tmp(tmp_bytes, st), d_text_len(src.n * 8, st), d_msg_len(src.n * 8, st);
    hip_check(sw_positions_launch(src.d_hashes, h0, nh, d_pos.as<uint64_t>(), d_tmp.p, tmp_bytes, st), "sw_positions");
    hip_check(sw_row_lengths_launch(src.d_offsets, src.n, d_pos.as<uint64_t>(), sw_digit_count(src.json_ksize()), d_text_len.as<uint64_t>(),
                                    d_msg_len.as<uint64_t>(), st), "sw_row_lengths");
    hip_check(hipMemcpyAsync(msg_len.data(), d_msg_len.p, src.n * 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
}

struct SigWriterHandle {
    std::unique_ptr<SigWriter> w;
};

}  // namespace

extern "C" {

SmgpuSketchSet* smgpu_sketchset_new(const SourmashKmerMinHash* const* mhs, uintptr_t n) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        for (uintptr_t i = 0; i < n; ++i) (void)MH(mhs[i]);          // queued records are hashed before the context is taken
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        std::unique_ptr<SketchSet> s(new SketchSet());
        std::vector<uint64_t> off(n + 1, 0);
        for (uintptr_t i = 0; i < n; ++i) off[i + 1] = off[i] + MH(mhs[i])->size();
        s->n = n; s->total = off[n];
        {   // the sketches' shared parameters, if they share them (what a writer needs to know; ksize stays 0 otherwise)
            bool same = n > 0 && !MH(mhs[0])->track_abundance;      // (a set is flat: a set of abundance sketches is not for the writer)
            for (uintptr_t i = 1; i < n && same; ++i) {
                const KmerMinHash *a = MH(mhs[0]), *b = MH(mhs[i]);
                same = !b->track_abundance && a->ksize == b->ksize && a->hash_function == b->hash_function && a->seed == b->seed && a->max_hash == b->max_hash && a->num == b->num;
            }
            if (same) {
                const KmerMinHash* a = MH(mhs[0]);
                s->hash_function = a->hash_function; s->ksize = a->ksize / (a->hash_function == HF_DNA ? 1u : 3u);
                s->seed = a->seed; s->max_hash = a->max_hash; s->num = a->num;
            }
        }
        hipStream_t st = ctx.stream();
        s->hashes.reserve(s->total * 8 + 16, st);
        s->offsets.reserve((n + 1) * 8, st);
        upload_rows(mhs, n, off, false, s->hashes.p, st);               // pinned chunks packed by worker threads, one H2D copy each
        hip_check(hipMemcpyAsync(s->offsets.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipStreamSynchronize(st), "sync");
        return reinterpret_cast<SmgpuSketchSet*>(s.release());
    });
}
void smgpu_sketchset_free(SmgpuSketchSet* p) { delete reinterpret_cast<SketchSet*>(p); }
uintptr_t smgpu_sketchset_len(const SmgpuSketchSet* p) { return reinterpret_cast<const SketchSet*>(p)->n; }

SmgpuCollection* smgpu_collection_load(const char* const* paths, uintptr_t n_paths, uint32_t ksize, const char* moltype,
                                       uint64_t scaled, uint32_t n_threads) {
    return landing<SmgpuCollection*>([&]() -> SmgpuCollection* {
        return reinterpret_cast<SmgpuCollection*>(new LoadedCollection(load_collection(paths, n_paths, ksize, moltype, scaled, n_threads)));
    });
}
void smgpu_collection_free(SmgpuCollection* p) { delete reinterpret_cast<LoadedCollection*>(p); }
uintptr_t smgpu_collection_len(const SmgpuCollection* p) { return reinterpret_cast<const LoadedCollection*>(p)->rows.size(); }
uint64_t smgpu_collection_total_hashes(const SmgpuCollection* p) { return reinterpret_cast<const LoadedCollection*>(p)->hashes.size(); }
uint64_t smgpu_collection_skipped(const SmgpuCollection* p) { return reinterpret_cast<const LoadedCollection*>(p)->skipped; }
const uint64_t* smgpu_collection_hashes(const SmgpuCollection* p) { return reinterpret_cast<const LoadedCollection*>(p)->hashes.data(); }
const uint64_t* smgpu_collection_offsets(const SmgpuCollection* p) { return reinterpret_cast<const LoadedCollection*>(p)->offsets.data(); }
SourmashStr smgpu_collection_manifest(const SmgpuCollection* p) {
    return landing<SourmashStr>([&]() -> SourmashStr {
        return make_str(manifest_to_csv(reinterpret_cast<const LoadedCollection*>(p)->rows));
    });
}
void smgpu_collection_params(const SmgpuCollection* p, uint32_t* ksize, uint32_t* hash_function, uint64_t* seed,
                             uint64_t* max_hash, uint64_t* num) {
    const LoadedCollection* c = reinterpret_cast<const LoadedCollection*>(p);
    *ksize = c->ksize; *hash_function = c->hash_function; *seed = c->seed; *max_hash = c->max_hash; *num = c->num;
}

// files -> CSR in HBM, no per-sketch objects
SmgpuSketchSet* smgpu_sketchset_load(const char* const* paths, uintptr_t n_paths, uint32_t ksize, const char* moltype,
                                     uint64_t scaled, uint32_t n_threads) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        DeviceCtx& ctx = DeviceCtx::get();                          // fail before parsing when there is no GPU
        static const bool host_only = [] { const char* e = getenv("SMG_SIGLOAD_DEVICE"); return e && e[0] == '0'; }();
        if (host_only)
            return reinterpret_cast<SmgpuSketchSet*>(upload_collection(load_collection(paths, n_paths, ksize, moltype, scaled, n_threads)));
        // inflate + number parsing on the device, the CSR never leaves HBM (sigload.hpp); what the device does not take is
        // parsed by the host path document by document
        LoadSelect sel;
        sel.ksize = ksize;
        sel.hash_function = (moltype && *moltype) ? (int)molecule_from_name(moltype) : -1;
        sel.scaled = scaled;
        CollectionLoader loader(sel, n_threads);
        for (uintptr_t i = 0; i < n_paths; ++i) loader.add_path(paths[i]);
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        CollectionLoader::DeviceResult res;
        loader.run_device(st, res);
        std::unique_ptr<SketchSet> s(new SketchSet());
        s->hashes.p = res.d_hashes;
        s->hashes.cap = (size_t)res.total * 8 + 16;
        s->hashes.st = st;
        s->n = res.rows.size();
        s->total = res.total;
        s->offsets.reserve((s->n + 1) * 8, st);
        hip_check(hipMemcpyAsync(s->offsets.p, res.offsets.data(), (s->n + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipStreamSynchronize(st), "sync");
        s->host_offsets = std::move(res.offsets);
        s->rows = std::move(res.rows);
        s->ksize = res.ksize; s->hash_function = res.hash_function; s->seed = res.seed;
        s->max_hash = res.max_hash; s->num = res.num; s->skipped = res.skipped;
        sigload_counters().on_device += res.on_device;
        sigload_counters().on_host += res.on_host;
        return reinterpret_cast<SmgpuSketchSet*>(s.release());
    });
}
SmgpuSketchSet* smgpu_sketchset_from_collection(const SmgpuCollection* p) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        LoadedCollection copy = *reinterpret_cast<const LoadedCollection*>(p);
        return reinterpret_cast<SmgpuSketchSet*>(upload_collection(std::move(copy)));
    });
}
// rows[0..n) of a loaded set as a new set (device-to-device row gather; manifest rows follow)
SmgpuSketchSet* smgpu_sketchset_subset(const SmgpuSketchSet* p, const uint64_t* rows, uintptr_t n) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (s->host_offsets.size() != s->n + 1) throw err_internal("smgpu_sketchset_subset needs a set made by smgpu_sketchset_load");
        std::unique_ptr<SketchSet> out(new SketchSet());
        out->n = n;
        out->ksize = s->ksize; out->hash_function = s->hash_function; out->seed = s->seed;
        out->max_hash = s->max_hash; out->num = s->num;
        out->host_offsets.assign(n + 1, 0);
        out->rows.reserve(n);
        for (uintptr_t i = 0; i < n; ++i) {
            if (rows[i] >= s->n) throw err_internal("sketch index out of range");
            out->host_offsets[i + 1] = out->host_offsets[i] + (s->host_offsets[rows[i] + 1] - s->host_offsets[rows[i]]);
            if (rows[i] < s->rows.size()) out->rows.push_back(s->rows[rows[i]]);
        }
        out->total = out->host_offsets[n];
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        out->hashes.reserve((out->total + 1) * 8, st);
        out->offsets.reserve((n + 1) * 8, st);
        DevBuf d_rows;                                              // (an arena block: released on the stream, no device-wide synchronisation)
        d_rows.reserve((n + 1) * 8, st);
        hip_check(hipMemcpyAsync(out->offsets.p, out->host_offsets.data(), (n + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
        if (n) hip_check(hipMemcpyAsync(d_rows.p, rows, n * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(copy_rows_launch(s->hashes.as<uint64_t>(), s->offsets.as<uint64_t>(), d_rows.as<uint64_t>(), n,
                                   out->offsets.as<uint64_t>(), out->hashes.as<uint64_t>(), st), "copy_rows");
        if (s->has_abunds()) {                                      // the same row gather, in the other column
            out->abunds.reserve((out->total + 1) * 8, st);
            out->abund_max = s->abund_max;
            hip_check(copy_rows_launch(s->abunds.as<uint64_t>(), s->offsets.as<uint64_t>(), d_rows.as<uint64_t>(), n,
                                       out->offsets.as<uint64_t>(), out->abunds.as<uint64_t>(), st), "copy_rows");
        }
        hip_check(hipStreamSynchronize(st), "sync");
        return reinterpret_cast<SmgpuSketchSet*>(out.release());
    });
}
uint64_t smgpu_sketchset_total_hashes(const SmgpuSketchSet* p) { return reinterpret_cast<const SketchSet*>(p)->total; }
uint64_t smgpu_sketchset_skipped(const SmgpuSketchSet* p) { return reinterpret_cast<const SketchSet*>(p)->skipped; }
SourmashStr smgpu_sketchset_manifest(const SmgpuSketchSet* p) {
    return landing<SourmashStr>([&]() -> SourmashStr {
        return make_str(manifest_to_csv(reinterpret_cast<const SketchSet*>(p)->rows));
    });
}
void smgpu_sketchset_params(const SmgpuSketchSet* p, uint32_t* ksize, uint32_t* hash_function, uint64_t* seed,
                            uint64_t* max_hash, uint64_t* num) {
    const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
    *ksize = s->ksize; *hash_function = s->hash_function; *seed = s->seed; *max_hash = s->max_hash; *num = s->num;
}
void smgpu_sketchset_sizes(const SmgpuSketchSet* p, uint64_t* out) {
    landing_void([&] {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (s->host_offsets.size() == s->n + 1) {
            for (uint64_t i = 0; i < s->n; ++i) out[i] = s->host_offsets[i + 1] - s->host_offsets[i];
            return;
        }
        std::vector<uint64_t> off(s->n + 1);
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hip_check(hipMemcpyAsync(off.data(), s->offsets.p, (s->n + 1) * 8, hipMemcpyDeviceToHost, ctx.stream()), "D2H");
        hip_check(hipStreamSynchronize(ctx.stream()), "sync");
        for (uint64_t i = 0; i < s->n; ++i) out[i] = off[i + 1] - off[i];
    });
}
// the sketch of row `index` as a new handle (for result rows that need a full object)
SourmashKmerMinHash* smgpu_sketchset_get(const SmgpuSketchSet* p, uint64_t index) {
    return landing<SourmashKmerMinHash*>([&]() -> SourmashKmerMinHash* {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (index >= s->n) throw err_internal("sketch index out of range");
        if (s->host_offsets.size() != s->n + 1) throw err_internal("smgpu_sketchset_get needs a set made by smgpu_sketchset_load");
        const uint64_t lo = s->host_offsets[index], len = s->host_offsets[index + 1] - lo;
        std::unique_ptr<KmerMinHash> mh(new KmerMinHash(0, s->ksize * (s->hash_function == HF_DNA ? 1 : 3), s->hash_function,
                                                        s->seed, s->has_abunds(), (uint32_t)s->num));
        mh->max_hash = s->max_hash;
        mh->mins.resize(len);
        if (s->has_abunds()) mh->abunds.resize(len);                // (an abundance set gives abundance sketches)
        mh->touch();
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        if (len) hip_check(hipMemcpyAsync(mh->mins.data(), s->hashes.as<uint64_t>() + lo, len * 8, hipMemcpyDeviceToHost, ctx.stream()), "D2H");
        if (len && s->has_abunds())
            hip_check(hipMemcpyAsync(mh->abunds.data(), s->abunds.as<uint64_t>() + lo, len * 8, hipMemcpyDeviceToHost, ctx.stream()), "D2H");
        hip_check(hipStreamSynchronize(ctx.stream()), "sync");
        return reinterpret_cast<SourmashKmerMinHash*>(mh.release());
    });
}
void smgpu_sketchset_device_csr(const SmgpuSketchSet* p, const uint64_t** d_hashes, const uint64_t** d_offsets) {
    const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
    *d_hashes = s->hashes.as<uint64_t>();
    *d_offsets = s->offsets.as<uint64_t>();
}
// |query ∩ row| for every row: one streaming pass, no gather index (search / prefetch over a loaded collection)
void smgpu_sketchset_overlaps(const SmgpuSketchSet* p, const SourmashKmerMinHash* query, uint64_t* out) {
    landing_void([&] {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (s->n == 0) return;
        const uint64_t nq = MH(query)->size();
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        AsyncBuf dq(nq * 8 + 16, st), dc(s->n * 8 + 16, st);
        if (nq) hip_check(hipMemcpyAsync(dq.p, MH(query)->mins.data(), nq * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipMemsetAsync(dc.p, 0, s->n * 8, st), "memset");
        hip_check(overlap_vector_launch(dq.as<uint64_t>(), nq, s->hashes.as<uint64_t>(), s->offsets.as<uint64_t>(), s->n,
                                        dc.as<unsigned long long>(), 0, st), "overlap");
        hip_check(hipMemcpyAsync(out, dc.p, s->n * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
    });
}
void smgpu_sketchset_compare(const SmgpuSketchSet* p, uint32_t* common_out, double* jaccard_out) {
    landing_void([&] {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (s->n == 0) return;
        if (s->num != 0) throw err_internal("smgpu_sketchset_compare handles scaled sketches");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        compare_device_csr(s->hashes.as<uint64_t>(), s->offsets.as<uint64_t>(), s->n, s->total, common_out, jaccard_out, ctx.stream());
    });
}

uint64_t smgpu_sigjson_text_pad(void) { return SJ_TEXT_PAD; }

void smgpu_sigjson_parse_raw(const uint8_t* d_text, uint64_t text_len, const uint64_t* docs, uint32_t n_docs, uint64_t keep_max, void* spans_out,
                             uint32_t* flags_out, uint64_t* d_values, uint64_t value_capacity, void* parsed_out, uint64_t parsed_capacity,
                             uint64_t* counts_out, void* stream) {
    landing_void([&] {
        if (!counts_out) throw err_internal("smgpu_sigjson_parse_raw: null pointer");
        counts_out[0] = counts_out[1] = 0;
        if (n_docs == 0) return;
        if (!d_text || !docs || !spans_out || !flags_out || !d_values || !parsed_out) throw err_internal("smgpu_sigjson_parse_raw: null pointer");
        std::vector<SjDoc> dv(n_docs);
        for (uint32_t d = 0; d < n_docs; ++d) {
            dv[d] = SjDoc{docs[2 * d], docs[2 * d + 1]};
            if (dv[d].off > text_len || dv[d].len > text_len - dv[d].off) throw err_internal("smgpu_sigjson_parse_raw: document " + std::to_string(d) + " reaches outside the text");
        }
        hipStream_t st = (hipStream_t)stream;
        AsyncBuf d_docs(dv.size() * sizeof(SjDoc), st), d_spans(dv.size() * SJ_MAX_SPANS * sizeof(SjSpan), st), d_flags(dv.size() * 4, st);
        hip_check(hipMemcpyAsync(d_docs.p, dv.data(), dv.size() * sizeof(SjDoc), hipMemcpyHostToDevice, st), "H2D");
        hip_check(sj_spans_launch(d_text, d_docs.as<SjDoc>(), n_docs, d_spans.as<SjSpan>(), d_flags.as<uint32_t>(), st), "sj_spans");
        std::vector<SjSpan> spans(dv.size() * SJ_MAX_SPANS);
        hip_check(hipMemcpyAsync(spans.data(), d_spans.p, spans.size() * sizeof(SjSpan), hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipMemcpyAsync(flags_out, d_flags.p, dv.size() * 4, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        SjSpan* so = static_cast<SjSpan*>(spans_out);                  // (the records a document does not have stay the caller's)
        for (size_t d = 0; d < dv.size(); ++d)
            for (uint32_t s = 0; s < (flags_out[d] & 0xffu) && s < SJ_MAX_SPANS; ++s) so[d * SJ_MAX_SPANS + s] = spans[d * SJ_MAX_SPANS + s];
        SjPlan planned;
        sj_plan(dv, spans.data(), flags_out, planned);
        counts_out[0] = planned.jobs.size(); counts_out[1] = planned.n_values;
        if (planned.jobs.size() > parsed_capacity || planned.n_values > value_capacity || planned.jobs.size() > 0x7fffffffull)
            throw err_internal("smgpu_sigjson_parse_raw: " + std::to_string(planned.jobs.size()) + " jobs with " + std::to_string(planned.n_values) +
                               " values do not fit the capacities");
        if (planned.jobs.empty()) return;
        AsyncBuf d_jobs(planned.jobs.size() * sizeof(SjParse), st), d_parsed(planned.jobs.size() * sizeof(SjParsed), st);
        hip_check(hipMemcpyAsync(d_jobs.p, planned.jobs.data(), planned.jobs.size() * sizeof(SjParse), hipMemcpyHostToDevice, st), "H2D");
        hip_check(sj_parse_launch(d_text, d_jobs.as<SjParse>(), (uint32_t)planned.jobs.size(), d_values, d_parsed.as<SjParsed>(), keep_max, st), "sj_parse");
        hip_check(hipMemcpyAsync(parsed_out, d_parsed.p, planned.jobs.size() * sizeof(SjParsed), hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
    });
}

// A set from a CSR the caller holds in HBM (torch tensors): n flat sketches of shared parameters, row r = d_hashes[d_offsets[r] ..
// d_offsets[r + 1]) ascending.  The rows are copied (device to device) on the library's stream; names / filenames: NULL or one C
// string per row for the manifest.  ksize: in residues of the molecule (amino acids for protein sketches).
SmgpuSketchSet* smgpu_sketchset_from_csr(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n, uint32_t ksize, uint32_t hash_function,
                                         uint64_t seed, uint64_t max_hash, uint64_t num, const char* const* names, const char* const* filenames) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        if (!d_offsets || ksize == 0) throw err_internal("smgpu_sketchset_from_csr: offsets and a ksize are needed");
        if (hash_function < HF_DNA || hash_function > HF_HP) throw err_internal("smgpu_sketchset_from_csr: unknown hash function");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::unique_ptr<SketchSet> s(new SketchSet());
        s->host_offsets.assign(n + 1, 0);
        hip_check(hipMemcpyAsync(s->host_offsets.data(), d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        const uint64_t base = s->host_offsets[0];
        for (uint64_t r = 0; r < n; ++r)
            if (s->host_offsets[r + 1] < s->host_offsets[r]) throw err_internal("smgpu_sketchset_from_csr: offsets must ascend");
        for (uint64_t r = 0; r <= n; ++r) s->host_offsets[r] -= base;
        s->n = n; s->total = s->host_offsets[n];
        if (s->total && !d_hashes) throw err_internal("smgpu_sketchset_from_csr: null pointer");
        s->ksize = ksize; s->hash_function = hash_function; s->seed = seed; s->max_hash = max_hash; s->num = num;
        s->hashes.reserve(s->total * 8 + 16, st);
        s->offsets.reserve((n + 1) * 8, st);
        if (s->total) hip_check(hipMemcpyAsync(s->hashes.p, d_hashes + base, s->total * 8, hipMemcpyDeviceToDevice, st), "D2D");
        hip_check(hipMemcpyAsync(s->offsets.p, s->host_offsets.data(), (n + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipStreamSynchronize(st), "sync");
        s->rows.resize(n);
        for (uint64_t r = 0; r < n; ++r) {
            ManifestRow& m = s->rows[r];
            m.ksize = ksize; m.moltype = molecule_name(hash_function); m.num = num;
            m.scaled = max_hash ? scaled_for_max_hash(max_hash) : 0;
            m.n_hashes = s->host_offsets[r + 1] - s->host_offsets[r];
            if (names && names[r]) m.name = names[r];
            if (filenames && filenames[r]) m.filename = filenames[r];
        }
        return reinterpret_cast<SmgpuSketchSet*>(s.release());
    });
}

// the names and file names of the set's rows (its manifest rows; made here for a set that has none)
void smgpu_sketchset_set_names(SmgpuSketchSet* p, const char* const* names, const char* const* filenames) {
    landing_void([&] {
        SketchSet* s = reinterpret_cast<SketchSet*>(p);
        if (!s) throw err_internal("null pointer");
        if (s->rows.size() != s->n) {
            std::vector<uint64_t> off = s->host_offsets;
            if (off.size() != s->n + 1) {
                off.assign(s->n + 1, 0);
                DeviceCtx& ctx = DeviceCtx::get();
                std::lock_guard<std::recursive_mutex> g(ctx.mutex());
                hip_check(hipMemcpyAsync(off.data(), s->offsets.p, (s->n + 1) * 8, hipMemcpyDeviceToHost, ctx.stream()), "D2H");
                hip_check(hipStreamSynchronize(ctx.stream()), "sync");
            }
            s->rows.assign(s->n, ManifestRow());
            for (uint64_t r = 0; r < s->n; ++r) {
                ManifestRow& m = s->rows[r];
                m.ksize = s->ksize; m.moltype = molecule_name(s->hash_function); m.num = s->num;
                m.scaled = s->max_hash ? scaled_for_max_hash(s->max_hash) : 0;
                m.n_hashes = off[r + 1] - off[r];
            }
        }
        for (uint64_t r = 0; r < s->n; ++r) {
            if (names) s->rows[r].name = names[r] ? names[r] : "";
            if (filenames) s->rows[r].filename = filenames[r] ? filenames[r] : "";
        }
    });
}

// out[16 r .. 16 r + 16): the MD5 of row r (minhash.rs:290-307), computed on the device
void smgpu_sketchset_md5sums(const SmgpuSketchSet* p, uint8_t* out) {
    landing_void([&] {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (s->n == 0) return;
        if (s->ksize == 0) throw err_internal("the set's sketches do not share one set of parameters");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::vector<uint64_t> off;
        SwSource src;
        sw_source_of(s, off, st, src);
        // in runs of rows like the writer's batches (the scan's positions take 8 bytes a hash)
        const std::vector<uint64_t> cut = sw_batches(src);
        for (size_t b = 0; b + 1 < cut.size(); ++b) {
            const uint64_t r0 = cut[b], n = cut[b + 1] - r0;
            if (n == 0) continue;
            SwSource part = src;
            part.d_offsets += r0; part.h_offsets += r0; part.n = n;
            std::vector<uint64_t> msg_len;
            sw_message_lengths(part, st, msg_len);
            AsyncBuf d_md5(n * 16, st);
            sigwrite_stats().md5_host_rows += sw_md5_rows(part.d_hashes, part.d_offsets, part.h_offsets, n, src.json_ksize(), msg_len, SW_MD5_HOST_BOUND,
                                                          d_md5.as<uint8_t>(), st);
            hip_check(hipMemcpyAsync(out + 16 * r0, d_md5.p, n * 16, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
        }
    });
}

// The JSON array of the set's signatures (rows: these rows in this order; NULL: all n rows of the set), the bytes
// signatures_save_buffer gives for the same signatures at compression 0; above 0 the array as one gzip member.
// Freed with nodegraph_buffer_free.
const uint8_t* smgpu_sketchset_to_json(const SmgpuSketchSet* p, const uint64_t* rows, uintptr_t n, uint8_t compression, uintptr_t* size) {
    return landing<const uint8_t*>([&]() -> const uint8_t* {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (!size) throw err_internal("null pointer");
        refuse_abundance_writer(*s, "smgpu_sketchset_to_json");
        if (s->n && s->ksize == 0) throw err_internal("the set's sketches do not share one set of parameters, or track abundance: it cannot be written");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::vector<uint64_t> off;
        SwSource src;
        sw_source_of(s, off, st, src);
        // a selection: its rows gathered into a CSR of their own (device to device), their names beside them
        DevBuf sub_hashes, sub_offsets;
        std::vector<uint64_t> sub_off;
        std::vector<std::string> names, filenames;
        std::vector<const char*> name_ptrs, filename_ptrs;
        if (rows) {
            sub_off.assign(n + 1, 0);
            for (uintptr_t i = 0; i < n; ++i) {
                if (rows[i] >= s->n) throw err_internal("sketch index out of range");
                sub_off[i + 1] = sub_off[i] + (src.h_offsets[rows[i] + 1] - src.h_offsets[rows[i]]);
                names.push_back(src.name(rows[i]));
                filenames.push_back(src.filename(rows[i]));
            }
            for (uintptr_t i = 0; i < n; ++i) { name_ptrs.push_back(names[i].c_str()); filename_ptrs.push_back(filenames[i].c_str()); }
            sub_hashes.reserve((sub_off[n] + 1) * 8, st);
            sub_offsets.reserve((n + 1) * 8, st);
            DevBuf d_rows;
            d_rows.reserve((n + 1) * 8, st);
            hip_check(hipMemcpyAsync(sub_offsets.p, sub_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
            if (n) hip_check(hipMemcpyAsync(d_rows.p, rows, n * 8, hipMemcpyHostToDevice, st), "H2D");
            hip_check(copy_rows_launch(src.d_hashes, src.d_offsets, d_rows.as<uint64_t>(), n, sub_offsets.as<uint64_t>(), sub_hashes.as<uint64_t>(), st),
                      "copy_rows");
            hip_check(hipStreamSynchronize(st), "sync");
            src.d_hashes = sub_hashes.as<uint64_t>(); src.d_offsets = sub_offsets.as<uint64_t>(); src.h_offsets = sub_off.data();
            src.n = n; src.rows = nullptr;
            src.names = name_ptrs.data(); src.filenames = filename_ptrs.data();
        }
        std::string bytes;
        auto sink = [&](const void* q, size_t k) { bytes.append(static_cast<const char*>(q), k); };
        SwGzStream gz;
        gz.compression = compression;
        bool any_rows = false;
        sw_array_add(src, compression ? &gz : nullptr, any_rows, sink, st);
        sw_array_close(compression ? &gz : nullptr, any_rows, sink, st);
        *size = bytes.size();
        uint8_t* out = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
        if (!out) throw err_internal("out of memory");
        memcpy(out, bytes.data(), bytes.size());
        return out;
    });
}

// A signature file written from the device.  The path's suffix chooses the form as the reference does (save_load.py:543-549):
// .zip -- an uncompressed zip of gzip members signatures/<md5>.sig.gz with SOURMASH-MANIFEST.csv last; .gz -- the JSON array as
// one gzip member; anything else -- the JSON array.  compression 0: stored blocks.  The file appears under its name when
// smgpu_sigwriter_close returns without an error, and not at all otherwise.
SmgpuSigWriter* smgpu_sigwriter_new(const char* path, uint8_t compression) {
    return landing<SmgpuSigWriter*>([&]() -> SmgpuSigWriter* {
        if (!path) throw err_internal("null path");
        std::unique_ptr<SigWriterHandle> h(new SigWriterHandle());
        h->w.reset(new SigWriter(path, compression));
        return reinterpret_cast<SmgpuSigWriter*>(h.release());
    });
}
// names / filenames: NULL, or one C string per row of the set (in place of the set's manifest rows)
void smgpu_sigwriter_add(SmgpuSigWriter* w, const SmgpuSketchSet* p, const char* const* names, const char* const* filenames) {
    landing_void([&] {
        SigWriterHandle* h = reinterpret_cast<SigWriterHandle*>(w);
        const SketchSet* s = reinterpret_cast<const SketchSet*>(p);
        if (!h || !h->w || !s) throw err_internal("null pointer");
        refuse_abundance_writer(*s, "smgpu_sigwriter_add");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::vector<uint64_t> off;
        SwSource src;
        sw_source_of(s, off, st, src);
        src.names = names; src.filenames = filenames;
        h->w->add(src, st);
    });
}
void smgpu_sigwriter_close(SmgpuSigWriter* w) {
    landing_void([&] {
        SigWriterHandle* h = reinterpret_cast<SigWriterHandle*>(w);
        if (!h || !h->w) throw err_internal("null pointer");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        h->w->close(ctx.stream());
    });
}
void smgpu_sigwriter_free(SmgpuSigWriter* w) { delete reinterpret_cast<SigWriterHandle*>(w); }

// out[0 .. 7): milliseconds spent in lengths, md5, text, crc, pack, device-to-host copies and file writes since the last reset;
// out[7 .. 12): rows, hashes, bytes of text, bytes written, rows whose MD5 the host computed.  reset != 0: zeroed afterwards.
void smgpu_sigwrite_stats(double* out, int32_t reset) {
    DeviceCtx* ctx = DeviceCtx::peek();                             // (no context: nothing has been written, nobody else is counting)
    std::unique_lock<std::recursive_mutex> g;
    if (ctx) g = std::unique_lock<std::recursive_mutex>(ctx->mutex());
    SwStats& s = sigwrite_stats();
    if (out) {
        const double v[12] = {s.lengths_ms, s.md5_ms, s.text_ms, s.crc_ms, s.pack_ms, s.d2h_ms, s.write_ms,
                              (double)s.rows, (double)s.hashes, (double)s.text_bytes, (double)s.out_bytes, (double)s.md5_host_rows};
        memcpy(out, v, sizeof v);
    }
    if (reset) s = SwStats();
}

// The kernels on caller-owned device buffers (torch tensors).  d_offsets: n_rows + 1 positions in d_hashes.
// MD5 of every row into d_md5 (16 bytes a row); rows whose message is longer than long_row_bound bytes are hashed by the host
// (0: the library's bound).  -> rows the host did.
uint64_t smgpu_sigwrite_md5_raw(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n_rows, uint32_t ksize, uint64_t long_row_bound,
                                uint8_t* d_md5, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        if (n_rows == 0) { ret = 0; return; }
        if (!d_offsets || !d_md5) throw err_internal("smgpu_sigwrite_md5_raw: null pointer");
        DeviceCtx& ctx = DeviceCtx::get();                          // (the pinned ring, the writer's tables and counters are the context's)
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = (hipStream_t)stream;
        std::vector<uint64_t> off(n_rows + 1);
        hip_check(hipMemcpyAsync(off.data(), d_offsets, (n_rows + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        for (uint64_t r = 0; r < n_rows; ++r) if (off[r + 1] < off[r]) throw err_internal("smgpu_sigwrite_md5_raw: offsets must ascend");
        SwSource src;
        src.d_hashes = d_hashes; src.d_offsets = d_offsets; src.h_offsets = off.data(); src.n = n_rows; src.ksize = ksize;
        std::vector<uint64_t> msg_len;
        sw_message_lengths(src, st, msg_len);
        ret = sw_md5_rows(d_hashes, d_offsets, off.data(), n_rows, ksize, msg_len, long_row_bound ? long_row_bound : SW_MD5_HOST_BOUND, d_md5, st);
    });
    return ret;
}

// The documents of the rows into d_text (capacity bytes): per_doc != 0 one `[{...}]` per row, each on a 16-byte line; otherwise
// one array of all rows.  params: ksize (as the JSON says it), hash_function, seed, max_hash, num.  names / filenames: NULL or one
// C string per row.  docs_out: offset and length of every row's document (2 n_rows values).  -> bytes of text (nothing is written
// when they exceed the capacity).
uint64_t smgpu_sigwrite_json_raw(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n_rows, const uint64_t* params, const char* const* names,
                                 const char* const* filenames, int32_t per_doc, uint8_t* d_text, uint64_t capacity, uint64_t* docs_out, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        if (!params || (n_rows && (!d_offsets || !docs_out))) throw err_internal("smgpu_sigwrite_json_raw: null pointer");
        DeviceCtx& ctx = DeviceCtx::get();                          // (the pinned ring, the writer's tables and counters are the context's)
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = (hipStream_t)stream;
        std::vector<uint64_t> off(n_rows + 1, 0);
        if (n_rows) hip_check(hipMemcpyAsync(off.data(), d_offsets, (n_rows + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        for (uint64_t r = 0; r < n_rows; ++r) if (off[r + 1] < off[r]) throw err_internal("smgpu_sigwrite_json_raw: offsets must ascend");
        SwSource src;
        src.d_hashes = d_hashes; src.d_offsets = d_offsets; src.h_offsets = off.data(); src.n = n_rows;
        src.hash_function = (uint32_t)params[1];
        src.ksize = (uint32_t)params[0] / (src.hash_function == HF_DNA ? 1u : 3u);
        src.seed = params[2]; src.max_hash = params[3]; src.num = params[4];
        src.names = names; src.filenames = filenames;
        SwBatch batch;
        sw_build_batch(src, 0, n_rows, per_doc != 0, true, true, SW_MD5_HOST_BOUND, batch, st);
        for (uint64_t r = 0; r < n_rows; ++r) { docs_out[2 * r] = batch.doc_off[r]; docs_out[2 * r + 1] = batch.doc_len[r]; }
        ret = batch.text_bytes;
        if (batch.text_bytes && batch.text_bytes <= capacity) {
            if (!d_text) throw err_internal("smgpu_sigwrite_json_raw: null pointer");
            hip_check(hipMemcpyAsync(d_text, batch.text.p, batch.text_bytes, hipMemcpyDeviceToDevice, st), "D2D");
            hip_check(hipStreamSynchronize(st), "sync");
        }
    });
    return ret;
}

// Every document docs[2 d] .. + docs[2 d + 1] of d_text (offsets: multiples of 16) as a gzip member of its own in d_out: compression
// 0 stored blocks, otherwise one dynamic-Huffman block of literals, packed `chunk` bytes a workgroup (0: the library's chunk).
// members_out: offset and length of every member in d_out.  -> bytes of output (nothing is written when they exceed the capacity).
uint64_t smgpu_deflate_literals_raw(const uint8_t* d_text, uint64_t text_len, const uint64_t* docs, uint32_t n_docs, uint8_t compression, uint32_t chunk,
                                    uint8_t* d_out, uint64_t capacity, uint64_t* members_out, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        if (n_docs == 0) { ret = 0; return; }
        if (!docs || !members_out) throw err_internal("smgpu_deflate_literals_raw: null pointer");
        std::vector<uint64_t> off(n_docs), len(n_docs);
        for (uint32_t d = 0; d < n_docs; ++d) {
            off[d] = docs[2 * d]; len[d] = docs[2 * d + 1];
            if (off[d] > text_len || len[d] > text_len - off[d]) throw err_internal("smgpu_deflate_literals_raw: document " + std::to_string(d) + " reaches outside the text");
            if (off[d] % SW_DOC_ALIGN) throw err_internal("smgpu_deflate_literals_raw: document offsets must be multiples of " + std::to_string(SW_DOC_ALIGN));
            if (len[d] && !d_text) throw err_internal("smgpu_deflate_literals_raw: null pointer");
            if (len[d] && reinterpret_cast<uintptr_t>(d_text) % SW_DOC_ALIGN)      // before anything is launched: the CRC kernel loads 16 bytes a lane
                throw err_internal("smgpu_deflate_literals_raw: d_text must be " + std::to_string(SW_DOC_ALIGN) + "-byte aligned");
        }
        DeviceCtx& ctx = DeviceCtx::get();                          // (the pinned ring, the writer's tables and counters are the context's)
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = (hipStream_t)stream;
        SwPacked packed;
        sw_deflate_docs(d_text, off, len, compression, chunk ? chunk : SW_PACK_CHUNK, packed, st);
        for (uint32_t d = 0; d < n_docs; ++d) { members_out[2 * d] = packed.off[d]; members_out[2 * d + 1] = packed.len[d]; }
        ret = packed.out_bytes;
        if (packed.out_bytes <= capacity) {
            if (!d_out) throw err_internal("smgpu_deflate_literals_raw: null pointer");
            hip_check(hipMemcpyAsync(d_out, packed.out.p, packed.out_bytes, hipMemcpyDeviceToDevice, st), "D2D");
            hip_check(hipStreamSynchronize(st), "sync");
        }
    });
    return ret;
}

}  // extern "C"
