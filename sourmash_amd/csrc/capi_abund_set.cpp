// capi_abund_set.cpp -- the C-ABI (include/sourmash_amd.h): resident collections that carry abundances (capi_common.hpp:
// SketchSet::abunds, a u64 column aligned with the hashes, every value >= 1).  Here a set gets its column (from abundance
// sketches, or from a CSR on the device), gives it back (the flag, the borrowed pointer, the per-row sums), loses it (flatten), and
// meets the value-moving forms of the set algebra (setops.hip): inflate takes another sketch's abundances, filter_abund keeps by a
// range of the set's own.  The angular all-pairs comparison runs on the set's own buffers.
#include <algorithm>
#include <memory>
#include "capi_common.hpp"
#include "setops_core.hpp"

using namespace smg;

namespace {

const SketchSet* SS(const SmgpuSketchSet* p, const char* entry) {
    if (!p) throw err_internal(std::string(entry) + ": null pointer");
    return reinterpret_cast<const SketchSet*>(p);
}

void need_params(const SketchSet& s) {
    if (s.ksize == 0) throw err_internal("the set's sketches do not share one set of parameters");
}

const char* INFLATE_ORDER = "inflate operates on a flat MinHash and takes a MinHash object with track_abundance=True";

// the largest value of a column on the device, with the refusal of a zero: no stored abundance is 0 (MinHash.set_abundances drops
// zeros), so a column that holds one did not come from sketches
uint64_t checked_abund_max(const uint64_t* d_abunds, uint64_t total, const char* entry, hipStream_t st) {
    AsyncBuf d_result(64, st);
    uint64_t result[2] = {0, ~0ull};
    hip_check(abund_check_launch(d_abunds, total, d_result.as<uint64_t>(), st), "abund_check");
    hip_check(hipMemcpyAsync(result, d_result.p, 16, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    if (result[1] != ~0ull)
        throw err_internal(std::string(entry) + ": abundance 0 at position " + std::to_string(result[1]) + " (every stored abundance is at least 1)");
    return result[0];
}

}  // namespace

namespace smg {

void refuse_abundance_writer(const SketchSet& s, const char* entry) {
    if (s.has_abunds())
        throw err_internal(std::string(entry) + ": the set carries abundance and the device writer writes flat sketches: write flatten(), or "
                                                "signature(row) for the rows with their abundance");
}

}  // namespace smg

extern "C" {

SmgpuSketchSet* smgpu_sketchset_new_abund(const SourmashKmerMinHash* const* mhs, uintptr_t n) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        for (uintptr_t i = 0; i < n; ++i) (void)MH(mhs[i]);          // queued records are hashed before the context is taken
        for (uintptr_t i = 0; i < n; ++i)
            if (!MH(mhs[i])->track_abundance) throw err_needs_abundance();
        for (uintptr_t i = 1; i < n; ++i) {
            const KmerMinHash *a = MH(mhs[0]), *b = MH(mhs[i]);
            a->check_compatible(*b);                                 // ksize, molecule, scaled, seed: the reference's errors, in its order
            if (a->num != b->num) throw Error(E_MISMATCH_NUM, "mismatch in num; comparison fail");
        }
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::unique_ptr<SketchSet> s(new SketchSet());
        s->host_offsets.assign(n + 1, 0);
        for (uintptr_t i = 0; i < n; ++i) {
            const KmerMinHash* m = MH(mhs[i]);
            if (m->abunds.size() != m->size()) throw err_internal("smgpu_sketchset_new_abund: a sketch's abundances are not as many as its hashes");
            s->host_offsets[i + 1] = s->host_offsets[i] + m->size();
            for (uint64_t a : m->abunds) {
                if (a == 0) throw err_internal("smgpu_sketchset_new_abund: a sketch holds abundance 0");
                if (a > s->abund_max) s->abund_max = a;
            }
        }
        s->n = n; s->total = s->host_offsets[n];
        if (n) {
            const KmerMinHash* a = MH(mhs[0]);
            s->hash_function = a->hash_function; s->ksize = a->ksize / (a->hash_function == HF_DNA ? 1u : 3u);
            s->seed = a->seed; s->max_hash = a->max_hash; s->num = a->num;
        }
        s->hashes.reserve(s->total * 8 + 16, st);
        s->abunds.reserve(s->total * 8 + 16, st);
        s->offsets.reserve((n + 1) * 8, st);
        upload_rows(mhs, n, s->host_offsets, false, s->hashes.p, st);
        upload_rows(mhs, n, s->host_offsets, true, s->abunds.p, st);
        hip_check(hipMemcpyAsync(s->offsets.p, s->host_offsets.data(), (n + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipStreamSynchronize(st), "sync");
        if (n) sketchset_finish_rows(*s, nullptr);
        return reinterpret_cast<SmgpuSketchSet*>(s.release());
    });
}

SmgpuSketchSet* smgpu_sketchset_from_csr_abund(const uint64_t* d_hashes, const uint64_t* d_abunds, const uint64_t* d_offsets, uint64_t n, uint32_t ksize,
                                               uint32_t hash_function, uint64_t seed, uint64_t max_hash, uint64_t num, const char* const* names,
                                               const char* const* filenames) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        SmgpuSketchSet* made = smgpu_sketchset_from_csr(d_hashes, d_offsets, n, ksize, hash_function, seed, max_hash, num, names, filenames);
        if (!made) return nullptr;                                   // (its error stands in the thread's slot)
        std::unique_ptr<SketchSet> s(reinterpret_cast<SketchSet*>(made));
        if (s->total && !d_abunds) throw err_internal("smgpu_sketchset_from_csr_abund: null pointer (d_abunds)");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        uint64_t base = 0;
        hip_check(hipMemcpyAsync(&base, d_offsets, 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        s->abunds.reserve(s->total * 8 + 16, st);
        if (s->total) hip_check(hipMemcpyAsync(s->abunds.p, d_abunds + base, s->total * 8, hipMemcpyDeviceToDevice, st), "D2D");
        s->abund_max = checked_abund_max(s->abunds.as<uint64_t>(), s->total, "smgpu_sketchset_from_csr_abund", st);
        for (ManifestRow& m : s->rows) m.with_abundance = true;
        return reinterpret_cast<SmgpuSketchSet*>(s.release());
    });
}

uint32_t smgpu_sketchset_track_abundance(const SmgpuSketchSet* p) { return p && reinterpret_cast<const SketchSet*>(p)->has_abunds() ? 1u : 0u; }
uint64_t smgpu_sketchset_abund_max(const SmgpuSketchSet* p) { return p ? reinterpret_cast<const SketchSet*>(p)->abund_max : 0; }

void smgpu_sketchset_device_abunds(const SmgpuSketchSet* p, const uint64_t** d_abunds) {
    landing_void([&] {
        const SketchSet* s = SS(p, "smgpu_sketchset_device_abunds");
        if (!d_abunds) throw err_internal("smgpu_sketchset_device_abunds: null pointer");
        *d_abunds = s->abunds.as<uint64_t>();
    });
}

void smgpu_sketchset_abund_sums(const SmgpuSketchSet* p, uint64_t* out) {
    landing_void([&] {
        const SketchSet* s = SS(p, "smgpu_sketchset_abund_sums");
        if (!s->has_abunds()) throw err_needs_abundance();
        if (s->n == 0) return;
        if (!out) throw err_internal("smgpu_sketchset_abund_sums: null pointer");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        AsyncBuf d_sums(s->n * 8, st);
        hip_check(abund_row_sums_launch(s->abunds.as<uint64_t>(), s->offsets.as<uint64_t>(), s->n, d_sums.as<uint64_t>(), st), "abund_row_sums");
        hip_check(hipMemcpyAsync(out, d_sums.p, s->n * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
    });
}

SmgpuSketchSet* smgpu_sketchset_flatten(const SmgpuSketchSet* p) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        const SketchSet* s = SS(p, "smgpu_sketchset_flatten");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::unique_ptr<SketchSet> out = sketchset_like(*s, s->n);
        out->total = s->total; out->skipped = s->skipped;
        out->hashes.reserve(s->total * 8 + 16, st);
        out->offsets.reserve((s->n + 1) * 8, st);
        if (s->total) hip_check(hipMemcpyAsync(out->hashes.p, s->hashes.p, s->total * 8, hipMemcpyDeviceToDevice, st), "D2D");
        hip_check(hipMemcpyAsync(out->offsets.p, s->offsets.p, (s->n + 1) * 8, hipMemcpyDeviceToDevice, st), "D2D");
        sketchset_fetch_offsets(*out, st);
        if (s->ksize) {                                              // manifest rows: the receiver's, now flat
            sketchset_finish_rows(*out, s);
            if (s->rows.size() == s->n)                             // (the md5 covers the hashes only: it stands)
                for (uint64_t r = 0; r < s->n; ++r) out->rows[r].md5 = s->rows[r].md5;
        }
        return reinterpret_cast<SmgpuSketchSet*>(out.release());
    });
}

SmgpuSketchSet* smgpu_sketchset_inflate(const SmgpuSketchSet* p, const SmgpuSketchSet* other_p) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        const SketchSet* s = SS(p, "smgpu_sketchset_inflate");
        const SketchSet* o = SS(other_p, "smgpu_sketchset_inflate");
        if (s->has_abunds() || !o->has_abunds()) throw err_internal(INFLATE_ORDER);
        need_params(*s);
        need_params(*o);
        check_filter_compatible(*s, o->ksize * (o->hash_function == HF_DNA ? 1u : 3u), o->hash_function, o->max_hash, o->seed);
        if (o->n != 1 && o->n != s->n) throw err_internal("smgpu_sketchset_inflate: the other set has one row, or as many as this one");
        if (o->n == 1 && o->total > SETOPS_OTHER_MAX_HASHES) throw err_internal("smgpu_sketchset_inflate: another sketch of 2^32 hashes is not taken");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        const bool one = o->n == 1;
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_filter_values(*s, o->hashes.as<uint64_t>(), one ? nullptr : o->offsets.as<uint64_t>(),
                                                                         one ? o->total : 0, 1u, SETOPS_VALUES_TAKE, o->abunds.as<uint64_t>(), 0, ~0ull, st,
                                                                         o->abund_max));
    });
}

SmgpuSketchSet* smgpu_sketchset_inflate_sketch(const SmgpuSketchSet* p, const SourmashKmerMinHash* mh_p) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        const SketchSet* s = SS(p, "smgpu_sketchset_inflate_sketch");
        if (!mh_p) throw err_internal("smgpu_sketchset_inflate_sketch: null pointer");
        const KmerMinHash* mh = MH(mh_p);                            // (queued records are hashed before the context is taken)
        if (s->has_abunds() || !mh->track_abundance) throw err_internal(INFLATE_ORDER);
        need_params(*s);
        check_filter_compatible(*s, mh->ksize, mh->hash_function, mh->max_hash, mh->seed);
        const uint64_t nq = mh->size();
        if (nq > SETOPS_OTHER_MAX_HASHES) throw err_internal("smgpu_sketchset_inflate_sketch: a sketch of 2^32 hashes is not taken");
        if (mh->abunds.size() != nq) throw err_internal("smgpu_sketchset_inflate_sketch: the sketch's abundances are not as many as its hashes");
        uint64_t abund_max = 0;
        for (uint64_t a : mh->abunds) abund_max = std::max(abund_max, a);
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        AsyncBuf dq(nq * 8 + 16, st), da(nq * 8 + 16, st);           // the abundance column travels beside the hashes
        if (nq) hip_check(hipMemcpyAsync(dq.p, mh->mins.data(), nq * 8, hipMemcpyHostToDevice, st), "H2D");
        if (nq) hip_check(hipMemcpyAsync(da.p, mh->abunds.data(), nq * 8, hipMemcpyHostToDevice, st), "H2D");
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_filter_values(*s, dq.as<uint64_t>(), nullptr, nq, 1u, SETOPS_VALUES_TAKE, da.as<uint64_t>(), 0, ~0ull,
                                                                         st, abund_max));
    });
}

SmgpuSketchSet* smgpu_sketchset_filter_abund(const SmgpuSketchSet* p, uint64_t min_abundance, uint64_t max_abundance) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        const SketchSet* s = SS(p, "smgpu_sketchset_filter_abund");
        if (!s->has_abunds()) throw err_needs_abundance();
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_filter_values(*s, nullptr, nullptr, 0, 1u, SETOPS_VALUES_RANGE, nullptr, min_abundance, max_abundance,
                                                                         ctx.stream()));
    });
}

void smgpu_sketchset_compare_angular(const SmgpuSketchSet* p, double* sims_out) {
    landing_void([&] {
        const SketchSet* s = SS(p, "smgpu_sketchset_compare_angular");
        if (!s->has_abunds()) throw err_needs_abundance();
        const uint64_t n = s->n;
        if (n == 0) return;
        if (!sims_out) throw err_internal("smgpu_sketchset_compare_angular: null pointer");
        if (n > 0xffffffffull) throw err_internal("too many sketches");
        std::vector<uint64_t> prod((size_t)n * n), sq(n);
        {
            DeviceCtx& ctx = DeviceCtx::get();
            std::lock_guard<std::recursive_mutex> g(ctx.mutex());
            hipStream_t st = ctx.stream();
            AsyncBuf dc((size_t)n * n * 4, st), dp((size_t)n * n * 8, st), ds(n * 8, st);
            hip_check(hipMemsetAsync(dc.p, 0, (size_t)n * n * 4, st), "memset");
            hip_check(hipMemsetAsync(dp.p, 0, (size_t)n * n * 8, st), "memset");
            smgpu_compare_abund_raw_n(s->hashes.as<uint64_t>(), s->abunds.as<uint64_t>(), s->offsets.as<uint64_t>(), (uint32_t)n, s->total,
                                      s->abund_max < (1ull << 32), dc.as<uint32_t>(), dp.as<uint64_t>(), ds.as<uint64_t>(), st);
            if (g_err_code) return;                                  // (the raw entry's error stands)
            HostXfer::get().device_to_host(prod.data(), dp.p, (size_t)n * n * 8, st);
            hip_check(hipMemcpyAsync(sq.data(), ds.p, n * 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
        }
        smgpu_host_angular_f64(prod.data(), sq.data(), n, sims_out, 0);
    });
}

}  // extern "C"
