// capi_common.hpp -- what the units of the extern "C" surface (capi.cpp and the capi_*.cpp families; include/sourmash_amd.h)
// share: the thread's error slot and the landing pad, the handle casts, small output helpers, the three helpers that cross
// units (sigs_out, upload_rows, compare_device_csr) and the device-resident sketch collection.  Internal to the
// library: everything here is hidden, and state lives in inline variables / inline functions so that the library has ONE of each.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/sourmash_amd.h"
#include "collection.hpp"
#include "device_ctx.hpp"
#include "hostxfer.hpp"
#include "record_queue.hpp"
#include "signature_host.hpp"

#pragma GCC visibility push(hidden)
namespace smg {

// ---------------------------------------------------------------------------------------------
// thread-local last error + landing pad (ffi/utils.rs:17-19,58-83,195-207)
// ---------------------------------------------------------------------------------------------
inline thread_local uint32_t g_err_code = 0;
inline thread_local std::string g_err_msg;

inline void set_error(uint32_t code, const std::string& msg) { g_err_code = code; g_err_msg = msg; }

template <class R, class F>
R landing(F&& f) {
    try {
        return f();
    } catch (const Error& e) {
        set_error(e.code, e.what());
    } catch (const std::bad_alloc&) {
        set_error(E_PANIC, "sourmash panicked: out of memory");
    } catch (const std::exception& e) {
        set_error(E_PANIC, std::string("sourmash panicked: ") + e.what());
    } catch (...) {
        set_error(E_PANIC, "sourmash panicked: unknown exception");
    }
    return R{};
}
template <class F>
void landing_void(F&& f) {
    landing<int>([&]() { f(); return 0; });
}

inline SourmashStr make_str(const std::string& s) {
    SourmashStr out;
    out.data = (char*)malloc(s.size() + 1);
    memcpy(out.data, s.data(), s.size());
    out.data[s.size()] = 0;
    out.len = s.size();
    out.owned = true;
    return out;
}

// ---- handles ---------------------------------------------------------------------------------------------------
// hash the records add_sequence queued on the sketch (capi.cpp; record_queue.hpp).  Every accessor goes through MH / SIG,
// which settle first: results are those of immediate hashing, since adding hashes to a sketch commutes (set union, counts add,
// bottom-k keeps the smallest) and everything that does not commute with it settles first.
void settle(KmerMinHash& mh, bool streaming = false);

inline KmerMinHash* RAW(SourmashKmerMinHash* p) { return reinterpret_cast<KmerMinHash*>(p); }
inline const KmerMinHash* RAW(const SourmashKmerMinHash* p) { return reinterpret_cast<const KmerMinHash*>(p); }
inline KmerMinHash* settled(KmerMinHash* m) {
    if (m && !m->pending.empty()) {
        // accessors without a landing pad cannot throw across the C boundary: the failure is left in the thread's error slot
        try { settle(*m); }
        catch (const Error& e) { set_error(e.code, e.what()); }
        catch (const std::exception& e) { set_error(E_PANIC, std::string("sourmash panicked: ") + e.what()); }
    }
    return m;
}
inline KmerMinHash* MH(SourmashKmerMinHash* p) { return settled(reinterpret_cast<KmerMinHash*>(p)); }
inline const KmerMinHash* MH(const SourmashKmerMinHash* p) { return settled(const_cast<KmerMinHash*>(reinterpret_cast<const KmerMinHash*>(p))); }
inline Signature* SIGRAW(SourmashSignature* p) { return reinterpret_cast<Signature*>(p); }
inline Signature* SIG(SourmashSignature* p) {
    Signature* s = reinterpret_cast<Signature*>(p);
    if (s) for (auto& mh : s->sketches) settled(&mh);
    return s;
}
inline const Signature* SIG(const SourmashSignature* p) { return SIG(const_cast<SourmashSignature*>(p)); }
inline ComputeParameters* CP(SourmashComputeParameters* p) { return reinterpret_cast<ComputeParameters*>(p); }
inline const ComputeParameters* CP(const SourmashComputeParameters* p) { return reinterpret_cast<const ComputeParameters*>(p); }

inline uint64_t* slice_out(const std::vector<uint64_t>& v, uintptr_t* size) {
    *size = v.size();
    uint64_t* p = (uint64_t*)malloc((v.size() ? v.size() : 1) * sizeof(uint64_t));
    if (v.size()) memcpy(p, v.data(), v.size() * sizeof(uint64_t));
    return p;
}

inline SourmashSignature** sigs_out(std::vector<Signature>&& sigs, uintptr_t* size) {
    *size = sigs.size();
    SourmashSignature** out = (SourmashSignature**)malloc((sigs.size() ? sigs.size() : 1) * sizeof(void*));
    for (size_t i = 0; i < sigs.size(); ++i) out[i] = reinterpret_cast<SourmashSignature*>(new Signature(std::move(sigs[i])));
    return out;
}

inline std::string upper_ascii(const uint8_t* p, size_t n) {
    std::string s((const char*)p, n);
    for (auto& c : s) if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    return s;
}

inline uint64_t keep_threshold(const KmerMinHash& mh) { return mh.max_hash ? mh.max_hash : ~0ull; }

// ---- helpers of the compare unit (capi_compare.cpp) that the sketch-set unit uses too
// n x n common counts (+ Jaccard) of a device-resident CSR into host matrices
void compare_device_csr(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n, uint64_t total,
                        uint32_t* common_out, double* jaccard_out, hipStream_t st);
// the hash vectors (or abundance vectors) of n sketches back to back into d_dst
void upload_rows(const SourmashKmerMinHash* const* mhs, uintptr_t n, const std::vector<uint64_t>& offsets, bool abunds,
                 void* d_dst, hipStream_t st);

// ---- device-resident sketch collections (capi_sketchset.cpp and capi_records.cpp make them; the gather and Nodegraph units read them)
struct SketchSet {
    DevBuf hashes, offsets;
    uint64_t n = 0, total = 0;
    // filled by smgpu_sketchset_load (empty for sets built from sketch handles)
    std::vector<uint64_t> host_offsets;
    std::vector<ManifestRow> rows;
    uint32_t ksize = 0, hash_function = HF_DNA;
    uint64_t seed = 42, max_hash = 0, num = 0, skipped = 0;
    // (the device blocks are arena blocks and go back to the arena with the DevBufs: no hipFree, which would synchronise the device)
    // An abundance set: u64 abundances aligned with `hashes`, every one >= 1 (MinHash.set_abundances drops zeros); no block: a flat
    // set.  Every reader of hashes / offsets sees an abundance set as its flattened self.  abund_max: the largest stored abundance
    // (it chooses the narrow form of the angular kernels).
    DevBuf abunds;
    uint64_t abund_max = 0;
    bool has_abunds() const { return abunds.p != nullptr; }
};

// ---- abundance sets (capi_abund_set.cpp) and what the set-algebra unit (capi_setops.cpp) shares with them
// an empty set of n rows with the parameters of s
std::unique_ptr<SketchSet> sketchset_like(const SketchSet& s, uint64_t n);
// The manifest rows of a result whose host offsets stand: those of `from` (row for row, when it has them) or fresh ones, with the
// new sizes; with_abundance says whether the result carries the column.
void sketchset_finish_rows(SketchSet& out, const SketchSet* from);
// the device offsets of a result (n + 1 values) to its host side, and its total
void sketchset_fetch_offsets(SketchSet& out, hipStream_t st);
// sig subtract / sig intersect / sig inflate refuse sketches of other parameters: the reference's order (check_compatible)
void check_filter_compatible(const SketchSet& s, uint32_t ksize, uint32_t hash_function, uint64_t max_hash, uint64_t seed);
// The filter of a resident set in any value mode (setops_core.hpp: SetopsValueMode) -> a new set; with a mode that moves values the
// result carries the column.  d_other_offsets null: one sketch d_other_hashes[0, other_len) (TAKE: d_other_abunds beside it);
// otherwise a second CSR row by row.  abund_max: of the other side, for TAKE.
SketchSet* sketchset_filter_values(const SketchSet& s, const uint64_t* d_other_hashes, const uint64_t* d_other_offsets, uint64_t other_len,
                                   uint32_t keep_present, uint32_t values, const uint64_t* d_other_abunds, uint64_t range_lo, uint64_t range_hi,
                                   hipStream_t st, uint64_t abund_max = 0);
// the writers' refusal of an abundance set
void refuse_abundance_writer(const SketchSet& s, const char* entry);

// ---- helpers of the many-queries unit (capi_many.cpp) and the gather unit (capi_gather.cpp) that the gather-many unit uses too
// throws the reference's mismatch error for two sets that cannot meet (many_core.hpp: many_compat_code)
void check_sets_compatible(const SketchSet& db, const SketchSet& q);
// the same for one query sketch against a set
void check_sketch_compatible(const SketchSet& db, const KmerMinHash& mh);
// the hits of the many-queries pass left on the device, ordered by (query, row); ms3: index build, passes, final sort
struct ManyDeviceHits {
    AsyncBuf queries, rows, common;
    uint64_t hits = 0, reruns = 0;
    float ms3[3] = {0.f, 0.f, 0.f};
};
// every row of qs against every row of db at `cutoff`, d_need[q] the count a hit of query q needs; runs again once when the hits
// did not fit the first capacity
void many_hits_on_device(const SketchSet& db, const SketchSet& qs, const uint32_t* d_need, uint64_t cutoff, ManyDeviceHits& out, hipStream_t st);
// One query that is resident on the device (d_query[0, nq), ascending) against a resident set by the one-query path: index build,
// arm, rounds to exhaustion.  -> rounds; idx / isect: the winners' rows and |intersect| in rank order.
uint64_t gather_one_on_device(const uint64_t* d_query, uint64_t nq, const SketchSet& db, uint64_t threshold_hashes, std::vector<uint64_t>& idx,
                              std::vector<uint64_t>& isect, hipStream_t st);

}  // namespace smg
#pragma GCC visibility pop
