// capi_compare.cpp -- the C-ABI (include/sourmash_amd.h): all pairs of a collection of sketches (compare.hip, bitindex.hip,
// dictindex.hip, sparse_pairs.hip; compare_ext.hip / abund_pairs.hip for num and abundance sketches) and the host float helpers of the
// compare layer.
#include <algorithm>
#include <cmath>
#include <memory>
#include <thread>
#include "capi_common.hpp"
#include "compare_core.hpp"

using namespace smg;

namespace {

// ---- compare indexes: bit rows over the collection's dictionary, or bit rows for the frequent hashes plus an
//      inverted list of the rare ones (bitindex.hip / sparse_pairs.hip) -----------------------------------------
struct BitIndex {
    uint32_t n = 0, words_per_row = 0;
    uint64_t universe = 0, total = 0;
    uint32_t* bits = nullptr;              // [n][words_per_row]; null when no hash is frequent
    // inverted part (null for the pure bit-row index)
    uint32_t* rows_sorted = nullptr;       // row of every (hash, row) element, ordered by hash
    uint32_t* run_end = nullptr;           // end of the element's run if its hash is rare, else 0
    uint64_t inv_total = 0;                // entries of rows_sorted / run_end (every element after the sort; the rare ones only
                                           // from the sort-free builder)
    uint64_t frequent = 0, rare_pairs = 0;
    uint32_t threshold = 0;
    uint32_t builder = 0;                  // 1: sort-free dictionary builder (dictindex.hip), 2: radix sort of all (hash, row) pairs
    hipStream_t stream = nullptr;          // the arrays come from this stream's pool and go back to it, in order
    ~BitIndex() {
        if (bits) arena_free(bits, stream);
        if (rows_sorted) arena_free(rows_sorted, stream);
        if (run_end) arena_free(run_end, stream);
    }
};

// What both builders end in: the cost model's verdict on what the builder counted (compare_core.hpp: compare_index_accept), the
// index's fields, and the zeroed bit rows.  false: the merge kernel wins, or the bitmap cap (~BitIndex frees what was allocated).
static bool bitindex_finish(BitIndex* bi, const ComparePathModel& model, uint64_t universe, uint64_t n_freq, uint64_t rare_pairs,
                            bool forced, hipStream_t st) {
    const CompareIndexAccept acc = compare_index_accept(bi->n, n_freq, rare_pairs, bi->total, model.t_merge, forced);
    if (!acc.accept) return false;
    bi->universe = universe; bi->frequent = n_freq; bi->rare_pairs = rare_pairs;
    bi->threshold = model.threshold; bi->words_per_row = acc.words;
    if (acc.words) {
        hip_check(arena_alloc((void**)&bi->bits, (size_t)bi->n * acc.words * 4, st), "arena_alloc");
        hip_check(hipMemsetAsync(bi->bits, 0, (size_t)bi->n * acc.words * 4, st), "memset");
    }
    return true;
}

// Build the cheapest exact index for the collection, or return nullptr (no error) when the merge kernel is.
static BitIndex* bitindex_build(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n, hipStream_t st,
                                uint32_t forced_threshold = 0, bool one_shot = false, uint64_t total = 0) {
    if (n == 0) return nullptr;
    if (total == 0) {                                               // the caller did not say how many hashes there are
        hip_check(hipMemcpyAsync(&total, d_offsets + n, 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
    }
    if (total == 0 || total > 0xffffffffull) return nullptr;
    // the threshold, the general kernel's expected time, and whether a builder is worth starting: compare_core.hpp
    const ComparePathModel model = compare_path_model(n, total, forced_threshold, one_shot);
    const uint32_t threshold = model.threshold;
    // The sort-free builder first (dictindex.hip): it serves collections whose distinct hashes fit its per-bucket tables
    // (any collection with heavy sharing: C3 / C4 have 55,000 distinct hashes for 5e6 / 5e7 elements); a bucket that
    // overflows sends the build to the sort below.  SMG_COMPARE_INDEX=sort skips it (tests run both).
    static const bool sort_only = [] { const char* e = getenv("SMG_COMPARE_INDEX"); return e && !strcmp(e, "sort"); }();
    if (!sort_only && model.try_dict) {
        std::unique_ptr<BitIndex> bi(new BitIndex());
        bi->n = n; bi->total = total; bi->stream = st;
        AsyncBuf scratch(dict_scratch_bytes(n), st);
        unsigned long long* d_out = reinterpret_cast<unsigned long long*>(scratch.as<char>() + 64);   // inside the zeroed header
        hip_check(hipMemsetAsync(scratch.p, 0, 256, st), "memset");
        hip_check(dict_count_launch(d_hashes, d_offsets, n, threshold, scratch.p, d_out, st), "dictionary pass 1");
        unsigned long long out[5] = {0, 0, 0, 0, 0};
        hip_check(hipMemcpyAsync(out, d_out, sizeof(out), hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        if (out[4] == 0) {
            const uint64_t rare_elems = out[3];
            if (!bitindex_finish(bi.get(), model, out[0], out[1], out[2], forced_threshold != 0, st)) return nullptr;
            if (rare_elems) {
                hip_check(arena_alloc((void**)&bi->rows_sorted, rare_elems * 4 + 16, st), "arena_alloc");
                hip_check(arena_alloc((void**)&bi->run_end, rare_elems * 4 + 16, st), "arena_alloc");
                bi->inv_total = rare_elems;
            }
            hip_check(dict_emit_launch(d_hashes, d_offsets, n, scratch.p, bi->bits, bi->words_per_row, bi->rows_sorted, bi->run_end, st),
                      "dictionary pass 2");
            bi->builder = 1;
            return bi.release();
        }
    }
    if (!model.try_sort) return nullptr;
    // (hash, row) of the whole collection sorted by hash; runs = distinct hashes with their number of holders.
    // Scratch comes from the stream-ordered pool and the host reads back once: the kernels of a small build take
    // less time than one hipMalloc / hipFree pair or one extra synchronisation.
    std::unique_ptr<BitIndex> bi(new BitIndex());
    bi->n = n; bi->total = total; bi->stream = st;
    const size_t tb = inverted_temp_bytes(total);
    AsyncBuf keys_a(total * 8, st), keys_b(total * 8, st), rows_tmp(total * 4, st), counts((total + 2) * 4, st), tmp(tb, st),
        scal(64, st), flags((total + 2) * 4, st), run_off((total + 2) * 8, st), freq_rank((total + 2) * 8, st);
    hip_check(arena_alloc((void**)&bi->rows_sorted, total * 4 + 16, st), "arena_alloc");
    hip_check(hipMemsetAsync(scal.p, 0, 64, st), "memset");
    uint64_t* d_n_runs = scal.as<uint64_t>();
    unsigned long long* d_out = scal.as<unsigned long long>() + 1;      // [runs, frequent, rare pair increments]
    hip_check(inverted_sort_launch(d_hashes, d_offsets, n, total, keys_a.as<uint64_t>(), keys_b.as<uint64_t>(),
                                   rows_tmp.as<uint32_t>(), bi->rows_sorted, counts.as<uint32_t>(), d_n_runs, tmp.p, tb, st),
              "inverted sort");
    hip_check(inverted_classify_launch(counts.as<uint32_t>(), d_n_runs, total, threshold, flags.as<uint32_t>(),
                                       run_off.as<uint64_t>(), freq_rank.as<uint64_t>(), d_out, tmp.p, tb, st), "classify");
    unsigned long long out[3] = {0, 0, 0};
    hip_check(hipMemcpyAsync(out, d_out, 24, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    const uint64_t U = out[0], n_freq = out[1], rare_pairs = out[2];
    bi->inv_total = total;
    if (!bitindex_finish(bi.get(), model, U, n_freq, rare_pairs, forced_threshold != 0, st)) return nullptr;
    hip_check(arena_alloc((void**)&bi->run_end, total * 4 + 16, st), "arena_alloc");
    hip_check(inverted_apply_launch(run_off.as<uint64_t>(), flags.as<uint32_t>(), freq_rank.as<uint64_t>(), U, total, bi->rows_sorted,
                                    bi->run_end, bi->bits, bi->words_per_row, st), "inverted apply");
    if (rare_pairs == 0 && n_freq == U) {             // nothing is rare: plain bit rows, drop the inverted part
        arena_free(bi->rows_sorted, st); arena_free(bi->run_end, st);
        bi->rows_sorted = bi->run_end = nullptr;
    }
    bi->builder = 2;
    return bi.release();                              // stream-ordered: usable by later work on `st` without a sync
}

static void bitindex_compare(const BitIndex* bi, uint32_t rb_first, uint32_t rb_stride, uint32_t rb_count, uint32_t* d_common,
                             hipStream_t st, bool upper_only = false) {
    if (bi->bits)
        hip_check(bitmatrix_launch(bi->bits, bi->words_per_row, bi->n, rb_first, rb_stride, rb_count, d_common, st, upper_only),
                  "bitmatrix");
    else
        hip_check(hipMemsetAsync(d_common, 0, (size_t)rb_count * 16 * bi->n * 4, st), "memset");
    if (bi->run_end)
        hip_check(rare_pairs_launch(bi->rows_sorted, bi->run_end, bi->inv_total, bi->n, rb_first, rb_stride, rb_count, d_common, st,
                                    upper_only),
                  "rare pairs");
}

// n x n counts of a device-resident CSR into dc (device; ceil(n / 16) * 16 rows): dense collections take the bit-row path
static void compare_counts_device(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n, uint64_t total, AsyncBuf& dc,
                                  hipStream_t st) {
    // result matrices from the arena (kept between calls): hipMalloc / hipFree of a gigabyte per call cost more than the
    // comparison on hosts with a slow driver path
    dc.reset((size_t)((n + 15) / 16 * 16) * n * 4, st);
    std::unique_ptr<BitIndex> bi(bitindex_build(d_hashes, d_offsets, (uint32_t)n, st, 0, true, total));
    if (bi) { // bit rows for the frequent hashes + inverted lists for the rare ones: the triangle, then its mirror image
        bitindex_compare(bi.get(), 0, 1, (uint32_t)((n + 15) / 16), dc.as<uint32_t>(), st, true);
        hip_check(symmetrize_launch(dc.as<uint32_t>(), (uint32_t)n, st), "symmetrize");
    } else    // LDS-tiled merge walk
        hip_check(compare_counts_launch(d_hashes, d_offsets, (uint32_t)n, 0, (uint32_t)n, dc.as<uint32_t>(), st), "compare");
}

static void sketch_params(const KmerMinHash* m, uint64_t* out) {
    out[0] = m->ksize; out[1] = m->hash_function; out[2] = m->seed; out[3] = m->max_hash; out[4] = m->num;
    out[5] = m->track_abundance ? 1 : 0; out[6] = m->size(); out[7] = 0;
}

// ---- all pairs of bottom-k / abundance-tracking sketches (compare_ext.hip) ------------------------------------------
// The reference's compare loop calls similarity() per pair (compare.py:36-54); for num sketches that is the merged-and-
// truncated union rule (minhash.rs:593-621), for sketches that track abundance the angular similarity (minhash.rs:635-702).
static void pack_collection(const SourmashKmerMinHash* const* mhs, uintptr_t n, bool with_abund, std::vector<uint64_t>& offsets,
                            AsyncBuf& dh, AsyncBuf& da, AsyncBuf& doff, bool* narrow, hipStream_t st) {
    offsets.assign(n + 1, 0);
    for (uintptr_t i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + MH(mhs[i])->size();
    const uint64_t total = offsets[n];
    dh.reset(total * 8 + 16, st);
    doff.reset((n + 1) * 8, st);
    if (with_abund) da.reset(total * 8 + 16, st);
    bool small = true;
    upload_rows(mhs, n, offsets, false, dh.p, st);
    if (with_abund) {
        upload_rows(mhs, n, offsets, true, da.p, st);
        for (uintptr_t i = 0; i < n && small; ++i)
            for (uint64_t a : MH(mhs[i])->abunds) small = small && a <= 0xffffffffull;
    }
    hip_check(hipMemcpyAsync(doff.p, offsets.data(), (n + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
    if (narrow) *narrow = small;
}

}  // namespace

namespace smg {

// ... (+ Jaccard) into host matrices.  The matrices leave through the pinned ring (hostxfer.hpp): the f64 matrix of config C4
// is 800 MB, and a pageable hipMemcpy of that size was most of the call.
void compare_device_csr(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n, uint64_t total,
                               uint32_t* common_out, double* jaccard_out, hipStream_t st) {
    AsyncBuf dc;
    compare_counts_device(d_hashes, d_offsets, n, total, dc, st);
    std::unique_ptr<AsyncBuf> dj;
    if (jaccard_out) {
        dj.reset(new AsyncBuf((size_t)n * n * 8, st));
        hip_check(jaccard_from_counts_launch(dc.as<uint32_t>(), d_offsets, (uint32_t)n, 0, (uint32_t)n, dj->as<double>(), st), "jaccard");
    }
    if (common_out) HostXfer::get().device_to_host(common_out, dc.p, (size_t)n * n * 4, st);     // (travels while the Jaccard kernel runs)
    if (jaccard_out) HostXfer::get().device_to_host(jaccard_out, dj->p, (size_t)n * n * 8, st);
    hip_check(hipStreamSynchronize(st), "sync");
}

// the hash vectors (or abundance vectors) of n sketches back to back into d_dst: worker threads pack pinned chunks, ONE H2D copy
// per 32 MiB chunk (round 4: one pageable copy per sketch)
void upload_rows(const SourmashKmerMinHash* const* mhs, uintptr_t n, const std::vector<uint64_t>& offsets, bool abunds,
                        void* d_dst, hipStream_t st) {
    std::vector<HostPiece> pieces(n);
    for (uintptr_t i = 0; i < n; ++i) {
        const KmerMinHash* m = MH(mhs[i]);
        pieces[i] = HostPiece{abunds ? (const void*)m->abunds.data() : (const void*)m->mins.data(), (size_t)offsets[i] * 8, m->size() * 8};
    }
    HostXfer::get().gather_to_device(d_dst, pieces, (size_t)offsets[n] * 8, st);
}

}  // namespace smg

extern "C" {

// host float helper of the compare layer: out[i] = pow(x[i], y[ny == 1 ? 0 : i]) with this process's libm -- the
// function CPython's float ** ends in (floatobject.c float_pow), which is what the reference's containment / ANI
// formulas evaluate (minhash.py:832-834, distance_utils.py:283).  No device involved; threads split the array.
void smgpu_host_pow_f64(const double* x, const double* y, uintptr_t ny, double* out, uintptr_t n, uint32_t n_threads) {
    landing_void([&] {
        if (n == 0) return;
        if (!x || !y || !out) throw err_internal("null pointer");
        size_t t = n_threads ? n_threads : std::thread::hardware_concurrency();
        if (t > 64) t = 64;
        if (t < 1 || n < 65536) t = 1;
        auto work = [&](size_t lo, size_t hi) {
            if (ny == 1) { const double e = y[0]; for (size_t i = lo; i < hi; ++i) out[i] = std::pow(x[i], e); }
            else for (size_t i = lo; i < hi; ++i) out[i] = std::pow(x[i], y[i]);
        };
        if (t == 1) { work(0, n); return; }
        std::vector<std::thread> pool;
        for (size_t k = 0; k < t; ++k) pool.emplace_back(work, n * k / t, n * (k + 1) / t);
        for (auto& th : pool) th.join();
    });
}

void smgpu_compare_raw(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n, uint32_t row_lo, uint32_t row_hi,
                       uint32_t* d_common, double* d_jaccard, void* stream) {
    landing_void([&] {
        if (!d_common) throw err_internal("d_common is required");
        hip_check(compare_counts_launch(d_hashes, d_offsets, n, row_lo, row_hi, d_common, (hipStream_t)stream), "compare");
        if (d_jaccard)
            hip_check(jaccard_from_counts_launch(d_common, d_offsets, n, row_lo, row_hi, d_jaccard, (hipStream_t)stream), "jaccard");
    });
}

void smgpu_compare_blocks_raw(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n, uint32_t rb_first,
                              uint32_t rb_stride, uint32_t rb_count, uint32_t* d_common, void* stream) {
    landing_void([&] {
        hip_check(compare_blocks_launch(d_hashes, d_offsets, n, rb_first, rb_stride, rb_count, d_common, (hipStream_t)stream),
                  "compare_blocks");
    });
}
void smgpu_symmetrize_raw(uint32_t* d_common, uint32_t n, void* stream) {
    landing_void([&] { hip_check(symmetrize_launch(d_common, n, (hipStream_t)stream), "symmetrize"); });
}
void smgpu_jaccard_raw(const uint32_t* d_common, const uint64_t* d_offsets, uint32_t n, uint32_t row_lo, uint32_t row_hi,
                       double* d_jaccard, void* stream) {
    landing_void([&] {
        hip_check(jaccard_from_counts_launch(d_common, d_offsets, n, row_lo, row_hi, d_jaccard, (hipStream_t)stream), "jaccard");
    });
}

SmgpuBitIndex* smgpu_bitindex_new(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n, void* stream) {
    return landing<SmgpuBitIndex*>([&]() -> SmgpuBitIndex* {
        return reinterpret_cast<SmgpuBitIndex*>(bitindex_build(d_hashes, d_offsets, n, (hipStream_t)stream));
    });
}
SmgpuBitIndex* smgpu_bitindex_new_ex(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n, uint64_t total_hashes,
                                     uint32_t threshold, bool one_shot, void* stream) {
    return landing<SmgpuBitIndex*>([&]() -> SmgpuBitIndex* {
        return reinterpret_cast<SmgpuBitIndex*>(bitindex_build(d_hashes, d_offsets, n, (hipStream_t)stream, threshold, one_shot,
                                                               total_hashes));
    });
}
void smgpu_bitindex_free(SmgpuBitIndex* p) { delete reinterpret_cast<BitIndex*>(p); }
uint64_t smgpu_bitindex_universe(const SmgpuBitIndex* p) { return reinterpret_cast<const BitIndex*>(p)->universe; }
uint32_t smgpu_bitindex_builder(const SmgpuBitIndex* p) { return reinterpret_cast<const BitIndex*>(p)->builder; }
void smgpu_bitindex_stats(const SmgpuBitIndex* p, uint64_t* frequent_hashes, uint64_t* rare_pairs, uint32_t* threshold) {
    const BitIndex* bi = reinterpret_cast<const BitIndex*>(p);
    *frequent_hashes = bi->frequent ? bi->frequent : (bi->run_end ? 0 : bi->universe);
    *rare_pairs = bi->rare_pairs;
    *threshold = bi->threshold;
}
void smgpu_bitindex_compare_raw(const SmgpuBitIndex* p, uint32_t rb_first, uint32_t rb_stride, uint32_t rb_count,
                                uint32_t* d_common, void* stream) {
    landing_void([&] {
        bitindex_compare(reinterpret_cast<const BitIndex*>(p), rb_first, rb_stride, rb_count, d_common, (hipStream_t)stream);
    });
}
void smgpu_bitindex_compare_upper_raw(const SmgpuBitIndex* p, uint32_t rb_first, uint32_t rb_stride, uint32_t rb_count,
                                      uint32_t* d_common, void* stream) {
    landing_void([&] {
        bitindex_compare(reinterpret_cast<const BitIndex*>(p), rb_first, rb_stride, rb_count, d_common, (hipStream_t)stream, true);
    });
}

void smgpu_compare_all_pairs(const SourmashKmerMinHash* const* mhs, uintptr_t n, uint32_t* common_out, double* jaccard_out) {
    landing_void([&] {
        if (n == 0) return;
        if (n > 0xffffffffu) throw err_internal("too many sketches");
        for (uintptr_t i = 1; i < n; ++i) MH(mhs[0])->check_compatible(*MH(mhs[i]));
        if (MH(mhs[0])->num != 0)
            throw err_internal("smgpu_compare_all_pairs handles scaled sketches; use kmerminhash_similarity for num sketches");
        std::vector<uint64_t> offsets(n + 1, 0);
        for (uintptr_t i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + MH(mhs[i])->size();
        const uint64_t total = offsets[n];
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        AsyncBuf dh(total * 8 + 16, st), doff((n + 1) * 8, st);
        upload_rows(mhs, n, offsets, false, dh.p, st);
        hip_check(hipMemcpyAsync(doff.p, offsets.data(), (n + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
        compare_device_csr(dh.as<uint64_t>(), doff.as<uint64_t>(), n, total, common_out, jaccard_out, st);
    });
}

// A list with SEVERAL scaled values, downsample = True: common_out[i][j] = |A ∩ B| with both sketches downsampled to the pair's
// coarser scaled (compare.py:14-64 -> minhash.rs:682-702, 777-798), the diagonal = the row's size as given.  class_of[i]: index of
// sketch i's own scaled value in the ascending list of distinct values; class_max_hash[c]: max_hash of value c.  sizes_out
// [n_classes][n]: the size of sketch i downsampled to value c (0 where c is finer than the sketch).  One upload of the
// sketches as given, the prefixes of every class gathered on the device; the host builds no downsampled sketch objects.
void smgpu_compare_all_pairs_mixed(const SourmashKmerMinHash* const* mhs, uintptr_t n, const uint32_t* class_of,
                                   const uint64_t* class_max_hash, uintptr_t n_classes, uint32_t* common_out, uint64_t* sizes_out) {
    landing_void([&] {
        if (n == 0 || n_classes == 0) return;
        if (n > 0xffffffffu) throw err_internal("too many sketches");
        if (!class_of || !class_max_hash || !common_out || !sizes_out) throw err_internal("null pointer");
        for (uintptr_t i = 1; i < n; ++i) {                          // as check_compatible with downsample = true: everything but the threshold
            const KmerMinHash *a = MH(mhs[0]), *b = MH(mhs[i]);
            if (a->ksize != b->ksize) throw Error(E_MISMATCH_KSIZES, "different ksizes cannot be compared");
            if (a->hash_function != b->hash_function) throw Error(E_MISMATCH_DNA_PROT, "DNA/prot minhashes cannot be compared");
            if (a->seed != b->seed) throw Error(E_MISMATCH_SEED, "mismatch in seed; comparison fail");
        }
        for (uintptr_t i = 0; i < n; ++i) {
            if (MH(mhs[i])->num != 0 || MH(mhs[i])->max_hash == 0) throw err_internal("smgpu_compare_all_pairs_mixed takes scaled sketches");
            if (class_of[i] >= n_classes) throw err_internal("class index out of range");
        }
        std::vector<uint64_t> offsets(n + 1, 0);
        for (uintptr_t i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + MH(mhs[i])->size();
        const uint64_t total = offsets[n];
        // prefix lengths: hashes <= max_hash of every class at least as coarse as the sketch's own (minhash.rs:777-798)
        for (uintptr_t c = 0; c < n_classes; ++c)
            for (uintptr_t i = 0; i < n; ++i) {
                const KmerMinHash* m = MH(mhs[i]);
                uint64_t len = 0;
                if (class_of[i] == c) len = m->size();
                else if (class_of[i] < c) len = (uint64_t)(std::upper_bound(m->mins.begin(), m->mins.end(), class_max_hash[c]) - m->mins.begin());
                sizes_out[c * n + i] = len;
            }
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        AsyncBuf dh(total * 8 + 16, st), dcls(n * 4 + 16, st), dout((size_t)n * n * 4 + 16, st);
        upload_rows(mhs, n, offsets, false, dh.p, st);
        hip_check(hipMemcpyAsync(dcls.p, class_of, n * 4, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipMemsetAsync(dout.p, 0, (size_t)n * n * 4, st), "memset");
        std::vector<uint64_t> src, noff;
        std::vector<uint32_t> rows;
        for (uintptr_t c = 0; c < n_classes; ++c) {
            rows.clear(); src.clear(); noff.assign(1, 0);
            bool any_own = false;
            for (uintptr_t i = 0; i < n; ++i)
                if (class_of[i] <= c) {
                    rows.push_back((uint32_t)i);
                    src.push_back(offsets[i]);
                    noff.push_back(noff.back() + sizes_out[c * n + i]);
                    any_own = any_own || class_of[i] == c;
                }
            const uint32_t m = (uint32_t)rows.size();
            if (!any_own || m == 0) continue;
            AsyncBuf dsrc(m * 8 + 16, st), dnoff((m + 1) * 8 + 16, st), drows(m * 4 + 16, st), dsub_h(noff.back() * 8 + 16, st), dsub;
            hip_check(hipMemcpyAsync(dsrc.p, src.data(), m * 8, hipMemcpyHostToDevice, st), "H2D");
            hip_check(hipMemcpyAsync(dnoff.p, noff.data(), (m + 1) * 8, hipMemcpyHostToDevice, st), "H2D");
            hip_check(hipMemcpyAsync(drows.p, rows.data(), m * 4, hipMemcpyHostToDevice, st), "H2D");
            hip_check(csr_prefix_gather_launch(dh.as<uint64_t>(), dsrc.as<uint64_t>(), dnoff.as<uint64_t>(), m, dsub_h.as<uint64_t>(), st), "gather rows");
            compare_counts_device(dsub_h.as<uint64_t>(), dnoff.as<uint64_t>(), m, noff.back(), dsub, st);
            hip_check(class_scatter_launch(dsub.as<uint32_t>(), m, drows.as<uint32_t>(), dcls.as<uint32_t>(), (uint32_t)c, (uint32_t)n,
                                           dout.as<uint32_t>(), st), "scatter class");
            hip_check(hipStreamSynchronize(st), "sync");             // (the host vectors above are reused by the next class)
        }
        HostXfer::get().device_to_host(common_out, dout.p, (size_t)n * n * 4, st);
        hip_check(hipStreamSynchronize(st), "sync");
    });
}

// The first sketch of each signature WITHOUT the clone signature_first_mh makes (ffi/signature.rs:167-182 clones; a 10,000-signature
// compare cloned 400 MB before it started), and every sketch's parameters in one call instead of a dozen FFI calls per sketch:
// params[i] = {ksize as stored, hash_function, seed, max_hash, num, track_abundance, size, 0}.  The handles are BORROWED: valid while
// the signature lives and is not modified, never to be freed.

void smgpu_signatures_sketch_views(const SourmashSignature* const* sigs, uintptr_t n, const SourmashKmerMinHash** out_mhs, uint64_t* params) {
    landing_void([&] {
        for (uintptr_t i = 0; i < n; ++i) {
            if (SIG(sigs[i])->sketches.empty()) throw err_internal("found unsupported sketch type");
            const KmerMinHash* m = &SIG(sigs[i])->sketches[0];
            out_mhs[i] = reinterpret_cast<const SourmashKmerMinHash*>(m);
            sketch_params(MH(out_mhs[i]), params + 8 * i);             // (MH: queued records are hashed first, like every reader)
        }
    });
}
void smgpu_minhashes_params(const SourmashKmerMinHash* const* mhs, uintptr_t n, uint64_t* params) {
    landing_void([&] { for (uintptr_t i = 0; i < n; ++i) sketch_params(MH(mhs[i]), params + 8 * i); });
}

void smgpu_compare_num_all_pairs(const SourmashKmerMinHash* const* mhs, uintptr_t n, uint32_t* common_out, uint32_t* union_out,
                                 double* jaccard_out) {
    landing_void([&] {
        if (n == 0) return;
        if (n > 0xffffffffu) throw err_internal("too many sketches");
        for (uintptr_t i = 1; i < n; ++i) MH(mhs[0])->check_compatible(*MH(mhs[i]));
        std::vector<uint32_t> nums(n);
        for (uintptr_t i = 0; i < n; ++i) {
            nums[i] = MH(mhs[i])->num;
            if (nums[i] == 0) throw err_internal("smgpu_compare_num_all_pairs takes bottom-k (num) sketches; scaled sketches go to smgpu_compare_all_pairs");
        }
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::vector<uint64_t> offsets;
        AsyncBuf dh, da, doff;
        pack_collection(mhs, n, false, offsets, dh, da, doff, nullptr, st);
        AsyncBuf dn(n * 4, st), dc((size_t)n * n * 4, st), du((size_t)n * n * 4, st), dj((size_t)n * n * 8, st);
        hip_check(hipMemcpyAsync(dn.p, nums.data(), n * 4, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipMemsetAsync(dc.p, 0, (size_t)n * n * 4, st), "memset");
        hip_check(compare_num_launch(dh.as<uint64_t>(), doff.as<uint64_t>(), dn.as<uint32_t>(), (uint32_t)n, dc.as<uint32_t>(),
                                     du.as<uint32_t>(), dj.as<double>(), st), "compare (num)");
        if (common_out) HostXfer::get().device_to_host(common_out, dc.p, (size_t)n * n * 4, st);
        if (union_out) HostXfer::get().device_to_host(union_out, du.p, (size_t)n * n * 4, st);
        if (jaccard_out) HostXfer::get().device_to_host(jaccard_out, dj.p, (size_t)n * n * 8, st);
        hip_check(hipStreamSynchronize(st), "sync");
    });
}

// out[i][j] = 1 - 2 acos(min(prod / (sqrt(sq_i) sqrt(sq_j)), 1)) / pi, 0 when a norm is 0 (minhash.rs:662-679); the host's libm
// like the reference's f64::sqrt / f64::acos; the diagonal is 1.0 (compare.py:33)
void smgpu_host_angular_f64(const uint64_t* prod, const uint64_t* sumsq, uintptr_t n, double* out, uint32_t n_threads) {
    landing_void([&] {
        if (n == 0) return;
        if (!prod || !sumsq || !out) throw err_internal("null pointer");
        size_t t = n_threads ? n_threads : std::thread::hardware_concurrency();
        if (t > 64) t = 64;
        if (t < 1 || n < 256) t = 1;
        std::vector<double> norm(n);
        for (uintptr_t i = 0; i < n; ++i) norm[i] = std::sqrt((double)sumsq[i]);
        auto work = [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i)
                for (size_t j = 0; j < n; ++j) {
                    double v;
                    if (i == j) v = 1.0;
                    else if (norm[i] == 0.0 || norm[j] == 0.0) v = 0.0;
                    else {
                        // the pair is evaluated as similarity(lower index, higher index): norm_a belongs to the lower one
                        const double na = i < j ? norm[i] : norm[j], nb = i < j ? norm[j] : norm[i];
                        double p = (double)prod[i * n + j] / (na * nb);
                        if (p > 1.0) p = 1.0;
                        v = 1.0 - 2.0 * std::acos(p) / 3.14159265358979323846264338327950288;
                    }
                    out[i * n + j] = v;
                }
        };
        if (t == 1) { work(0, n); return; }
        std::vector<std::thread> pool;
        for (size_t k = 0; k < t; ++k) pool.emplace_back(work, n * k / t, n * (k + 1) / t);
        for (auto& th : pool) th.join();
    });
}

void smgpu_compare_angular_all_pairs(const SourmashKmerMinHash* const* mhs, uintptr_t n, double* sims_out, uint64_t* prod_out,
                                     uint64_t* sumsq_out) {
    landing_void([&] {
        if (n == 0) return;
        if (n > 0xffffffffu) throw err_internal("too many sketches");
        for (uintptr_t i = 1; i < n; ++i) MH(mhs[0])->check_compatible(*MH(mhs[i]));
        for (uintptr_t i = 0; i < n; ++i)
            if (!MH(mhs[i])->track_abundance) throw Error(E_NEEDS_ABUNDANCE_TRACKING, "sketch needs abundance for this operation");
        std::vector<uint64_t> prod((size_t)n * n), sq(n);
        {
            DeviceCtx& ctx = DeviceCtx::get();
            std::lock_guard<std::recursive_mutex> g(ctx.mutex());
            hipStream_t st = ctx.stream();
            std::vector<uint64_t> offsets;
            AsyncBuf dh, da, doff;
            bool narrow = true;
            pack_collection(mhs, n, true, offsets, dh, da, doff, &narrow, st);
            AsyncBuf dc((size_t)n * n * 4, st), dp((size_t)n * n * 8, st), ds(n * 8, st);
            hip_check(hipMemsetAsync(dc.p, 0, (size_t)n * n * 4, st), "memset");
            hip_check(hipMemsetAsync(dp.p, 0, (size_t)n * n * 8, st), "memset");
            hip_check(compare_abund_launch(dh.as<uint64_t>(), da.as<uint64_t>(), doff.as<uint64_t>(), (uint32_t)n, narrow,
                                           dc.as<uint32_t>(), dp.as<unsigned long long>(), ds.as<unsigned long long>(), st, offsets.empty() ? 0 : offsets.back()),
                      "compare (abundance)");
            HostXfer::get().device_to_host(prod.data(), dp.p, (size_t)n * n * 8, st);
            hip_check(hipMemcpyAsync(sq.data(), ds.p, n * 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
        }
        if (prod_out) memcpy(prod_out, prod.data(), (size_t)n * n * 8);
        if (sumsq_out) memcpy(sumsq_out, sq.data(), n * 8);
        if (sims_out) smgpu_host_angular_f64(prod.data(), sq.data(), n, sims_out, 0);
    });
}

// the same kernels on caller-owned device buffers (torch tensors): benchmarks, and callers that keep collections resident
void smgpu_compare_num_raw(const uint64_t* d_hashes, const uint64_t* d_offsets, const uint32_t* d_nums, uint32_t n, uint32_t* d_common,
                           uint32_t* d_union, double* d_jaccard, void* stream) {
    landing_void([&] { hip_check(compare_num_launch(d_hashes, d_offsets, d_nums, n, d_common, d_union, d_jaccard, (hipStream_t)stream), "compare (num)"); });
}
void smgpu_compare_abund_raw(const uint64_t* d_hashes, const uint64_t* d_abunds, const uint64_t* d_offsets, uint32_t n, bool narrow,
                             uint32_t* d_common, uint64_t* d_prod, uint64_t* d_sumsq, void* stream) {
    landing_void([&] {
        hip_check(compare_abund_launch(d_hashes, d_abunds, d_offsets, n, narrow, d_common, (unsigned long long*)d_prod,
                                       (unsigned long long*)d_sumsq, (hipStream_t)stream), "compare (abundance)");
    });
}

void smgpu_compare_abund_raw_n(const uint64_t* d_hashes, const uint64_t* d_abunds, const uint64_t* d_offsets, uint32_t n, uint64_t total_hashes,
                               bool narrow, uint32_t* d_common, uint64_t* d_prod, uint64_t* d_sumsq, void* stream) {
    landing_void([&] {
        hip_check(compare_abund_launch(d_hashes, d_abunds, d_offsets, n, narrow, d_common, (unsigned long long*)d_prod,
                                       (unsigned long long*)d_sumsq, (hipStream_t)stream, total_hashes), "compare (abundance)");
    });
}

}  // extern "C"
