// capi_ingest.cpp -- the C-ABI (include/sourmash_amd.h): files and device buffers into sketches (ingest.hpp, sketch.hip,
// uniform_sort.hip / device_sort.hip, protein.hip, synth.hip), inflating gzip files (gunzip.hip, pargz.hpp), and the library's memory:
// page-locked host buffers (hostxfer.hpp) and the device arena (arena.hpp).
#include <stdio.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include "capi_common.hpp"
#include "ingest.hpp"
#include "pargz.hpp"
#include "residues.hpp"
#include "sigload.hpp"
#include "uniform_sort_core.hpp"

using namespace smg;

namespace {

// Workspace of a sketch call: [unordered kept hashes: cap u64][a report of three words and the fall-back flag: 256 bytes][the sort's
// scratch: the uniform sort's regions (uniform_sort.hip), which the general sort reuses when it has to take over]
static size_t sketch_ws_raw_bytes(uint64_t cap) { return al256(cap * 8); }
static size_t sketch_ws_sort_bytes(uint64_t cap, bool counts) {
    return std::max(sort_unique_temp_bytes(cap), sort_unique_uniform_temp_bound(cap, counts));
}

struct SortCounters { std::atomic<uint64_t> bucket{0}, small{0}, fellback{0}; };
static SortCounters& sort_counters() { static SortCounters c; return c; }

// The uniform sort on d_keys[0, min(*d_n, n_max)), then ONE copy to the host and ONE synchronisation: -> {*d_n, distinct, fell back}
// as the device left them.  d_head: 256 bytes of workspace (report and flag).
static void uniform_sort_and_report(const uint64_t* d_keys, const unsigned long long* d_n, uint64_t n_max, uint64_t thr, uint64_t* d_out,
                                    uint64_t* d_counts, uint64_t* d_n_out, void* d_head, void* d_tmp, size_t tmp_bytes, hipStream_t st,
                                    uint64_t report[3]) {
    uint64_t* d_report = (uint64_t*)d_head;
    uint32_t* d_flag = (uint32_t*)((char*)d_head + 64);
    hip_check(sort_unique_uniform(d_keys, d_n, n_max, thr, d_out, d_counts, d_n_out, d_flag, d_tmp, tmp_bytes, st), "sort_unique_uniform");
    hip_check(sort_report_launch(d_n, d_n_out, d_flag, d_report, st), "sort_report");
    hip_check(hipMemcpyAsync(report, d_report, 24, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
}
static void count_sort_call(uint64_t n_max, uint64_t thr, size_t tmp_bytes, bool counts, bool fellback) {
    if (fellback) ++sort_counters().fellback;
    else if (sort_unique_uniform_form(n_max, thr, tmp_bytes, counts) == US_SMALL) ++sort_counters().small;
    else ++sort_counters().bucket;
}
static int key_bits(uint64_t thr) {
    int bits = 64;
    if (thr != ~0ull) { bits = 1; while (bits < 64 && (thr >> bits)) ++bits; }
    return bits;
}

}  // namespace

extern "C" {

uint64_t smgpu_signature_add_file(SourmashSignature* p, const char* path, uint64_t* n_records) {
    return landing<uint64_t>([&]() -> uint64_t {
        if (!path) throw err_internal("null path");
        std::vector<KmerMinHash*> mhs;
        for (auto& mh : SIG(p)->sketches) mhs.push_back(&mh);
        uint64_t recs = 0, bases = 0;
        sketch_file_into(mhs, path, &recs, &bases);
        if (n_records) *n_records = recs;
        return bases;
    });
}
SourmashSignature** smgpu_sketch_files(const char* const* paths, uintptr_t n, const SourmashComputeParameters* params,
                                       uint32_t n_threads, uint64_t* total_bases) {
    return landing<SourmashSignature**>([&]() -> SourmashSignature** {
        if (!paths && n) throw err_internal("null paths");
        if (!CP(params)->dna || CP(params)->protein || CP(params)->dayhoff || CP(params)->hp)
            throw err_internal("smgpu_sketch_files takes DNA parameters; protein / dayhoff / hp sketches are fed record by record");
        std::vector<std::string> files(paths, paths + n);
        std::vector<Signature> sigs;
        uint64_t bases = 0;
        sketch_files_parallel(files, *CP(params), n_threads, sigs, &bases);
        if (total_bases) *total_bases = bases;
        uintptr_t size = 0;
        return sigs_out(std::move(sigs), &size);
    });
}
uint64_t smgpu_gunzip_files(const char* const* paths, uintptr_t n, uint8_t* out, uint64_t capacity, uint64_t* lens, double* stats) {
    return landing<uint64_t>([&]() -> uint64_t {
        if ((!paths || !lens) && n) throw err_internal("null paths");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<GunzipMember> ms(n);
        std::vector<std::vector<uint8_t>> blobs(n);
        uint64_t total = 0;
        for (uintptr_t i = 0; i < n; ++i) {
            FILE* f = fopen(paths[i], "rb");
            if (!f) throw Error(E_IO, std::string("No such file or directory: ") + paths[i]);
            fseek(f, 0, SEEK_END);
            const long sz = ftell(f);
            fseek(f, 0, SEEK_SET);
            blobs[i].resize((size_t)std::max(0L, sz));
            const size_t got = sz > 0 ? fread(blobs[i].data(), 1, (size_t)sz, f) : 0;
            fclose(f);
            if (got != (size_t)std::max(0L, sz)) throw Error(E_IO, std::string("short read on ") + paths[i]);
            ms[i].file_off = total;
            ms[i].file_len = (uint64_t)sz;
            total += ((uint64_t)sz + 7) & ~7ull;
        }
        PinnedBuf host;
        host.reserve((size_t)total + GUNZIP_PAD);
        memset(host.p, 0, (size_t)total + GUNZIP_PAD);
        for (uintptr_t i = 0; i < n; ++i) memcpy(host.p + ms[i].file_off, blobs[i].data(), blobs[i].size());
        blobs.clear();
        AsyncBuf dev((size_t)total + GUNZIP_PAD, st);
        hip_check(hipMemcpyAsync(dev.p, host.p, (size_t)total + GUNZIP_PAD, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipStreamSynchronize(st), "sync");
        const double io_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        void* d_out = nullptr;
        GunzipStats gs;
        gunzip_device(host.p, dev.as<uint8_t>(), total, ms, &d_out, st, &gs);
        struct FreeOut { void* p; hipStream_t st; ~FreeOut() { if (p) arena_free(p, st); } } free_out{d_out, st};
        uint64_t at = 0;
        for (uintptr_t i = 0; i < n; ++i) {
            if (!ms[i].ok) { lens[i] = ~0ull; continue; }
            if (at + ms[i].out_len > capacity) throw err_internal("smgpu_gunzip_files: output capacity too small");
            if (ms[i].out_len)
                hip_check(hipMemcpyAsync(out + at, (const uint8_t*)d_out + ms[i].out_off, (size_t)ms[i].out_len, hipMemcpyDeviceToHost, st), "D2H");
            lens[i] = ms[i].out_len;
            at += ms[i].out_len;
        }
        hip_check(hipStreamSynchronize(st), "sync");
        if (stats) {
            const double v[10] = {(double)gs.survivors, (double)gs.candidates, (double)gs.runs, gs.scan_ms, gs.pass1_ms, gs.link_ms, gs.pass2_ms,
                                  gs.finish_ms, gs.total_ms, io_ms};
            for (int k = 0; k < 16; ++k) stats[k] = k < 10 ? v[k] : 0.0;
        }
        return at;
    });
}
void smgpu_sigload_counters(uint64_t* out) {
    if (!out) return;
    out[0] = sigload_counters().on_device.load();
    out[1] = sigload_counters().on_host.load();
}
void smgpu_gunzip_counters(uint64_t* out) {
    if (!out) return;
    out[0] = gunzip_counters().on_device.load();
    out[1] = gunzip_counters().refused.load();
}
uint64_t smgpu_minhash_add_file(SourmashKmerMinHash* p, const char* path, uint64_t* n_records) {
    return landing<uint64_t>([&]() -> uint64_t {
        if (!path) throw err_internal("null path");
        std::vector<KmerMinHash*> mhs{MH(p)};
        uint64_t recs = 0, bases = 0;
        sketch_file_into(mhs, path, &recs, &bases);
        if (n_records) *n_records = recs;
        return bases;
    });
}

uint64_t smgpu_sketch_workspace_bytes(uint64_t out_capacity) {
    return (uint64_t)sketch_ws_raw_bytes(out_capacity) + 256 + sketch_ws_sort_bytes(out_capacity, false) + 512;
}

void smgpu_sort_counters(uint64_t* out) {
    if (!out) return;
    out[0] = sort_counters().bucket.load();
    out[1] = sort_counters().small.load();
    out[2] = sort_counters().fellback.load();
}

uint64_t smgpu_sketch_dna_raw(const uint8_t* d_seq, uint64_t len, uint32_t ksize, uint64_t seed, uint64_t max_hash,
                              uint64_t* d_out, uint64_t cap, uint64_t* d_result, void* d_ws, uint64_t ws_bytes,
                              void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        hipStream_t st = (hipStream_t)stream;
        if (ws_bytes < smgpu_sketch_workspace_bytes(cap)) throw err_internal("workspace too small (smgpu_sketch_workspace_bytes)");
        uint64_t* d_raw = (uint64_t*)d_ws;                                   // unordered kept hashes
        void* d_head = (char*)d_ws + sketch_ws_raw_bytes(cap);
        void* d_tmp = (char*)d_head + 256;
        const size_t tmp_bytes = (size_t)(ws_bytes - sketch_ws_raw_bytes(cap) - 256);
        const uint64_t thr = max_hash ? max_hash : ~0ull;
        check_dna_ksize(ksize);
        hip_check(hipMemsetAsync(d_result, 0, 16, st), "memset");
        hip_check(sketch_dna_launch(d_seq, len, ksize, seed, thr, d_raw, (unsigned long long*)d_result, cap, st), "sketch_dna");
        // the kept count stays on the device: the sort reads it there, and the one synchronisation of the call is behind the sort
        uint64_t report[3] = {0, 0, 0};
        uniform_sort_and_report(d_raw, (const unsigned long long*)d_result, cap, thr, d_out, nullptr, d_result + 1, d_head, d_tmp, tmp_bytes,
                                st, report);
        const uint64_t kept = report[0];
        if (kept > cap)
            throw err_internal("output capacity too small: " + std::to_string(kept) + " kept hashes > capacity " + std::to_string(cap));
        count_sort_call(cap, thr, tmp_bytes, false, report[2] != 0);
        if (report[2] == 0) { ret = report[1]; return; }
        // the keys did not spread like hashes (one k-mer repeated, a short period): the general sort, on the kept hashes as they were
        hip_check(sort_unique(d_raw, kept, d_out, nullptr, d_result + 1, d_tmp, tmp_bytes, key_bits(thr), st), "sort_unique");
        unsigned long long nu = 0;
        hip_check(hipMemcpyAsync(&nu, d_result + 1, 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        ret = nu;
    });
    return ret;
}

uint64_t smgpu_sort_unique_uniform_workspace_bytes(uint64_t n_max, int32_t counts) {
    return 256 + (uint64_t)sketch_ws_sort_bytes(n_max, counts != 0) + 512;
}

uint64_t smgpu_sort_unique_uniform_raw(uint64_t* d_keys, const uint64_t* d_n, uint64_t n_max, uint64_t thr, uint64_t* d_out, uint64_t* d_counts,
                                       uint64_t* d_result, void* d_ws, uint64_t ws_bytes, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        hipStream_t st = (hipStream_t)stream;
        if (!d_keys || !d_n || !d_out || !d_result || !d_ws) throw err_internal("null pointer");
        if (ws_bytes < smgpu_sort_unique_uniform_workspace_bytes(n_max, d_counts != nullptr))
            throw err_internal("workspace too small (smgpu_sort_unique_uniform_workspace_bytes)");
        void* d_tmp = (char*)d_ws + 256;
        const size_t tmp_bytes = (size_t)(ws_bytes - 256);
        uint64_t report[3] = {0, 0, 0};
        uniform_sort_and_report(d_keys, (const unsigned long long*)d_n, n_max, thr, d_out, d_counts, d_result, d_ws, d_tmp, tmp_bytes, st, report);
        count_sort_call(n_max, thr, tmp_bytes, d_counts != nullptr, report[2] != 0);
        if (report[2] == 0) { ret = report[1]; return; }
        const uint64_t n = std::min(report[0], n_max);
        hip_check(sort_unique(d_keys, n, d_out, d_counts, d_result, d_tmp, tmp_bytes, 64, st), "sort_unique");
        unsigned long long nu = 0;
        hip_check(hipMemcpyAsync(&nu, d_result, 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        ret = nu;
    });
    return ret;
}

uint64_t smgpu_sort_unique_raw(uint64_t* d_keys, uint64_t n, uint64_t* d_out, uint64_t* d_n_out, void* d_ws, uint64_t ws_bytes, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        hipStream_t st = (hipStream_t)stream;
        if (ws_bytes < sort_unique_temp_bytes(n)) throw err_internal("workspace too small (smgpu_sketch_workspace_bytes)");
        hip_check(sort_unique(d_keys, n, d_out, nullptr, d_n_out, d_ws, (size_t)ws_bytes, 64, st), "sort_unique");
        unsigned long long nu = 0;
        hip_check(hipMemcpyAsync(&nu, d_n_out, 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        ret = nu;
    });
    return ret;
}

void smgpu_sketch_dna_kernel_raw(const uint8_t* d_seq, uint64_t len, uint32_t ksize, uint64_t seed, uint64_t max_hash,
                                 uint64_t* d_out, uint64_t cap, uint64_t* d_count, void* stream) {
    landing_void([&] {
        check_dna_ksize(ksize);
        hip_check(sketch_dna_launch(d_seq, len, ksize, seed, max_hash ? max_hash : ~0ull, d_out,
                                    (unsigned long long*)d_count, cap, (hipStream_t)stream), "sketch_dna");
    });
}
void smgpu_sketch_dna_kernel_grid_raw(const uint8_t* d_seq, uint64_t len, uint32_t ksize, uint64_t seed, uint64_t max_hash,
                                      uint64_t* d_out, uint64_t cap, uint64_t* d_count, uint32_t grid, void* stream) {
    landing_void([&] {
        check_dna_ksize(ksize);
        if (grid > (1u << 20)) throw err_internal("grid: at most 1048576 workgroups");
        hip_check(sketch_dna_launch_grid(d_seq, len, ksize, seed, max_hash ? max_hash : ~0ull, d_out,
                                         (unsigned long long*)d_count, cap, grid, (hipStream_t)stream), "sketch_dna");
    });
}

// The kernels behind protein / dayhoff / hp sketches on device-resident input (benchmarks; the object API goes through
// DeviceCtx::protein_sketch_host): residues of a protein sequence, or the six-frame translation of DNA (signature.rs:307-393), into
// d_aa, then every window of k_aa residues hashed and the hashes 1 <= h <= max_hash appended to d_out.  -> residues written.
uint64_t smgpu_sketch_residues_kernels_raw(const uint8_t* d_seq, uint64_t len, uint32_t k_aa, uint32_t hash_function, uint64_t seed,
                                           uint64_t max_hash, bool translate, uint8_t* d_aa, uint64_t aa_capacity, uint64_t* d_out,
                                           uint64_t cap, uint64_t* d_count, void* stream) {
    return landing<uint64_t>([&]() -> uint64_t {
        if (hash_function < HF_PROTEIN || hash_function > HF_HP) throw err_internal("hash_function must be protein, dayhoff or hp");
        const uint64_t n_aa = translate ? translated_bytes(len) : len;
        // (the window kernel reads d_aa in aligned 8-byte words: the capacity has to cover the last word it touches)
        if (((n_aa + 7) & ~7ull) > aa_capacity) throw err_internal("d_aa is too small: " + std::to_string(n_aa) + " residues need " + std::to_string((n_aa + 7) & ~7ull) + " bytes");
        hipStream_t st = (hipStream_t)stream;
        if (translate) hip_check(translate_launch(d_seq, len, hash_function, d_aa, st), "translate");
        else hip_check(residues_launch(d_seq, len, hash_function, d_aa, st), "residues");
        // (fewer than three bases: d_aa holds the six separators and no window; k_aa is still validated)
        hip_check(residue_windows_launch(d_aa, translate && len < 3 ? 0 : n_aa, k_aa, seed, max_hash ? max_hash : ~0ull, d_out, (unsigned long long*)d_count, cap,
                                         false, st), "residue windows");
        return n_aa;
    });
}

void smgpu_synth_dna_raw(uint8_t* d_out, uint64_t start, uint64_t n, uint64_t seed, uint64_t record_len, void* stream) {
    landing_void([&] { hip_check(synth_dna_launch(d_out, start, n, seed, record_len, (hipStream_t)stream), "synth_dna"); });
}

// Page-locked host memory for large results (cached by the library's arena on release): a device-to-host copy into it runs at the
// link's rate with no staging and no page faults -- sourmash_amd/compare.py puts the n x n matrices of large collections there.
void* smgpu_host_alloc(uintptr_t bytes) {
    return landing<void*>([&]() -> void* {
        void* p = nullptr;
        hip_check(arena_pinned_alloc(&p, bytes ? bytes : 1), "pinned host allocation");
        return p;
    });
}
void smgpu_host_free(void* p) { arena_pinned_free(p); }

void smgpu_xfer_roundtrip(const void* const* pieces, const uint64_t* lens, uintptr_t n, void* out, uint64_t out_bytes) {
    landing_void([&] {
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::vector<HostPiece> ps(n);
        size_t total = 0;
        for (uintptr_t i = 0; i < n; ++i) { ps[i] = HostPiece{pieces[i], total, (size_t)lens[i]}; total += (size_t)lens[i]; }
        if (total != out_bytes) throw err_internal("smgpu_xfer_roundtrip: the pieces do not add up to out_bytes");
        AsyncBuf dev(total + 16, st);
        HostXfer::get().gather_to_device(dev.p, ps, total, st);
        HostXfer::get().device_to_host(out, dev.p, total, st);
    });
}
void smgpu_xfer_stats(uint64_t* out5, bool reset) {
    const HostXfer::Stats x = HostXfer::get().stats();
    if (out5) { out5[0] = x.h2d_bytes; out5[1] = x.d2h_bytes; out5[2] = x.h2d_ns; out5[3] = x.d2h_ns; out5[4] = x.calls; }
    if (reset) HostXfer::get().reset_stats();
}

void smgpu_arena_stats(uint64_t* out) {
    const ArenaStats a = arena_stats();
    out[0] = a.driver_allocs; out[1] = a.driver_frees; out[2] = a.driver_ns; out[3] = a.reuse_hits;
    out[4] = a.live_bytes; out[5] = a.cached_bytes; out[6] = a.peak_bytes; out[7] = a.cross_stream_waits;
}
void smgpu_arena_trim(uint64_t keep_bytes) { arena_trim(keep_bytes); }
uint64_t smgpu_gunzip_file(const char* path, uint32_t threads, uint64_t span_bytes, uint8_t* out, uint64_t cap, uint32_t* crc_out,
                           bool* parallel_used) {
    return landing<uint64_t>([&]() -> uint64_t {
        try {
            ParallelGunzip pg(path, threads, span_bytes ? (size_t)span_bytes : ((size_t)1 << 20));
            std::vector<uint8_t> buf((size_t)8 << 20);
            uint64_t total = 0;
            uint32_t crc = 0;
            for (;;) {
                const size_t n = pg.read(buf.data(), buf.size());
                if (n == 0) break;
                if (crc_out) crc = (uint32_t)crc32_z(crc, buf.data(), n);
                if (out && total < cap) memcpy(out + total, buf.data(), (size_t)std::min<uint64_t>(n, cap - total));
                total += n;
            }
            if (crc_out) *crc_out = crc;
            if (parallel_used) *parallel_used = pg.parallel();
            return total;
        } catch (const std::runtime_error& e) {
            throw Error(E_NIFFLER, e.what());
        }
    });
}
uint32_t smgpu_gunzip_position_code(uint32_t p) { return ParallelGunzip::position_code(p & 32767u); }

}  // extern "C"
