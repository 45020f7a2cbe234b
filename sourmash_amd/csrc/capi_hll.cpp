// capi_hll.cpp -- the extern "C" surface (include/sourmash_amd.h): HyperLogLog.
#include <algorithm>
#include <fstream>
#include <sstream>
#include "capi_common.hpp"
#include "hll_host.hpp"
#include "ingest.hpp"

using namespace smg;

// =============================================================================================
// HyperLogLog (ffi/hyperloglog.rs over sketch/hyperloglog/mod.rs): the host container is hll_host.hpp; k-mers reach the
// registers through hll.hip.  add_sequence queues records like the MinHash path (capi.cpp: add_sequence_dna; record_queue.hpp):
// no launch per record, since the reference's tests make 1.5 million add calls of 21 bases; every reader of the registers
// settles the queue first.  Creating, add_hash, merge, the estimators and load / save never touch the device.
// =============================================================================================
namespace {

inline HyperLogLog* HLLRAW(SourmashHyperLogLog* p) { return reinterpret_cast<HyperLogLog*>(p); }
inline HyperLogLog* HLLRAW(const SourmashHyperLogLog* p) { return reinterpret_cast<HyperLogLog*>(const_cast<SourmashHyperLogLog*>(p)); }

// Run device work on the handle's registers: upload them as u32, `work(d_regs, stream)`, pack to u8 on the device, read back.
template <class F>
void hll_on_device(HyperLogLog& h, F&& work) {
    if (h.registers.empty()) throw err_internal("HyperLogLog without registers (made by hll_new)");
    DeviceCtx& ctx = DeviceCtx::get();
    std::lock_guard<std::recursive_mutex> g(ctx.mutex());
    hipStream_t st = ctx.stream();
    const uint32_t n = (uint32_t)h.registers.size();
    std::vector<uint32_t> wide(h.registers.begin(), h.registers.end());
    AsyncBuf d_regs((size_t)n * 4, st), d_packed(n, st);
    hip_check(hipMemcpyAsync(d_regs.p, wide.data(), (size_t)n * 4, hipMemcpyHostToDevice, st), "H2D");
    work(d_regs.as<uint32_t>(), st);
    hip_check(hll_pack_launch(d_regs.as<uint32_t>(), n, d_packed.as<uint8_t>(), st), "hll_pack");
    hip_check(hipMemcpyAsync(h.registers.data(), d_packed.p, n, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
}

// HyperLogLog's rule (record_queue.hpp): the handle's lock, and the queue is consumed only once the registers hold the records.
void hll_settle(HyperLogLog& h, bool streaming = false) {
    std::lock_guard<std::recursive_mutex> sg(h.settle_mu);
    if (h.pending.empty()) return;
    std::string& q = h.pending;
    hll_on_device(h, [&](uint32_t* d_regs, hipStream_t st) {
        AsyncBuf d_seq(q.size() + 64, st);
        hip_check(hipMemcpyAsync(d_seq.p, q.data(), q.size(), hipMemcpyHostToDevice, st), "H2D");
        hip_check(hll_dna_launch(d_seq.as<uint8_t>(), q.size(), (uint32_t)h.ksize, (uint32_t)h.p, d_regs, st), "hll_dna");
        hip_check(hipStreamSynchronize(st), "sync");    // d_seq is released at the end of this scope
    });
    // If the device work throws, the queue stays and the error reaches the caller; hashing it again later is harmless (register
    // updates are max operations, so repeating one changes nothing).
    release_queue(q, streaming);
}

// Every reader settles the queue first; the emptiness test is made under the handle's lock (hll_settle), as the appends are.
inline HyperLogLog* HLL(SourmashHyperLogLog* p) {
    HyperLogLog* h = HLLRAW(p);
    if (h) hll_settle(*h);
    return h;
}
inline const HyperLogLog* HLL(const SourmashHyperLogLog* p) { return HLL(const_cast<SourmashHyperLogLog*>(p)); }

// SigsTrait::add_sequence (signature.rs:38-58) into an HLL: seed 42, hash 0 skipped; force == false raises InvalidDNA naming
// the first bad k-mer after the k-mers before it have been queued (like capi.cpp: add_sequence_dna; record_queue.hpp)
void hll_add_sequence_impl(HyperLogLog& h, const uint8_t* seq, size_t len, bool force) {
    const size_t k = h.ksize;
    if (h.registers.empty()) throw err_internal("HyperLogLog without registers (made by hll_new)");
    if (k == 0 || len < k) return;
    (void)DeviceCtx::get();
    check_dna_ksize((uint32_t)std::min<size_t>(k, UINT32_MAX));
    const ValidPrefix v = valid_prefix(seq, len, k, force);
    if (v.use_len >= k) {                                            // nothing to queue: no lock taken
        std::lock_guard<std::recursive_mutex> sg(h.settle_mu);
        if (queue_record(h.pending, seq, v.use_len, k)) hll_settle(h, true);
    }
    if (v.raise) throw err_invalid_dna(upper_ascii(seq + v.bad_kmer, k));
}

// hashes of a sketch into h: small sketches on the host, large ones through hll_hashes_kernel
void hll_add_hashes(HyperLogLog& h, const std::vector<uint64_t>& hs) {
    constexpr size_t DEVICE_FROM = (size_t)1 << 16;
    if (hs.size() < DEVICE_FROM) {
        for (uint64_t x : hs) h.add_hash(x);
        return;
    }
    hll_on_device(h, [&](uint32_t* d_regs, hipStream_t st) {
        AsyncBuf d_h(hs.size() * 8, st);
        hip_check(hipMemcpyAsync(d_h.p, hs.data(), hs.size() * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hll_hashes_launch(d_h.as<uint64_t>(), hs.size(), (uint32_t)h.p, d_regs, false, st), "hll_hashes");
        hip_check(hipStreamSynchronize(st), "sync");
    });
}

HyperLogLog hll_read_plain(const std::string& raw) {
    const std::string text = maybe_gunzip(raw.data(), raw.size());
    return HyperLogLog::parse((const uint8_t*)text.data(), text.size());
}

}  // namespace
extern "C" {

SourmashHyperLogLog* hll_new(void) { return reinterpret_cast<SourmashHyperLogLog*>(new HyperLogLog()); }
void hll_free(SourmashHyperLogLog* ptr) { delete HLLRAW(ptr); }

SourmashHyperLogLog* hll_with_error_rate(double error_rate, uintptr_t ksize) {
    return landing<SourmashHyperLogLog*>([&] {
        return reinterpret_cast<SourmashHyperLogLog*>(new HyperLogLog(HyperLogLog::make(HyperLogLog::precision_for(error_rate), ksize)));
    });
}

uintptr_t hll_ksize(const SourmashHyperLogLog* ptr) { return HLLRAW(ptr)->ksize; }

uintptr_t hll_cardinality(const SourmashHyperLogLog* ptr) {
    return landing<uintptr_t>([&] { return (uintptr_t)HLL(ptr)->cardinality(); });
}
double hll_similarity(const SourmashHyperLogLog* ptr, const SourmashHyperLogLog* optr) {
    return landing<double>([&] { return HLL(ptr)->similarity(*HLL(optr)); });
}
double hll_containment(const SourmashHyperLogLog* ptr, const SourmashHyperLogLog* optr) {
    return landing<double>([&] { return HLL(ptr)->containment(*HLL(optr)); });
}
uintptr_t hll_intersection_size(const SourmashHyperLogLog* ptr, const SourmashHyperLogLog* optr) {
    return landing<uintptr_t>([&] { return (uintptr_t)HLL(ptr)->intersection(*HLL(optr)); });
}

void hll_add_sequence(SourmashHyperLogLog* ptr, const char* sequence, uintptr_t insize, bool force) {
    landing_void([&] {
        if (!sequence && insize) throw err_internal("null sequence");
        hll_add_sequence_impl(*HLLRAW(ptr), (const uint8_t*)sequence, insize, force);
    });
}
void hll_add_hash(SourmashHyperLogLog* ptr, uint64_t hash) {
    landing_void([&] { HLLRAW(ptr)->add_hash(hash); });
}

void hll_merge(SourmashHyperLogLog* ptr, const SourmashHyperLogLog* optr) {
    landing_void([&] {
        HyperLogLog* a = HLL(ptr);
        const HyperLogLog* b = HLL(optr);
        if (a == b) return;
        std::lock_guard<std::recursive_mutex> sg(a->settle_mu);
        a->merge(*b);
    });
}

void hll_update_mh(SourmashHyperLogLog* ptr, const SourmashKmerMinHash* optr) {
    landing_void([&] {
        HyperLogLog* h = HLL(ptr);
        const KmerMinHash* mh = MH(optr);
        if (h->registers.empty()) throw err_internal("HyperLogLog without registers (made by hll_new)");
        std::lock_guard<std::recursive_mutex> sg(h->settle_mu);
        hll_add_hashes(*h, mh->mins);
    });
}

// KmerMinHash::as_hll (minhash.rs:759-767): the sketch's hashes in a fresh HLL at error rate 0.01, then `intersection`
uintptr_t hll_matches(const SourmashHyperLogLog* ptr, const SourmashKmerMinHash* mh_ptr) {
    return landing<uintptr_t>([&] {
        const HyperLogLog* h = HLL(ptr);
        const KmerMinHash* mh = MH(mh_ptr);
        HyperLogLog other = HyperLogLog::make(HyperLogLog::precision_for(0.01), mh->ksize);
        hll_add_hashes(other, mh->mins);
        return (uintptr_t)h->intersection(other);
    });
}

SourmashHyperLogLog* hll_from_path(const char* filename) {
    return landing<SourmashHyperLogLog*>([&]() -> SourmashHyperLogLog* {
        if (!filename) throw err_internal("null filename");
        std::ifstream f(filename, std::ios::binary);
        if (!f) throw Error(E_IO, std::string("No such file or directory: ") + filename);
        std::stringstream ss;
        ss << f.rdbuf();
        return reinterpret_cast<SourmashHyperLogLog*>(new HyperLogLog(hll_read_plain(ss.str())));
    });
}

SourmashHyperLogLog* hll_from_buffer(const char* ptr, uintptr_t insize) {
    return landing<SourmashHyperLogLog*>([&]() -> SourmashHyperLogLog* {
        if (!ptr && insize) throw err_internal("null buffer");
        return reinterpret_cast<SourmashHyperLogLog*>(new HyperLogLog(hll_read_plain(std::string(ptr ? ptr : "", insize))));
    });
}

void hll_save(const SourmashHyperLogLog* ptr, const char* filename) {
    landing_void([&] {
        if (!filename) throw err_internal("null filename");
        const std::string s = HLL(ptr)->serialize();
        std::ofstream f(filename, std::ios::binary | std::ios::trunc);
        if (!f) throw Error(E_IO, std::string("cannot create ") + filename);
        f.write(s.data(), (std::streamsize)s.size());
        if (!f) throw Error(E_IO, std::string("cannot write ") + filename);
    });
}

// gzip (level 1) of the file layout, as ffi/hyperloglog.rs writes it; freed with nodegraph_buffer_free
const uint8_t* hll_to_buffer(const SourmashHyperLogLog* ptr, uintptr_t* size) {
    return landing<const uint8_t*>([&]() -> const uint8_t* {
        const std::string s = gzip_bytes(HLL(ptr)->serialize(), 1);
        uint8_t* out = (uint8_t*)malloc(s.size() ? s.size() : 1);
        memcpy(out, s.data(), s.size());
        *size = s.size();
        return out;
    });
}

// ---- HyperLogLog extensions ----
void smgpu_hll_flush(SourmashHyperLogLog* ptr) {
    landing_void([&] { HLL(ptr); });
}

const uint8_t* smgpu_hll_registers(const SourmashHyperLogLog* ptr, uintptr_t* size) {
    return landing<const uint8_t*>([&]() -> const uint8_t* {
        const HyperLogLog* h = HLL(ptr);
        *size = h->registers.size();
        return h->registers.data();
    });
}

uint64_t smgpu_hll_add_file(SourmashHyperLogLog* ptr, const char* path, uint64_t* n_records) {
    uint64_t bases = 0;
    landing_void([&] {
        if (!path) throw err_internal("null path");
        HyperLogLog* h = HLL(ptr);
        std::lock_guard<std::recursive_mutex> sg(h->settle_mu);
        if (h->ksize == 0) return;
        check_dna_ksize((uint32_t)std::min<size_t>(h->ksize, UINT32_MAX));
        uint64_t recs = 0;
        hll_on_device(*h, [&](uint32_t* d_regs, hipStream_t) {
            std::vector<KmerMinHash*> none;
            const std::vector<HllSink> sinks{HllSink{(uint32_t)h->ksize, (uint32_t)h->p, d_regs}};
            sketch_file_into(none, path, &recs, &bases, &sinks);
        });
        if (n_records) *n_records = recs;
    });
    return bases;
}

void smgpu_hll_add_device(SourmashHyperLogLog* ptr, const uint8_t* d_seq, uint64_t len, void* stream) {
    landing_void([&] {
        HyperLogLog* h = HLL(ptr);
        std::lock_guard<std::recursive_mutex> sg(h->settle_mu);
        if (h->ksize == 0 || len < h->ksize) return;
        check_dna_ksize((uint32_t)std::min<size_t>(h->ksize, UINT32_MAX));
        hll_on_device(*h, [&](uint32_t* d_regs, hipStream_t st) {
            hipStream_t src = (hipStream_t)stream;
            if (src != st) hip_check(hipStreamSynchronize(src), "sync");   // the caller's writes of d_seq are complete
            hip_check(hll_dna_launch(d_seq, len, (uint32_t)h->ksize, (uint32_t)h->p, d_regs, st), "hll_dna");
        });
    });
}

void smgpu_hll_dna_raw(const uint8_t* d_seq, uint64_t len, uint32_t ksize, uint32_t p, uint32_t* d_regs, void* stream) {
    landing_void([&] {
        if (p < 4 || p > 18) throw Error(E_HLL_PRECISION_BOUNDS, "HLL precision must be between 4 and 18");
        check_dna_ksize(ksize);
        hip_check(hll_dna_launch(d_seq, len, ksize, p, d_regs, (hipStream_t)stream), "hll_dna");
    });
}

uint32_t smgpu_hll_precision(const SourmashHyperLogLog* ptr) { return (uint32_t)HLLRAW(ptr)->p; }

}  // extern "C"
