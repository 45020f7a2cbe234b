// capi_nodegraph.cpp -- the extern "C" surface (include/sourmash_amd.h): Nodegraph.
#include <algorithm>
#include <fstream>
#include <memory>
#include <sstream>
#include "capi_common.hpp"
#include "ingest.hpp"
#include "nodegraph_host.hpp"

using namespace smg;

// =============================================================================================
// Nodegraph (ffi/nodegraph.rs over sketch/nodegraph.rs): the host container is nodegraph_host.hpp; k-mers and large hash lists
// reach the tables through nodegraph.hip.  The handle keeps a device mirror of the tables tagged with the host copy's content
// generation: a bulk call uploads the tables only when the host copy changed since the last upload, runs its kernel and leaves
// the result on the device; the first host read after that downloads the tables and adds the device's count of table-0 bits
// turned on to `occupied`.  A run of bulk calls therefore costs one upload and one download.  add_sequence queues records as
// the HLL path does.  Creating, count / get of single hashes, update, load / save never touch the device on their own.
// =============================================================================================
namespace {

struct NgHandle {
    Nodegraph g;
    DevBuf d_words, d_tabs, d_occ;      // the device mirror (arena blocks)
    std::vector<NgTable> tabs;          // its table descriptors, as uploaded
    uint64_t dev_gen = ~0ull;           // the host generation the mirror holds (~0: none)
    bool host_stale = false;            // the mirror holds bits (and an occupied delta) the host copy does not
};

inline NgHandle* NGRAW(SourmashNodegraph* p) { return reinterpret_cast<NgHandle*>(p); }
inline NgHandle* NGRAW(const SourmashNodegraph* p) { return reinterpret_cast<NgHandle*>(const_cast<SourmashNodegraph*>(p)); }

// the mirror, current: uploads the tables when the host copy changed since the last upload.  Context lock held by the caller.
NgDev ng_mirror(NgHandle& h, hipStream_t st) {
    Nodegraph& g = h.g;
    if (h.dev_gen != g.gen) {
        if (h.host_stale) throw err_internal("nodegraph mirror out of step");
        h.tabs.clear();
        for (size_t t = 0; t < g.n_tables(); ++t) {
            g.check_size(t);
            if (g.sizes[t] >> 63) throw Error(E_MSG, "Nodegraph tables of 2^63 bits and more are not supported on the GPU");
            h.tabs.push_back(NgTable{g.sizes[t], ng_magic(g.sizes[t]), g.offs[t]});
        }
        const size_t nw = g.words.size();
        h.d_words.reserve(std::max<size_t>(nw, 1) * 4, st);
        h.d_tabs.reserve(std::max<size_t>(h.tabs.size(), 1) * sizeof(NgTable), st);
        h.d_occ.reserve(8, st);
        if (nw) hip_check(hipMemcpyAsync(h.d_words.p, g.words.data(), nw * 4, hipMemcpyHostToDevice, st), "H2D");
        if (!h.tabs.empty())
            hip_check(hipMemcpyAsync(h.d_tabs.p, h.tabs.data(), h.tabs.size() * sizeof(NgTable), hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipMemsetAsync(h.d_occ.p, 0, 8, st), "memset");
        hip_check(hipStreamSynchronize(st), "sync");
        h.dev_gen = g.gen;
    }
    NgDev d;
    d.tabs = h.d_tabs.as<NgTable>();
    d.n_tables = (uint32_t)g.n_tables();
    d.words = h.d_words.as<uint32_t>();
    d.n_words = g.words.size();
    d.t0_words = g.n_tables() ? Nodegraph::n_words(g.sizes[0]) : 0;
    d.occ = h.d_occ.as<unsigned long long>();
    return d;
}

// Device work on the mirror, `work(dev, stream)`, then a synchronisation.  writes: the work sets bits (the host copy is stale
// from here on); otherwise it only reads them.
template <class F>
void ng_on_device(NgHandle& h, bool writes, F&& work) {
    if (h.g.n_tables() > UINT32_MAX) throw err_internal("too many Nodegraph tables");
    DeviceCtx& ctx = DeviceCtx::get();
    std::lock_guard<std::recursive_mutex> g(ctx.mutex());
    hipStream_t st = ctx.stream();
    const NgDev d = ng_mirror(h, st);
    if (writes) h.host_stale = true;    // (a failed launch may have set some bits: they and their count are read back alike)
    work(d, st);
    hip_check(hipStreamSynchronize(st), "sync");
}

// Nodegraph's rule (record_queue.hpp): the handle's lock.  Hash the queued records into the mirror; consumed only once the tables
// hold them: if the device work throws, the queue stays and the error reaches the caller; counting it again later is harmless
// (bits only turn on, and a bit already on is not counted again).
void ng_settle(NgHandle& h, bool streaming = false) {
    Nodegraph& g = h.g;
    std::lock_guard<std::recursive_mutex> sg(g.settle_mu);
    if (g.pending.empty()) return;
    std::string& q = g.pending;
    ng_on_device(h, true, [&](const NgDev& d, hipStream_t st) {
        AsyncBuf d_seq(q.size() + 64, st);
        hip_check(hipMemcpyAsync(d_seq.p, q.data(), q.size(), hipMemcpyHostToDevice, st), "H2D");
        hip_check(nodegraph_dna_launch(d_seq.as<uint8_t>(), q.size(), (uint32_t)g.ksize, d, st), "nodegraph_dna");
        hip_check(hipStreamSynchronize(st), "sync");    // d_seq is released at the end of this scope
    });
    release_queue(q, streaming);
}

// The host copy, current: queued records counted, device bits and the occupied delta read back.  Every host read and every
// host change goes through here first (under the handle's lock).
Nodegraph& ng_host(NgHandle& h) {
    ng_settle(h);
    if (!h.host_stale) return h.g;
    Nodegraph& g = h.g;
    DeviceCtx& ctx = DeviceCtx::get();
    std::lock_guard<std::recursive_mutex> lk(ctx.mutex());
    hipStream_t st = ctx.stream();
    unsigned long long delta = 0;
    if (!g.words.empty())
        hip_check(hipMemcpyAsync(g.words.data(), h.d_words.p, g.words.size() * 4, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipMemcpyAsync(&delta, h.d_occ.p, 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipMemsetAsync(h.d_occ.p, 0, 8, st), "memset");
    hip_check(hipStreamSynchronize(st), "sync");
    g.occupied += delta;
    h.host_stale = false;               // the mirror equals the host copy again (same generation)
    return g;
}

// k-mers reach the tables only through the kernel: k = 1 .. 32
void ng_check_bulk_k(const Nodegraph& g) {
    if (g.ksize == 0 || g.ksize > NG_MAX_K)
        throw Error(E_MISMATCH_KSIZES, "Nodegraph k-mer input takes ksize 1 .. 32 (khmer's limit); this graph has ksize " +
                                           std::to_string(g.ksize));
}

// add_sequence into the queue: force == false raises InvalidDNA naming the first bad k-mer after the k-mers before it were
// queued (hll_add_sequence_impl's rule); force == true leaves bad k-mers to the kernel, which skips them
void ng_add_sequence_impl(NgHandle& h, const uint8_t* seq, size_t len, bool force) {
    Nodegraph& g = h.g;
    ng_check_bulk_k(g);
    const size_t k = g.ksize;
    if (len < k) return;
    (void)DeviceCtx::get();
    const ValidPrefix v = valid_prefix(seq, len, k, force);
    if (v.use_len >= k) {                                            // nothing to queue: no lock taken
        std::lock_guard<std::recursive_mutex> sg(g.settle_mu);
        if (queue_record(g.pending, seq, v.use_len, k)) ng_settle(h, true);
    }
    if (v.raise) throw err_invalid_dna(upper_ascii(seq + v.bad_kmer, k));
}

constexpr size_t NG_DEVICE_FROM = (size_t)1 << 16;   // sketches of this many hashes and more go through the hash kernels

// Update<Nodegraph> for KmerMinHash: count every hash (small sketches on the host, large ones through the hash kernel)
void ng_add_hashes(NgHandle& h, const std::vector<uint64_t>& hs) {
    if (hs.size() < NG_DEVICE_FROM) {
        Nodegraph& g = ng_host(h);
        for (uint64_t x : hs) g.count(x);
        return;
    }
    ng_settle(h);
    ng_on_device(h, true, [&](const NgDev& d, hipStream_t st) {
        AsyncBuf d_h(hs.size() * 8, st);
        hip_check(hipMemcpyAsync(d_h.p, hs.data(), hs.size() * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(nodegraph_hashes_launch(d_h.as<uint64_t>(), hs.size(), d, st), "nodegraph_hashes");
        hip_check(hipStreamSynchronize(st), "sync");
    });
}

uint64_t ng_matches_hashes(NgHandle& h, const std::vector<uint64_t>& hs) {
    if (hs.size() < NG_DEVICE_FROM) {
        const Nodegraph& g = ng_host(h);
        uint64_t n = 0;
        for (uint64_t x : hs) n += g.get(x);
        return n;
    }
    ng_settle(h);
    uint64_t n = 0;
    ng_on_device(h, false, [&](const NgDev& d, hipStream_t st) {
        const uint64_t off[2] = {0, (uint64_t)hs.size()};
        AsyncBuf d_h(hs.size() * 8 + 16, st), d_out(8, st);
        uint64_t* d_off = d_h.as<uint64_t>() + hs.size();
        hip_check(hipMemcpyAsync(d_h.p, hs.data(), hs.size() * 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipMemcpyAsync(d_off, off, 16, hipMemcpyHostToDevice, st), "H2D");
        hip_check(nodegraph_matches_launch(d_h.as<uint64_t>(), d_off, 1, d, d_out.as<uint64_t>(), st), "nodegraph_matches");
        hip_check(hipMemcpyAsync(&n, d_out.p, 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
    });
    return n;
}

NgHandle* ng_read_plain(const std::string& raw) {
    const std::string text = maybe_gunzip(raw.data(), raw.size());
    std::unique_ptr<NgHandle> h(new NgHandle());
    h->g.parse((const uint8_t*)text.data(), text.size());
    return h.release();
}

}  // namespace
extern "C" {

SourmashNodegraph* nodegraph_new(void) { return reinterpret_cast<SourmashNodegraph*>(new NgHandle()); }
void nodegraph_free(SourmashNodegraph* ptr) { delete NGRAW(ptr); }

SourmashNodegraph* nodegraph_with_tables(uintptr_t ksize, uintptr_t starting_size, uintptr_t n_tables) {
    return landing<SourmashNodegraph*>([&]() -> SourmashNodegraph* {
        std::unique_ptr<NgHandle> h(new NgHandle());
        h->g.with_tables(ksize, starting_size, n_tables);
        return reinterpret_cast<SourmashNodegraph*>(h.release());
    });
}

bool nodegraph_count(SourmashNodegraph* ptr, uint64_t h) {
    return landing<bool>([&] {
        NgHandle* n = NGRAW(ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        return ng_host(*n).count(h);
    });
}
bool nodegraph_count_kmer(SourmashNodegraph* ptr, const char* kmer) {
    return landing<bool>([&] {
        if (!kmer) throw err_internal("null k-mer");
        const uint64_t hv = ng_twobit_hash((const uint8_t*)kmer, strlen(kmer));
        NgHandle* n = NGRAW(ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        return ng_host(*n).count(hv);
    });
}
uintptr_t nodegraph_get(const SourmashNodegraph* ptr, uint64_t h) {
    return landing<uintptr_t>([&] {
        NgHandle* n = NGRAW(ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        return (uintptr_t)ng_host(*n).get(h);
    });
}
uintptr_t nodegraph_get_kmer(const SourmashNodegraph* ptr, const char* kmer) {
    return landing<uintptr_t>([&] {
        if (!kmer) throw err_internal("null k-mer");
        const uint64_t hv = ng_twobit_hash((const uint8_t*)kmer, strlen(kmer));
        NgHandle* n = NGRAW(ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        return (uintptr_t)ng_host(*n).get(hv);
    });
}

double nodegraph_expected_collisions(const SourmashNodegraph* ptr) {
    return landing<double>([&] {
        NgHandle* n = NGRAW(ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        return ng_host(*n).expected_collisions();
    });
}
uintptr_t nodegraph_ksize(const SourmashNodegraph* ptr) { return NGRAW(ptr)->g.ksize; }
uintptr_t nodegraph_ntables(const SourmashNodegraph* ptr) { return NGRAW(ptr)->g.n_tables(); }
uintptr_t nodegraph_noccupied(const SourmashNodegraph* ptr) {
    return landing<uintptr_t>([&] {
        NgHandle* n = NGRAW(ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        return (uintptr_t)ng_host(*n).occupied;
    });
}
// freed with kmerminhash_slice_free (the reference's Python does so)
const uint64_t* nodegraph_hashsizes(const SourmashNodegraph* ptr, uintptr_t* size) {
    const std::vector<uint64_t>& s = NGRAW(ptr)->g.sizes;
    uint64_t* out = (uint64_t*)malloc(s.empty() ? 8 : s.size() * 8);
    if (!s.empty()) memcpy(out, s.data(), s.size() * 8);
    *size = s.size();
    return out;
}

uintptr_t nodegraph_matches(const SourmashNodegraph* ptr, const SourmashKmerMinHash* mh_ptr) {
    return landing<uintptr_t>([&] {
        NgHandle* n = NGRAW(ptr);
        const KmerMinHash* mh = MH(mh_ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        return (uintptr_t)ng_matches_hashes(*n, mh->mins);
    });
}

void nodegraph_update(SourmashNodegraph* ptr, const SourmashNodegraph* optr) {
    landing_void([&] {
        NgHandle* a = NGRAW(ptr);
        NgHandle* b = NGRAW(optr);
        std::lock_guard<std::recursive_mutex> sa(a->g.settle_mu);
        std::lock_guard<std::recursive_mutex> sb(b->g.settle_mu);
        const Nodegraph& other = ng_host(*b);
        ng_host(*a).update(other);
    });
}
void nodegraph_update_mh(SourmashNodegraph* ptr, const SourmashKmerMinHash* optr) {
    landing_void([&] {
        NgHandle* n = NGRAW(ptr);
        const KmerMinHash* mh = MH(optr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        ng_add_hashes(*n, mh->mins);
    });
}

SourmashNodegraph* nodegraph_from_path(const char* filename) {
    return landing<SourmashNodegraph*>([&]() -> SourmashNodegraph* {
        if (!filename) throw err_internal("null filename");
        std::ifstream f(filename, std::ios::binary);
        if (!f) throw Error(E_IO, std::string("No such file or directory: ") + filename);
        std::stringstream ss;
        ss << f.rdbuf();
        return reinterpret_cast<SourmashNodegraph*>(ng_read_plain(ss.str()));
    });
}
SourmashNodegraph* nodegraph_from_buffer(const char* ptr, uintptr_t insize) {
    return landing<SourmashNodegraph*>([&]() -> SourmashNodegraph* {
        if (!ptr && insize) throw err_internal("null buffer");
        return reinterpret_cast<SourmashNodegraph*>(ng_read_plain(std::string(ptr ? ptr : "", insize)));
    });
}

// always the plain layout (nodegraph.rs `save`)
void nodegraph_save(const SourmashNodegraph* ptr, const char* filename) {
    landing_void([&] {
        if (!filename) throw err_internal("null filename");
        NgHandle* n = NGRAW(ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        const std::string s = ng_host(*n).serialize();
        std::ofstream f(filename, std::ios::binary | std::ios::trunc);
        if (!f) throw Error(E_IO, std::string("cannot create ") + filename);
        f.write(s.data(), (std::streamsize)s.size());
        if (!f) throw Error(E_IO, std::string("cannot write ") + filename);
    });
}

// compression 0: the plain layout; 1 .. 9: gzip at that level (above 9: 9).  Freed with nodegraph_buffer_free.
const uint8_t* nodegraph_to_buffer(const SourmashNodegraph* ptr, uint8_t compression, uintptr_t* size) {
    return landing<const uint8_t*>([&]() -> const uint8_t* {
        NgHandle* n = NGRAW(ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        std::string s = ng_host(*n).serialize();
        if (compression > 0) s = gzip_bytes(s, compression > 9 ? 9 : compression);
        uint8_t* out = (uint8_t*)malloc(s.size() ? s.size() : 1);
        if (!out) throw std::bad_alloc();
        memcpy(out, s.data(), s.size());
        *size = s.size();
        return out;
    });
}

// ---- Nodegraph extensions ----
void smgpu_nodegraph_add_sequence(SourmashNodegraph* ptr, const char* sequence, uintptr_t insize, bool force) {
    landing_void([&] {
        if (!sequence && insize) throw err_internal("null sequence");
        ng_add_sequence_impl(*NGRAW(ptr), (const uint8_t*)sequence, insize, force);
    });
}

void smgpu_nodegraph_flush(SourmashNodegraph* ptr) {
    landing_void([&] { ng_settle(*NGRAW(ptr)); });
}

uint64_t smgpu_nodegraph_add_file(SourmashNodegraph* ptr, const char* path, uint64_t* n_records) {
    uint64_t bases = 0;
    landing_void([&] {
        if (!path) throw err_internal("null path");
        NgHandle* n = NGRAW(ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        ng_check_bulk_k(n->g);
        ng_settle(*n);
        uint64_t recs = 0;
        ng_on_device(*n, true, [&](const NgDev& d, hipStream_t) {
            std::vector<KmerMinHash*> none;
            const std::vector<NgSink> sinks{NgSink{(uint32_t)n->g.ksize, d}};
            sketch_file_into(none, path, &recs, &bases, nullptr, &sinks);
        });
        if (n_records) *n_records = recs;
    });
    return bases;
}

void smgpu_nodegraph_add_device(SourmashNodegraph* ptr, const uint8_t* d_seq, uint64_t len, void* stream) {
    landing_void([&] {
        NgHandle* n = NGRAW(ptr);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        ng_check_bulk_k(n->g);
        if (len < n->g.ksize) return;
        ng_settle(*n);
        ng_on_device(*n, true, [&](const NgDev& d, hipStream_t st) {
            hipStream_t src = (hipStream_t)stream;
            if (src != st) hip_check(hipStreamSynchronize(src), "sync");   // the caller's writes of d_seq are complete
            hip_check(nodegraph_dna_launch(d_seq, len, (uint32_t)n->g.ksize, d, st), "nodegraph_dna");
        });
    });
}

// every hash of every row of a SketchSet, in one launch over the resident CSR
void smgpu_nodegraph_update_sketchset(SourmashNodegraph* ptr, const SmgpuSketchSet* set) {
    landing_void([&] {
        NgHandle* n = NGRAW(ptr);
        const SketchSet* s = reinterpret_cast<const SketchSet*>(set);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        if (s->total == 0) return;
        ng_settle(*n);
        ng_on_device(*n, true, [&](const NgDev& d, hipStream_t st) {
            hip_check(nodegraph_hashes_launch(s->hashes.as<uint64_t>(), s->total, d, st), "nodegraph_hashes");
        });
    });
}

// out[r] = nodegraph_matches of row r, for every row of a SketchSet (one read-only launch)
void smgpu_nodegraph_matches_sketchset(const SourmashNodegraph* ptr, const SmgpuSketchSet* set, uint64_t* out) {
    landing_void([&] {
        NgHandle* n = NGRAW(ptr);
        const SketchSet* s = reinterpret_cast<const SketchSet*>(set);
        std::lock_guard<std::recursive_mutex> sg(n->g.settle_mu);
        if (s->n == 0) return;
        if (!out) throw err_internal("null output");
        ng_settle(*n);
        ng_on_device(*n, false, [&](const NgDev& d, hipStream_t st) {
            AsyncBuf d_out(s->n * 8, st);
            hip_check(nodegraph_matches_launch(s->hashes.as<uint64_t>(), s->offsets.as<uint64_t>(), s->n, d, d_out.as<uint64_t>(), st),
                      "nodegraph_matches");
            hip_check(hipMemcpyAsync(out, d_out.p, s->n * 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
        });
    });
}

double smgpu_nodegraph_similarity(const SourmashNodegraph* ptr, const SourmashNodegraph* optr) {
    return landing<double>([&] {
        NgHandle* a = NGRAW(ptr);
        NgHandle* b = NGRAW(optr);
        std::lock_guard<std::recursive_mutex> sa(a->g.settle_mu);
        std::lock_guard<std::recursive_mutex> sb(b->g.settle_mu);
        const Nodegraph& other = ng_host(*b);
        return ng_host(*a).similarity(other);
    });
}
double smgpu_nodegraph_containment(const SourmashNodegraph* ptr, const SourmashNodegraph* optr) {
    return landing<double>([&] {
        NgHandle* a = NGRAW(ptr);
        NgHandle* b = NGRAW(optr);
        std::lock_guard<std::recursive_mutex> sa(a->g.settle_mu);
        std::lock_guard<std::recursive_mutex> sb(b->g.settle_mu);
        const Nodegraph& other = ng_host(*b);
        return ng_host(*a).containment(other);
    });
}

uintptr_t smgpu_nodegraph_table_sizes(uintptr_t starting_size, uintptr_t n_tables, uint64_t* out, uintptr_t cap) {
    return landing<uintptr_t>([&] {
        const std::vector<uint64_t> s = ng_table_sizes(starting_size, n_tables);
        for (size_t i = 0; i < s.size() && i < cap; ++i) out[i] = s[i];
        return (uintptr_t)s.size();
    });
}

}  // extern "C"
