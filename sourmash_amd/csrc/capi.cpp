// capi.cpp -- the extern "C" surface of libsourmash_amd.so (include/sourmash_amd.h): the reference's FFI.
//
// Part 1 re-implements the hot-path subset of the reference's FFI shims
// (src/core/src/ffi/{utils,mod,minhash,signature,cmd/compute}.rs) on top of the
// host containers (minhash_host.hpp, signature_host.hpp) and the HIP kernels
// (DeviceCtx / device_api.hpp).  Part 2 keeps the smgpu_* entries of the per-record MinHash path (add_sequence_dna) only.
// Every other family is a unit of its own: capi_ingest.cpp, capi_compare.cpp, capi_sketchset.cpp, capi_records.cpp, capi_gather.cpp,
// capi_hll.cpp, capi_nodegraph.cpp.  capi_common.hpp is what the units share, record_queue.hpp the deferred-record queue of all
// three add_sequence families.
#include <hip/hip_runtime_api.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <fstream>
#include <sstream>
#include "capi_common.hpp"
#include "murmur3.hpp"
#include "residues.hpp"

using namespace smg;

namespace {

// ---- deferred sketching behind the per-record API (record_queue.hpp) ---------------------------------------------
// The DNA add_sequence path (signature.rs:38-58 + :246-306) on the GPU.
// force == false: the walk is streaming in the reference, so the hashes of every
// k-mer before the first offending one are added before InvalidDNA is raised.
// protein / dayhoff / hp sketches: residues (is_protein) or DNA translated in six frames; no validity test in
// either mode (signature.rs:307-393), so `force` plays no role
void add_residue_kmers(KmerMinHash& mh, const uint8_t* seq, size_t len, bool is_protein) {
    if (mh.num == 0 && mh.max_hash == 0) return;
    if (mh.ksize / 3 == 0 || len < mh.ksize / 3) return;
    if (mh.is_dna())                                                // signature.rs:367-384: no alphabet to map to
        throw Error(E_INVALID_HASH_FUNCTION, "Invalid hash function: \"DNA\"");
    DeviceCtx& ctx = DeviceCtx::get();
    std::lock_guard<std::recursive_mutex> g(ctx.mutex());
    std::vector<uint64_t> hs, cs;
    ctx.protein_sketch_host(seq, len, mh.ksize, mh.hash_function, mh.seed, is_protein, keep_threshold(mh),
                            mh.track_abundance, mh.num, hs, cs);
    mh.add_sorted_batch(hs.data(), mh.track_abundance ? cs.data() : nullptr, hs.size());
}

}  // namespace

// MinHash's rule: ONE process-wide lock for settling, none for appending, and the queue is consumed whatever the device work does.
void smg::settle(KmerMinHash& mh, bool streaming) {
    // Accessors that only read (get_mins, md5sum, similarity ...) come through here too, possibly from two threads on
    // the same sketch (ctypes releases the GIL): one of them hashes the queue, the other finds it empty afterwards.
    static std::recursive_mutex settle_mu;
    std::lock_guard<std::recursive_mutex> sg(settle_mu);
    if (mh.pending.empty()) return;
    // whatever happens below, the records are consumed once: adding their hashes a second time would count them twice
    struct Consume {
        std::string& q;
        bool keep;
        ~Consume() { release_queue(q, keep); }
    } consume{mh.pending, streaming};
    DeviceCtx& ctx = DeviceCtx::get();
    std::lock_guard<std::recursive_mutex> g(ctx.mutex());
    std::vector<uint64_t> hs, cs;
    ctx.sketch_host((const uint8_t*)mh.pending.data(), mh.pending.size(), mh.ksize, mh.seed, keep_threshold(mh), mh.track_abundance,
                    mh.num, hs, cs);
    mh.add_sorted_batch(hs.data(), mh.track_abundance ? cs.data() : nullptr, hs.size());
}

namespace {

// The DNA add_sequence path (signature.rs:38-58 + :246-306).
// force == false: the walk is streaming in the reference, so the hashes of every k-mer before the first offending
// one are added before InvalidDNA is raised: the valid prefix is queued, then the error is raised from this call.
// `scanned`: the caller has run first_invalid_byte over seq[0, len) already and passes its result in `first_bad`
void add_sequence_dna(KmerMinHash& mh, const uint8_t* seq, size_t len, bool force, bool scanned = false, size_t first_bad = SIZE_MAX) {
    if (!mh.is_dna()) { add_residue_kmers(mh, seq, len, false); return; }
    const uint32_t k = mh.ksize;
    if (len < k || k == 0) return;                                  // signature.rs:206-210
    if (mh.num == 0 && mh.max_hash == 0) return;                    // sketch that can never hold anything
    (void)DeviceCtx::get();                                         // no device: fail now, not at the first accessor
    check_dna_ksize(k);
    const ValidPrefix v = valid_prefix(seq, len, k, force, scanned, first_bad);
    if (queue_record(mh.pending, seq, v.use_len, k)) settle(mh, true);
    if (v.raise) throw err_invalid_dna(upper_ascii(seq + v.bad_kmer, k));   // errors.rs:49-50
}

struct Downsampled {
    const KmerMinHash* a;
    const KmerMinHash* b;
    KmerMinHash tmp;
};
// minhash.rs:540-548 / 688-696: the finer sketch is downsampled to the coarser scaled
void align_scaled(const KmerMinHash& x, const KmerMinHash& y, bool downsample, Downsampled& d) {
    d.a = &x; d.b = &y;
    if (downsample && x.scaled() != y.scaled()) {
        if (x.scaled() > y.scaled()) { d.tmp = y.downsample_scaled(x.scaled()); d.b = &d.tmp; }
        else { d.tmp = x.downsample_scaled(y.scaled()); d.a = &d.tmp; }
    }
}

PairStats device_pair(const KmerMinHash& a, const KmerMinHash& b, bool want_abund, bool want_list, uint64_t num,
                      std::vector<uint64_t>* list) {
    DeviceCtx& ctx = DeviceCtx::get();
    std::lock_guard<std::recursive_mutex> g(ctx.mutex());
    return ctx.pair(a, b, want_abund, want_list, num, list);
}

// minhash.rs:593-621 -> (common, union)
std::pair<uint64_t, uint64_t> intersection_size(const KmerMinHash& a, const KmerMinHash& b) {
    a.check_compatible(b);
    if (a.num != 0) {
        const PairStats st = device_pair(a, b, false, false, a.num, nullptr);
        const uint64_t uni_all = a.size() + b.size() - st.common;
        return {st.common_num, uni_all < a.num ? uni_all : a.num};
    }
    const PairStats st = device_pair(a, b, false, false, 0, nullptr);
    return {st.common, a.size() + b.size() - st.common};
}

double jaccard(const KmerMinHash& a, const KmerMinHash& b) {      // minhash.rs:624-631
    const auto cu = intersection_size(a, b);
    return (double)cu.first / (double)(cu.second > 1 ? cu.second : 1);
}

double angular(const KmerMinHash& a, const KmerMinHash& b) {      // minhash.rs:635-680
    a.check_compatible(b);
    if (!a.track_abundance || !b.track_abundance) throw err_needs_abundance();
    const PairStats st = device_pair(a, b, true, false, 0, nullptr);
    const double na = std::sqrt((double)st.a_sq), nb = std::sqrt((double)st.b_sq);
    if (na == 0.0 || nb == 0.0) return 0.0;
    double p = (double)st.prod / (na * nb);
    if (p > 1.0) p = 1.0;
    return 1.0 - 2.0 * std::acos(p) / 3.14159265358979323846264338327950288;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------
// library / errors
// ---------------------------------------------------------------------------------------------
void sourmash_init(void) {}
void sourmash_err_clear(void) { g_err_code = 0; g_err_msg.clear(); }
SourmashErrorCode sourmash_err_get_last_code(void) { return g_err_code; }
SourmashStr sourmash_err_get_last_message(void) {
    if (g_err_code == 0) { SourmashStr s = {nullptr, 0, false}; return s; }
    return make_str(g_err_msg);
}
SourmashStr sourmash_err_get_backtrace(void) { SourmashStr s = {nullptr, 0, false}; return s; }
void sourmash_str_free(SourmashStr* s) {
    if (s && s->owned && s->data) { free(s->data); s->data = nullptr; s->len = 0; s->owned = false; }
}
// module-level residue helpers (ffi/mod.rs; encodings.rs:299-347)
char sourmash_aa_to_dayhoff(char aa) { return (char)aa_to_dayhoff((uint8_t)aa); }
char sourmash_aa_to_hp(char aa) { return (char)aa_to_hp((uint8_t)aa); }
char sourmash_translate_codon(const char* codon) {
    return landing<char>([&]() -> char {
        const size_t n = codon ? strlen(codon) : 0;
        if (n == 1) return 'X';                                                 // encodings.rs:309-311
        if (n == 2) return (char)translate_codon(ascii_upper((uint8_t)codon[0]), ascii_upper((uint8_t)codon[1]), 'N');
        if (n == 3) return (char)translate_codon(ascii_upper((uint8_t)codon[0]), ascii_upper((uint8_t)codon[1]),
                                                 ascii_upper((uint8_t)codon[2]));
        throw Error(E_INVALID_CODON_LENGTH, std::to_string(n));
    });
}
SourmashStr sourmash_str_from_cstr(const char* s) { return make_str(s ? s : ""); }

uint64_t hash_murmur(const char* kmer, uint64_t seed) {           // ffi/mod.rs:22-31
    if (!kmer) return 0;
    return mmh3_h1_bytes((const uint8_t*)kmer, strlen(kmer), seed);
}

// ---------------------------------------------------------------------------------------------
// compute parameters (ffi/cmd/compute.rs)
// ---------------------------------------------------------------------------------------------
SourmashComputeParameters* computeparams_new(void) { return reinterpret_cast<SourmashComputeParameters*>(new ComputeParameters()); }
void computeparams_free(SourmashComputeParameters* p) { delete CP(p); }
bool computeparams_dayhoff(const SourmashComputeParameters* p) { return CP(p)->dayhoff; }
bool computeparams_dna(const SourmashComputeParameters* p) { return CP(p)->dna; }
bool computeparams_hp(const SourmashComputeParameters* p) { return CP(p)->hp; }
bool computeparams_protein(const SourmashComputeParameters* p) { return CP(p)->protein; }
bool computeparams_track_abundance(const SourmashComputeParameters* p) { return CP(p)->track_abundance; }
const uint32_t* computeparams_ksizes(const SourmashComputeParameters* p, uintptr_t* size) {
    const auto& k = CP(p)->ksizes;
    *size = k.size();
    uint32_t* out = (uint32_t*)malloc((k.size() ? k.size() : 1) * sizeof(uint32_t));
    if (k.size()) memcpy(out, k.data(), k.size() * sizeof(uint32_t));
    return out;
}
void computeparams_ksizes_free(uint32_t* ptr, uintptr_t) { free(ptr); }
uint32_t computeparams_num_hashes(const SourmashComputeParameters* p) { return CP(p)->num_hashes; }
uint64_t computeparams_scaled(const SourmashComputeParameters* p) { return CP(p)->scaled; }
uint64_t computeparams_seed(const SourmashComputeParameters* p) { return CP(p)->seed; }
void computeparams_set_dayhoff(SourmashComputeParameters* p, bool v) { CP(p)->dayhoff = v; }
void computeparams_set_dna(SourmashComputeParameters* p, bool v) { CP(p)->dna = v; }
void computeparams_set_hp(SourmashComputeParameters* p, bool v) { CP(p)->hp = v; }
void computeparams_set_protein(SourmashComputeParameters* p, bool v) { CP(p)->protein = v; }
void computeparams_set_track_abundance(SourmashComputeParameters* p, bool v) { CP(p)->track_abundance = v; }
void computeparams_set_ksizes(SourmashComputeParameters* p, const uint32_t* ks, uintptr_t n) {
    landing_void([&] { CP(p)->ksizes.assign(ks, ks + n); });
}
void computeparams_set_num_hashes(SourmashComputeParameters* p, uint32_t n) { CP(p)->num_hashes = n; }
void computeparams_set_scaled(SourmashComputeParameters* p, uint64_t s) { CP(p)->scaled = s; }
void computeparams_set_seed(SourmashComputeParameters* p, uint64_t s) { CP(p)->seed = s; }

// ---------------------------------------------------------------------------------------------
// sketch object (ffi/minhash.rs)
// ---------------------------------------------------------------------------------------------
SourmashKmerMinHash* kmerminhash_new(uint64_t scaled, uint32_t k, HashFunctions hf, uint64_t seed, bool track,
                                     uint32_t n) {
    return landing<SourmashKmerMinHash*>([&]() -> SourmashKmerMinHash* {
        return reinterpret_cast<SourmashKmerMinHash*>(new KmerMinHash(scaled, k, hf, seed, track, n));
    });
}
void kmerminhash_free(SourmashKmerMinHash* p) {
    KmerMinHash* m = RAW(p);
    if (m) {
        if (DeviceCtx* ctx = DeviceCtx::peek()) {                       // its device mirror goes with it
            if (m->mirrored_gen) {
                std::lock_guard<std::recursive_mutex> g(ctx->mutex());
                ctx->forget(*m);
            }
        }
    }
    delete m;
}
void kmerminhash_slice_free(uint64_t* ptr, uintptr_t) { free(ptr); }

void kmerminhash_add_sequence(SourmashKmerMinHash* p, const char* sequence, bool force) {
    landing_void([&] {
        if (!sequence) throw err_internal("null sequence");
        add_sequence_dna(*RAW(p), (const uint8_t*)sequence, strlen(sequence), force);   // CStr: stops at NUL (ffi/minhash.rs:53-59)
    });
}

const uint64_t* kmerminhash_seq_to_hashes(SourmashKmerMinHash* p, const char* sequence, uintptr_t insize, bool force,
                                          bool bad_kmers_as_zeroes, bool is_protein, uintptr_t* size) {
    return landing<const uint64_t*>([&]() -> const uint64_t* {
        KmerMinHash& mh = *MH(p);
        const uint8_t* seq = (const uint8_t*)sequence;
        std::vector<uint64_t> out;
        if (is_protein || !mh.is_dna()) {
            const uint32_t kr = mh.ksize / 3;
            if (kr == 0 || insize < kr || (!is_protein && insize < (uintptr_t)kr * 3)) return slice_out(out, size);
            if (mh.is_dna()) throw Error(E_INVALID_HASH_FUNCTION, "Invalid hash function: \"DNA\"");
            std::vector<uint64_t> hs;
            {
                DeviceCtx& ctx = DeviceCtx::get();
                std::lock_guard<std::recursive_mutex> g(ctx.mutex());
                ctx.protein_hashes_host(seq, insize, mh.ksize, mh.hash_function, mh.seed, is_protein, hs);
            }
            const bool zeros = force && bad_kmers_as_zeroes;
            // the translate iterator brackets its buffer with two Ok(0) markers (signature.rs:330-348), which only
            // the keep-zeroes mode lets through (ffi/minhash.rs:76-84)
            if (zeros && !is_protein) out.push_back(0);
            for (uint64_t h : hs) if (h != 0 || zeros) out.push_back(h);
            if (zeros && !is_protein) out.push_back(0);
            return slice_out(out, size);
        }
        const uint32_t k = mh.ksize;
        if (insize >= k && k != 0) {
            DeviceCtx& ctx = DeviceCtx::get();
            std::lock_guard<std::recursive_mutex> g(ctx.mutex());
            ctx.kmer_hashes_host(seq, insize, k, mh.seed, out);       // 0 where a k-mer covers an invalid byte
            if (!force) {
                // ffi/minhash.rs:76-96: the first bad k-mer aborts with InvalidDNA
                const size_t pos = ctx.first_invalid_host(seq, insize);
                if (pos != SIZE_MAX) {
                    const size_t bad = pos + 1 >= k ? pos + 1 - k : 0;
                    if (bad < out.size()) throw err_invalid_dna(upper_ascii(seq + bad, k));
                }
            }
            if (!(force && bad_kmers_as_zeroes)) {
                size_t w = 0;
                for (uint64_t h : out) if (h != 0) out[w++] = h;
                out.resize(w);
            }
        }
        return slice_out(out, size);
    });
}

void kmerminhash_add_hash(SourmashKmerMinHash* p, uint64_t h) { RAW(p)->add_hash(h); }   // commutes with the queued records
void kmerminhash_add_hash_with_abundance(SourmashKmerMinHash* p, uint64_t h, uint64_t a) {
    landing_void([&] { MH(p)->add_hash_with_abundance(h, a); });   // abundance 0 removes: settles the queued records first
}
void kmerminhash_add_many(SourmashKmerMinHash* p, const uint64_t* hs, uintptr_t n) {
    landing_void([&] {
        if (!hs && n) throw err_internal("null hashes pointer");
        for (uintptr_t i = 0; i < n; ++i) MH(p)->add_hash(hs[i]);
    });
}
void kmerminhash_add_from(SourmashKmerMinHash* p, const SourmashKmerMinHash* o) {
    landing_void([&] { for (uint64_t h : MH(o)->mins) MH(p)->add_hash(h); });   // minhash.rs:518-523
}
void kmerminhash_add_word(SourmashKmerMinHash* p, const char* word) {           // minhash.rs:401-404
    if (!word) return;
    landing_void([&] { RAW(p)->add_hash(mmh3_h1_bytes((const uint8_t*)word, strlen(word), RAW(p)->seed)); });
}
void kmerminhash_add_protein(SourmashKmerMinHash* p, const char* sequence) {
    landing_void([&] {
        if (!sequence) throw err_internal("null sequence");
        add_residue_kmers(*MH(p), (const uint8_t*)sequence, strlen(sequence), true);
    });
}
void kmerminhash_remove_hash(SourmashKmerMinHash* p, uint64_t h) { landing_void([&] { MH(p)->remove_hash(h); }); }
void kmerminhash_remove_many(SourmashKmerMinHash* p, const uint64_t* hs, uintptr_t n) {
    landing_void([&] {
        if (n < 16) { for (uintptr_t i = 0; i < n; ++i) MH(p)->remove_hash(hs[i]); return; }
        std::vector<uint64_t> sorted(hs, hs + n);
        std::sort(sorted.begin(), sorted.end());
        MH(p)->remove_sorted(sorted.data(), sorted.size());
    });
}
void kmerminhash_remove_from(SourmashKmerMinHash* p, const SourmashKmerMinHash* o) {
    landing_void([&] { MH(p)->remove_sorted(MH(o)->mins.data(), MH(o)->mins.size()); });
}
void kmerminhash_clear(SourmashKmerMinHash* p) { RAW(p)->clear(); }   // drops the queued records too

const uint64_t* kmerminhash_get_mins(const SourmashKmerMinHash* p, uintptr_t* size) {
    return landing<const uint64_t*>([&]() -> const uint64_t* { return slice_out(MH(p)->mins, size); });
}
uintptr_t kmerminhash_get_mins_size(const SourmashKmerMinHash* p) { return MH(p)->size(); }
const uint64_t* kmerminhash_get_abunds(SourmashKmerMinHash* p, uintptr_t* size) {
    return landing<const uint64_t*>([&]() -> const uint64_t* {
        if (!MH(p)->track_abundance) throw Error(E_PANIC, "sourmash panicked: not implemented");   // ffi/minhash.rs:248-260
        return slice_out(MH(p)->abunds, size);
    });
}
void kmerminhash_set_abundances(SourmashKmerMinHash* p, const uint64_t* hs, const uint64_t* as, uintptr_t n, bool clear) {
    landing_void([&] {                                                          // ffi/minhash.rs:269-300
        if ((!hs || !as) && n) throw err_internal("null pointer");
        std::vector<std::pair<uint64_t, uint64_t>> pairs(n);
        for (uintptr_t i = 0; i < n; ++i) pairs[i] = {hs[i], as[i]};
        std::sort(pairs.begin(), pairs.end());
        if (clear) MH(p)->clear();
        for (auto& pr : pairs) MH(p)->add_hash_with_abundance(pr.first, pr.second);
    });
}
SourmashStr kmerminhash_md5sum(const SourmashKmerMinHash* p) {
    return landing<SourmashStr>([&] { return make_str(MH(p)->md5sum()); });
}
void kmerminhash_merge(SourmashKmerMinHash* p, const SourmashKmerMinHash* o) {
    landing_void([&] { MH(p)->merge(*MH(o)); });
}
bool kmerminhash_is_compatible(const SourmashKmerMinHash* p, const SourmashKmerMinHash* o) {
    try { MH(p)->check_compatible(*MH(o)); return true; } catch (const Error&) { return false; }
}

uint64_t kmerminhash_count_common(const SourmashKmerMinHash* p, const SourmashKmerMinHash* o, bool downsample) {
    return landing<uint64_t>([&]() -> uint64_t {                                // minhash.rs:539-558
        Downsampled d;
        align_scaled(*MH(p), *MH(o), downsample, d);
        d.a->check_compatible(*d.b);
        return device_pair(*d.a, *d.b, false, false, 0, nullptr).common;
    });
}

SourmashKmerMinHash* kmerminhash_intersection(const SourmashKmerMinHash* p, const SourmashKmerMinHash* o) {
    return landing<SourmashKmerMinHash*>([&]() -> SourmashKmerMinHash* {        // ffi/minhash.rs:428-441, minhash.rs:560-589
        const KmerMinHash& a = *MH(p);
        const KmerMinHash& b = *MH(o);
        a.check_compatible(b);
        std::vector<uint64_t> list;
        device_pair(a, b, false, true, 0, &list);
        if (a.num != 0) {
            // bottom-k: keep only hashes that survive the merged-and-truncated union (minhash.rs:563-585)
            const uint64_t uni = a.size() + b.size() - list.size();
            if (uni > a.num) {
                // the num-th smallest of the union bounds the kept intersection
                KmerMinHash u = a;
                u.disable_abundance();
                KmerMinHash bb = b; bb.disable_abundance();
                u.merge(bb);
                const uint64_t cutoff = u.mins.empty() ? 0 : u.mins.back();
                while (!list.empty() && list.back() > cutoff) list.pop_back();
            }
        }
        KmerMinHash* out = new KmerMinHash(a);
        out->clear();
        for (uint64_t h : list) out->add_hash(h);
        return reinterpret_cast<SourmashKmerMinHash*>(out);
    });
}

uint64_t kmerminhash_intersection_union_size(const SourmashKmerMinHash* p, const SourmashKmerMinHash* o, uint64_t* usize) {
    return landing<uint64_t>([&]() -> uint64_t {                                // ffi/minhash.rs:443-457
        try {
            const auto cu = intersection_size(*MH(p), *MH(o));
            *usize = cu.second;
            return cu.first;
        } catch (const Error& e) {
            if (e.code >= 101 && e.code <= 104) { *usize = 0; return 0; }      // incompatible -> (0, 0), no error
            throw;
        }
    });
}

double kmerminhash_jaccard(const SourmashKmerMinHash* p, const SourmashKmerMinHash* o) {
    return landing<double>([&] { return jaccard(*MH(p), *MH(o)); });
}

double kmerminhash_similarity(const SourmashKmerMinHash* p, const SourmashKmerMinHash* o, bool ignore_abundance,
                              bool downsample) {
    return landing<double>([&]() -> double {                                    // minhash.rs:682-702
        Downsampled d;
        align_scaled(*MH(p), *MH(o), downsample, d);
        if (ignore_abundance || !d.a->track_abundance || !d.b->track_abundance) return jaccard(*d.a, *d.b);
        return angular(*d.a, *d.b);
    });
}

double kmerminhash_angular_similarity(const SourmashKmerMinHash* p, const SourmashKmerMinHash* o) {
    return landing<double>([&] { return angular(*MH(p), *MH(o)); });
}

uint32_t kmerminhash_num(const SourmashKmerMinHash* p) { return RAW(p)->num; }
uint32_t kmerminhash_ksize(const SourmashKmerMinHash* p) { return RAW(p)->ksize; }
uint64_t kmerminhash_seed(const SourmashKmerMinHash* p) { return RAW(p)->seed; }
uint64_t kmerminhash_max_hash(const SourmashKmerMinHash* p) { return RAW(p)->max_hash; }
HashFunctions kmerminhash_hash_function(const SourmashKmerMinHash* p) { return RAW(p)->hash_function; }
void kmerminhash_hash_function_set(SourmashKmerMinHash* p, HashFunctions hf) {
    landing_void([&] {
        if (hf < 1 || hf > 4) throw Error(E_INVALID_HASH_FUNCTION, "Invalid hash function: \"" + std::to_string(hf) + "\"");
        MH(p)->set_hash_function(hf);
    });
}
bool kmerminhash_is_protein(const SourmashKmerMinHash* p) { return RAW(p)->hash_function == HF_PROTEIN; }
bool kmerminhash_dayhoff(const SourmashKmerMinHash* p) { return RAW(p)->hash_function == HF_DAYHOFF; }
bool kmerminhash_hp(const SourmashKmerMinHash* p) { return RAW(p)->hash_function == HF_HP; }
bool kmerminhash_track_abundance(const SourmashKmerMinHash* p) { return RAW(p)->track_abundance; }
void kmerminhash_enable_abundance(SourmashKmerMinHash* p) { landing_void([&] { MH(p)->enable_abundance(); }); }
void kmerminhash_disable_abundance(SourmashKmerMinHash* p) { MH(p)->disable_abundance(); }

// ---------------------------------------------------------------------------------------------
// signature container (ffi/signature.rs)
// ---------------------------------------------------------------------------------------------
SourmashSignature* signature_new(void) {
    return landing<SourmashSignature*>([&]() -> SourmashSignature* { return reinterpret_cast<SourmashSignature*>(new Signature()); });
}
void signature_free(SourmashSignature* p) { delete SIGRAW(p); }
SourmashSignature* signature_from_params(const SourmashComputeParameters* p) {
    return landing<SourmashSignature*>([&]() -> SourmashSignature* {
        return reinterpret_cast<SourmashSignature*>(new Signature(Signature::from_params(*CP(p))));
    });
}
uintptr_t signature_len(const SourmashSignature* p) { return SIGRAW(const_cast<SourmashSignature*>(p))->sketches.size(); }

void signature_add_sequence(SourmashSignature* p, const char* sequence, bool force) {
    landing_void([&] {                                                          // signature.rs:661-677
        if (!sequence) throw err_internal("null sequence");
        const size_t len = strlen(sequence);
        for (auto& mh : SIGRAW(p)->sketches) add_sequence_dna(mh, (const uint8_t*)sequence, len, force);
    });
}
void signature_add_protein(SourmashSignature* p, const char* sequence) {
    landing_void([&] {                                                          // signature.rs:679-697
        if (!sequence) throw err_internal("null sequence");
        const size_t len = strlen(sequence);
        for (auto& mh : SIG(p)->sketches) add_residue_kmers(mh, (const uint8_t*)sequence, len, true);
    });
}
void signature_set_name(SourmashSignature* p, const char* name) { landing_void([&] { if (name) SIGRAW(p)->name = std::string(name); }); }
void signature_set_filename(SourmashSignature* p, const char* name) { landing_void([&] { if (name) SIGRAW(p)->filename = std::string(name); }); }
SourmashStr signature_get_name(const SourmashSignature* p) {
    return landing<SourmashStr>([&] { return make_str(SIG(p)->name ? *SIG(p)->name : std::string()); });
}
SourmashStr signature_get_filename(const SourmashSignature* p) {
    return landing<SourmashStr>([&] { return make_str(SIG(p)->filename ? *SIG(p)->filename : std::string()); });
}
SourmashStr signature_get_license(const SourmashSignature* p) {
    return landing<SourmashStr>([&] { return make_str(SIG(p)->license); });
}
SourmashKmerMinHash* signature_first_mh(const SourmashSignature* p) {
    return landing<SourmashKmerMinHash*>([&]() -> SourmashKmerMinHash* {        // ffi/signature.rs:167-182: a fresh clone
        if (SIG(p)->sketches.empty()) throw err_internal("found unsupported sketch type");
        return reinterpret_cast<SourmashKmerMinHash*>(new KmerMinHash(SIG(p)->sketches[0]));
    });
}
SourmashKmerMinHash** signature_get_mhs(const SourmashSignature* p, uintptr_t* size) {
    return landing<SourmashKmerMinHash**>([&]() -> SourmashKmerMinHash** {
        const auto& sk = SIG(p)->sketches;
        *size = sk.size();
        SourmashKmerMinHash** out = (SourmashKmerMinHash**)malloc((sk.size() ? sk.size() : 1) * sizeof(void*));
        for (size_t i = 0; i < sk.size(); ++i) out[i] = reinterpret_cast<SourmashKmerMinHash*>(new KmerMinHash(sk[i]));
        return out;
    });
}
void signature_set_mh(SourmashSignature* p, const SourmashKmerMinHash* o) {
    landing_void([&] { SIG(p)->sketches.clear(); SIG(p)->sketches.push_back(*MH(o)); });
}
void signature_push_mh(SourmashSignature* p, const SourmashKmerMinHash* o) {
    landing_void([&] { SIG(p)->sketches.push_back(*MH(o)); });
}
bool signature_eq(const SourmashSignature* p, const SourmashSignature* o) {
    return landing<bool>([&] { return SIG(p)->equals(*SIG(o)); });
}
SourmashStr signature_save_json(const SourmashSignature* p) {
    return landing<SourmashStr>([&] { std::string s; SIG(p)->to_json(s); return make_str(s); });
}


SourmashSignature** signatures_load_buffer(const char* ptr, uintptr_t insize, bool, uintptr_t ksize,
                                           const char* select_moltype, uintptr_t* size) {
    return landing<SourmashSignature**>([&]() -> SourmashSignature** {
        if (!ptr) throw err_internal("null buffer");
        uint32_t mol = 0;
        if (select_moltype) mol = molecule_from_name(select_moltype);
        return sigs_out(load_signatures(ptr, insize, ksize, select_moltype ? &mol : nullptr), size);
    });
}
SourmashSignature** signatures_load_path(const char* path, bool, uintptr_t ksize, const char* select_moltype,
                                         uintptr_t* size) {
    return landing<SourmashSignature**>([&]() -> SourmashSignature** {
        if (!path) throw err_internal("null path");
        std::ifstream in(path, std::ios::binary);
        if (!in) throw Error(E_IO, std::string("No such file or directory: ") + path);
        std::stringstream ss;
        ss << in.rdbuf();
        const std::string data = ss.str();
        uint32_t mol = 0;
        if (select_moltype) mol = molecule_from_name(select_moltype);
        return sigs_out(load_signatures(data.data(), data.size(), ksize, select_moltype ? &mol : nullptr), size);
    });
}
const uint8_t* signatures_save_buffer(const SourmashSignature* const* ptr, uintptr_t n, uint8_t compression,
                                      uintptr_t* osize) {
    return landing<const uint8_t*>([&]() -> const uint8_t* {                    // ffi/signature.rs:220-259
        if (!ptr && n) throw err_internal("null pointer");
        std::string s = "[";
        for (uintptr_t i = 0; i < n; ++i) { if (i) s += ','; SIG(ptr[i])->to_json(s); }
        s += ']';
        if (compression > 0) s = gzip_bytes(s, compression > 9 ? 9 : compression);
        *osize = s.size();
        uint8_t* out = (uint8_t*)malloc(s.size() ? s.size() : 1);
        memcpy(out, s.data(), s.size());
        return out;
    });
}
void nodegraph_buffer_free(uint8_t* ptr, uintptr_t) { free(ptr); }

// =============================================================================================
// PART 2: batch extensions
// =============================================================================================
uintptr_t smgpu_first_invalid_dna_byte(const char* seq, uintptr_t len) {
    if (!seq || !len) return UINTPTR_MAX;
    const size_t p = first_invalid_byte((const uint8_t*)seq, len);
    return p == SIZE_MAX ? UINTPTR_MAX : (uintptr_t)p;
}

int32_t smgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
bool smgpu_available(void) { return smgpu_device_count() > 0; }

void smgpu_minhash_add_buffer(SourmashKmerMinHash* p, const char* buf, uintptr_t len, bool force) {
    landing_void([&] {
        if (!buf && len) throw err_internal("null buffer");
        if (!MH(p)->is_dna())     // records joined in one buffer would shift the reading frames of the later records
            throw err_internal("smgpu_minhash_add_buffer takes DNA sketches; feed protein sketches record by record");
        add_sequence_dna(*RAW(p), (const uint8_t*)buf, len, force);
    });
}

// add_sequence with the error code as the return value (0 = fine): one call per record for bindings whose call overhead
// matters (ctypes); the message is left in the thread's error slot as usual.  len bytes, no NUL needed.
uint32_t smgpu_minhash_add_sequence_rc(SourmashKmerMinHash* p, const char* sequence, uintptr_t len, bool force) {
    g_err_code = 0;
    landing_void([&] {
        if (!sequence && len) throw err_internal("null sequence");
        // C-string semantics of kmerminhash_add_sequence: a NUL ends the record.  force = false scans the record anyway, and
        // a NUL is an invalid byte like any other: one pass finds whichever comes first.
        KmerMinHash& mh = *RAW(p);
        const uint8_t* seq = (const uint8_t*)sequence;
        if (!force && mh.is_dna()) {
            const size_t bad = first_invalid_byte(seq, len);
            if (bad == SIZE_MAX) { add_sequence_dna(mh, seq, len, false, true, SIZE_MAX); return; }
            if (seq[bad] == 0) { add_sequence_dna(mh, seq, bad, false, true, SIZE_MAX); return; }   // clean up to the NUL
            const void* nul = memchr(seq + bad, 0, len - bad);
            add_sequence_dna(mh, seq, nul ? (size_t)((const uint8_t*)nul - seq) : len, false, true, bad);
            return;
        }
        const void* nul = len ? memchr(sequence, 0, len) : nullptr;
        add_sequence_dna(mh, seq, nul ? (size_t)((const char*)nul - sequence) : len, force);
    });
    return g_err_code;
}
// settle the records queued by add_sequence now (the accessors do it on their own; this is for timing and tests)
void smgpu_minhash_flush(SourmashKmerMinHash* p) { landing_void([&] { settle(*RAW(p)); }); }
uint64_t smgpu_minhash_pending_bytes(const SourmashKmerMinHash* p) { return RAW(p)->pending.size(); }

}  // extern "C"
