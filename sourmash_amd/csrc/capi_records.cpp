// capi_records.cpp -- the C-ABI (include/sourmash_amd.h): one pass over the records of a device buffer or of a file, into one
// sketch per record (sketch_records.hip) or into the k-mers of a query sketch that the records hold (sketch_find.hip, find_core.hpp);
// fastx.hip parses the files.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <cmath>
#include <memory>
#include <thread>
#include "capi_common.hpp"
#include "ingest.hpp"
#include "pargz.hpp"

using namespace smg;

namespace {

// ---- one sketch per record of a device buffer / of a file (sketch_records.hip) ----------------------------------------------
// The reference's singleton loop (src/sourmash/command_sketch.py:712-739) makes a signature object, an add_sequence call and a
// sorted insert per record; here the records of a buffer become the rows of one CSR in a single pass over the buffer.

constexpr uint64_t RECORDS_MAX_FILE = (uint64_t)2 << 30;            // a file is resident as a whole (ingest.hpp: MAX_FILE)

// ---- what the passes over records (sketch_records_run and residue_records_run here, find_kmers_run below) share ----
// The workspace of a pass, carved: [pair hashes: cap u64][pair positions: cap u64][the scratch of the pass's second step]
struct PairWorkspace {
    uint64_t* d_pair_hash;
    uint64_t* d_pair_pos;
    void* d_tmp;
    size_t tmp_bytes;
    PairWorkspace(void* d_ws, uint64_t ws_bytes, uint64_t cap)
        : d_pair_hash((uint64_t*)d_ws), d_pair_pos((uint64_t*)((char*)d_ws + al256(cap * 8))), d_tmp((char*)d_ws + 2 * al256(cap * 8)),
          tmp_bytes((size_t)(ws_bytes - 2 * al256(cap * 8))) {}
};
// the arguments of a pass; ws_needed / ws_function: what the pass's workspace function answers, and its name
void check_pass_arguments(const uint64_t* d_starts, uint64_t n_records, uint64_t cap, uint64_t ws_bytes, uint64_t ws_needed, const char* ws_function) {
    if (!d_starts) throw err_internal("record starts: null (n_records + 1 ascending offsets are needed)");
    if (n_records > 0xfffffffeull) throw err_internal("record starts: too many records");
    if (cap > 0xffffffffull) throw err_internal("pair capacity above 2^32 - 1");
    if (ws_bytes < ws_needed) throw err_internal(std::string("workspace too small (") + ws_function + ")");
}
// head: d_result as read back; head[3] is the word records_check_starts_launch wrote
void raise_bad_starts(const unsigned long long head[4], uint64_t len) {
    if (head[3] & 2) throw err_internal("record starts: the last offset lies behind the end of the buffer (" + std::to_string(len) + " bytes)");
    if (head[3] & 1) throw err_internal("record starts: the offsets are not ascending");
}
// -> whether `pairs` (kept / matched: `what`) fit the capacity; if not, reported through *exceeded when there is one, else raised
bool pairs_fit(uint64_t pairs, uint64_t cap, const char* what, uint64_t* exceeded) {
    if (pairs <= cap) return true;
    if (exceeded) { *exceeded = pairs; return false; }
    throw err_internal("output capacity too small: " + std::to_string(pairs) + " " + what + " pairs > capacity " + std::to_string(cap));
}
// the count that the second step of a pass left in d_result[1]: the last read-back and synchronisation of the pass
uint64_t read_back_rows(const uint64_t* d_result, hipStream_t st) {
    unsigned long long n = 0;
    hip_check(hipMemcpyAsync(&n, d_result + 1, 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    return n;
}

// What differs between the passes.  pairs_first: the pair kernel does not read what the records say and is launched in front of
// the first read-back, so the pass synchronises twice; otherwise nothing is launched behind refused records, at a third
// synchronisation.
struct PassSpec {
    uint64_t ws_needed;             // what the pass's workspace function answers,
    const char* ws_function;        // and its name
    const char* ws_aligned_for;     // the entry point whose workspace has to be 8-byte aligned, or null
    const uint64_t* d_ends;         // checked against the starts when given
    bool pairs_first;
    const char* what;               // the pairs of the capacity error: "kept" / "matched"
};

// One pass over the records of a buffer: arguments, starts and ends checked, pairs(ws) produces (hash, position) pairs and counts
// them in d_result[0], rows(ws, n_pairs) makes the output from them and leaves its count in d_result[1].  -> that count.
// d_result: 4 x u64 -- [0] pairs, [1] the second step's count, [2] unused, [3] what is wrong with the records (1, 2: the starts;
// 4: an end outside its record).  *exceeded (may be null): instead of raising, report the pairs when they outnumber `cap`, and
// return ~0.  The errors come in this order: starts, ends, capacity.
template <class Pairs, class Rows>
uint64_t records_pass(const PassSpec& p, uint64_t len, const uint64_t* d_starts, uint64_t n_records, uint64_t cap, uint64_t* d_result, void* d_ws,
                      uint64_t ws_bytes, hipStream_t st, uint64_t* exceeded, Pairs&& pairs, Rows&& rows) {
    check_pass_arguments(d_starts, n_records, cap, ws_bytes, p.ws_needed, p.ws_function);
    if (p.ws_aligned_for && reinterpret_cast<uintptr_t>(d_ws) % 8) throw err_internal(std::string(p.ws_aligned_for) + ": the workspace must be 8-byte aligned");
    const PairWorkspace ws(d_ws, ws_bytes, cap);
    hip_check(hipMemsetAsync(d_result, 0, 32, st), "memset");
    hip_check(records_check_starts_launch(d_starts, n_records, len, (unsigned long long*)d_result + 3, st), "record starts");
    if (p.d_ends) hip_check(records_check_ends_launch(d_starts, p.d_ends, n_records, (unsigned long long*)d_result + 3, st), "record ends");
    if (p.pairs_first) pairs(ws);
    unsigned long long head[4] = {0, 0, 0, 0};
    hip_check(hipMemcpyAsync(head, d_result, 32, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    raise_bad_starts(head, len);
    if (head[3] & 4) throw err_internal("record ends: an end lies outside its record, [starts[r], starts[r + 1]]");
    if (!p.pairs_first) {
        pairs(ws);
        hip_check(hipMemcpyAsync(head, d_result, 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
    }
    if (!pairs_fit(head[0], cap, p.what, exceeded)) return ~0ull;
    rows(ws, head[0]);
    return read_back_rows(d_result, st);
}

// run(cap, exceeded) is a pass at a capacity: with the estimate first, where too many pairs are reported through *exceeded, and
// then once more with the reported count, where they are raised.  -> what the pass returns
template <class Run>
uint64_t with_pair_capacity(uint64_t estimate, Run&& run) {
    uint64_t cap = estimate;
    for (int attempt = 0;; ++attempt) {
        uint64_t exceeded = 0;
        const uint64_t n = run(cap, attempt == 0 ? &exceeded : nullptr);
        if (n != ~0ull) return n;
        cap = exceeded;                                              // repetitive input beat the estimate: once more with the count
    }
}

// DNA: the pair kernel runs in front of the verdict on the starts, which it does not read
uint64_t sketch_records_run(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, uint64_t n_records, uint32_t ksize, uint64_t seed,
                            uint64_t max_hash, uint64_t* d_hashes, uint64_t* d_abunds, uint64_t cap, uint64_t* d_offsets, uint64_t* d_result,
                            void* d_ws, uint64_t ws_bytes, hipStream_t st, uint64_t* exceeded) {
    if (ksize < 1 || ksize > 88) throw err_internal("per-record sketches take ksize 1 .. 88, not " + std::to_string(ksize));
    const PassSpec spec{smgpu_sketch_records_workspace_bytes(cap, n_records), "smgpu_sketch_records_workspace_bytes", nullptr, nullptr, true, "kept"};
    return records_pass(
        spec, len, d_starts, n_records, cap, d_result, d_ws, ws_bytes, st, exceeded,
        [&](const PairWorkspace& ws) {
            hip_check(records_pairs_launch(d_seq, len, ksize, seed, max_hash ? max_hash : ~0ull, ws.d_pair_hash, ws.d_pair_pos, (unsigned long long*)d_result, cap, st),
                      "sketch_records");
        },
        [&](const PairWorkspace& ws, uint64_t n_pairs) {
            hip_check(records_csr_launch(ws.d_pair_hash, ws.d_pair_pos, n_pairs, d_starts, n_records, ksize, max_hash, d_hashes, d_abunds, d_offsets, d_result + 1,
                                         ws.d_tmp, ws.tmp_bytes, st), "records_csr");
        });
}

// ---- one protein / dayhoff / hp sketch per record (protein_records.hip) -------------------------------------------------------
constexpr uint32_t RESIDUE_RECORDS_MAX_K = 79;                      // the register-window form (residue_core.hpp: RW_MAX_NB)

// bytes of the residue buffer of a pass: protein input, the input's own; translated, the bound of the records' blocks
uint64_t residue_buffer_bytes(uint64_t len, uint64_t n_records, bool translate) {
    return al256((translate ? translated_records_bytes_bound(len, n_records) : len) + 64);
}
uint64_t residue_records_workspace(uint64_t cap, uint64_t n_records, uint64_t len, bool translate) {
    return 2 * al256(cap * 8) + al256(records_csr_temp_bytes(cap)) + residue_buffer_bytes(len, n_records, translate) +
           (translate ? al256((n_records + 2) * 8) + al256(translate_records_temp_bytes(n_records)) : 0) + 512;
}

// Residue windows: the translation reads what the records say, so the verdict comes first.  The workspace behind the pairs: [CSR
// scratch][residue buffer][translated: block starts, n_records + 1 u64][translated: the scan's scratch].
uint64_t residue_records_run(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, const uint64_t* d_ends, uint64_t n_records, uint32_t ksize,
                             uint32_t hf, bool translate, uint64_t seed, uint64_t max_hash, uint64_t* d_hashes, uint64_t* d_abunds, uint64_t cap,
                             uint64_t* d_offsets, uint64_t* d_result, void* d_ws, uint64_t ws_bytes, hipStream_t st, uint64_t* exceeded) {
    if (ksize < 1 || ksize > RESIDUE_RECORDS_MAX_K)
        throw err_internal("per-record residue sketches take ksize 1 .. 79 residues, not " + std::to_string(ksize));
    if (hf != HF_PROTEIN && hf != HF_DAYHOFF && hf != HF_HP) throw err_internal("per-record residue sketches are protein, dayhoff or hp sketches");
    const size_t csr_bytes = al256(records_csr_temp_bytes(cap));
    uint64_t* d_blocks = nullptr;                                   // (translated) the records' blocks in the residue buffer
    const PassSpec spec{residue_records_workspace(cap, n_records, len, translate), "smgpu_sketch_residue_records_workspace_bytes",
                        "smgpu_sketch_residue_records_raw", d_ends, false, "kept"};
    return records_pass(
        spec, len, d_starts, n_records, cap, d_result, d_ws, ws_bytes, st, exceeded,
        [&](const PairWorkspace& ws) {
            uint8_t* d_aa = (uint8_t*)ws.d_tmp + csr_bytes;
            char* at = (char*)d_aa + residue_buffer_bytes(len, n_records, translate);
            const uint64_t thr = max_hash ? max_hash : ~0ull;
            if (translate) {
                d_blocks = (uint64_t*)at;
                void* d_scan = at + al256((n_records + 2) * 8);
                hip_check(translate_records_launch(d_seq, len, d_starts, d_ends, n_records, hf, d_blocks, d_aa, d_scan, al256(translate_records_temp_bytes(n_records)), st),
                          "translate_records");
                if (n_records)
                    hip_check(residue_pairs_launch(d_aa, translated_records_bytes_bound(len, n_records), d_blocks + n_records, ksize, seed, thr, ws.d_pair_hash,
                                                   ws.d_pair_pos, (unsigned long long*)d_result, cap, st), "residue_pairs");
            } else {
                hip_check(residues_launch(d_seq, len, hf, d_aa, st), "residues");
                hip_check(residue_pairs_launch(d_aa, len, nullptr, ksize, seed, thr, ws.d_pair_hash, ws.d_pair_pos, (unsigned long long*)d_result, cap, st),
                          "residue_pairs");
            }
        },
        [&](const PairWorkspace& ws, uint64_t n_pairs) {
            // translated: a window's record is the block of its start, and no window reaches out of a block (every block ends in 0xFF)
            hip_check(records_csr_ends_launch(ws.d_pair_hash, ws.d_pair_pos, n_pairs, translate ? d_blocks : d_starts, translate ? nullptr : d_ends, n_records, ksize,
                                              max_hash, d_hashes, d_abunds, d_offsets, d_result + 1, ws.d_tmp, csr_bytes, st), "records_csr");
        });
}

// pairs a buffer of len bytes is expected to keep, with the slack of sketch_slices_batched (ingest.hpp); never more than len
uint64_t records_pair_estimate(uint64_t len, uint64_t max_hash) {
    const double frac = max_hash ? (double)max_hash / 18446744073709551616.0 : 1.0;
    const double l = (double)len;
    const uint64_t est = (uint64_t)(l * frac * 2.0 + 16.0 * std::sqrt(l * frac + 1.0)) + 4096;
    return std::max<uint64_t>(1, std::min<uint64_t>(len, est));
}

// The CSR of one (ksize, hf, seed, max_hash) over the records of a device buffer, in blocks of its own.  residue: the residue
// pass, windows of ksize residues (translated input has two residues per base), which refuses an hf that is not protein, dayhoff
// or hp; else the DNA pass, k-mers, with hf, d_ends and translate unused.  The caller says which: a C-ABI entry serves one of
// the two, whatever hash_function it is handed.
struct RecordsCsr { DevBuf hashes, abunds, offsets; uint64_t total = 0; };
void records_csr(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, const uint64_t* d_ends, uint64_t n_records, uint32_t ksize, bool residue,
                 uint32_t hf, bool translate, uint64_t seed, uint64_t max_hash, bool want_abunds, RecordsCsr& out, hipStream_t st) {
    const bool dna = !residue;
    out.offsets.reserve((n_records + 1) * 8 + 16, st);
    AsyncBuf result(64, st);
    out.total = with_pair_capacity(records_pair_estimate(!dna && translate ? 2 * len : len, max_hash), [&](uint64_t cap, uint64_t* exceeded) {
        out.hashes.reserve(cap * 8 + 16, st);
        if (want_abunds) out.abunds.reserve(cap * 8 + 16, st);
        const uint64_t ws_bytes = dna ? smgpu_sketch_records_workspace_bytes(cap, n_records) : residue_records_workspace(cap, n_records, len, translate);
        AsyncBuf ws((size_t)ws_bytes, st);
        uint64_t *h = out.hashes.as<uint64_t>(), *a = want_abunds ? out.abunds.as<uint64_t>() : nullptr, *o = out.offsets.as<uint64_t>();
        return dna ? sketch_records_run(d_seq, len, d_starts, n_records, ksize, seed, max_hash, h, a, cap, o, result.as<uint64_t>(), ws.p, ws_bytes, st, exceeded)
                   : residue_records_run(d_seq, len, d_starts, d_ends, n_records, ksize, hf, translate, seed, max_hash, h, a, cap, o, result.as<uint64_t>(), ws.p,
                                         ws_bytes, st, exceeded);
    });
}

// a set that takes over the blocks of the records' CSR; ksize in units of the molecule.  want_abunds: an abundance set, which
// takes over the third block too -- every kept hash's multiplicity in its record (at least 1)
SketchSet* sketchset_from_records(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, const uint64_t* d_ends, uint64_t n_records, uint32_t ksize,
                                  bool residue, uint32_t hf, bool translate, uint64_t seed, uint64_t scaled, hipStream_t st, bool want_abunds = false) {
    if (scaled == 0) throw err_internal("per-record sketches are scaled sketches: scaled must not be 0");
    const uint64_t max_hash = max_hash_for_scaled(scaled);
    RecordsCsr csr;
    records_csr(d_seq, len, d_starts, d_ends, n_records, ksize, residue, hf, translate, seed, max_hash, want_abunds, csr, st);
    std::unique_ptr<SketchSet> s(new SketchSet());
    s->n = n_records; s->total = csr.total;
    s->ksize = ksize; s->hash_function = hf; s->seed = seed; s->max_hash = max_hash; s->num = 0;
    s->host_offsets.assign(n_records + 1, 0);
    hip_check(hipMemcpyAsync(s->host_offsets.data(), csr.offsets.p, (n_records + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    std::swap(s->hashes.p, csr.hashes.p); std::swap(s->hashes.cap, csr.hashes.cap); std::swap(s->hashes.st, csr.hashes.st);
    std::swap(s->offsets.p, csr.offsets.p); std::swap(s->offsets.cap, csr.offsets.cap); std::swap(s->offsets.st, csr.offsets.st);
    if (want_abunds) {
        std::swap(s->abunds.p, csr.abunds.p); std::swap(s->abunds.cap, csr.abunds.cap); std::swap(s->abunds.st, csr.abunds.st);
        if (!s->abunds.p) s->abunds.reserve(16, st);                 // (no record kept a hash: still an abundance set)
        AsyncBuf d_max(64, st);
        uint64_t found[2] = {0, ~0ull};
        hip_check(abund_check_launch(s->abunds.as<uint64_t>(), s->total, d_max.as<uint64_t>(), st), "abund_check");
        hip_check(hipMemcpyAsync(found, d_max.p, 16, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        if (found[1] != ~0ull) throw err_internal("per-record sketches: a kept hash with multiplicity 0");
        s->abund_max = found[0];
    }
    s->rows.resize(n_records);
    for (uint64_t r = 0; r < n_records; ++r) {
        ManifestRow& m = s->rows[r];
        m.ksize = ksize; m.moltype = molecule_name(hf); m.scaled = scaled; m.with_abundance = want_abunds;
        m.n_hashes = s->host_offsets[r + 1] - s->host_offsets[r];
    }
    return s.release();
}

// the whole file in host memory (gzip: through the host inflater); throws when it is larger than RECORDS_MAX_FILE
void read_whole_file(const std::string& path, std::vector<uint8_t>& out) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) throw Error(E_IO, "No such file or directory: " + path);
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { ::close(fd); throw Error(E_IO, "cannot read " + path); }
    uint8_t magic[2] = {0, 0};
    const bool gz = ::pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    const std::string too_large = "file outside the size limit of per-record sketching (" + std::to_string(RECORDS_MAX_FILE) + " bytes): " + path;
    if (!gz) {
        const uint64_t size = (uint64_t)sb.st_size;
        if (size > RECORDS_MAX_FILE) { ::close(fd); throw err_internal(too_large); }
        out.resize((size_t)size);
        uint64_t got = 0;
        while (got < size) {
            const ssize_t r = ::pread(fd, out.data() + got, (size_t)(size - got), (off_t)got);
            if (r <= 0) { ::close(fd); throw Error(E_IO, "short read on " + path); }
            got += (uint64_t)r;
        }
        ::close(fd);
        return;
    }
    ::close(fd);
    try {
        ParallelGunzip pg(path);
        size_t at = 0;
        out.resize((size_t)64 << 20);
        for (;;) {
            const size_t got = pg.read(out.data() + at, out.size() - at);
            at += got;
            if (at < out.size()) break;                              // short only at the end of the stream
            if (at > RECORDS_MAX_FILE) throw err_internal(too_large);
            out.resize(out.size() * 2);
        }
        out.resize(at);
    } catch (const std::runtime_error& e) {
        if (dynamic_cast<const Error*>(&e)) throw;
        throw Error(E_NIFFLER, std::string("cannot inflate ") + path + ": " + e.what());
    }
    if (out.size() > RECORDS_MAX_FILE) throw err_internal(too_large);
}

// the header lines of a FASTA / 4-line FASTQ file as the device parser counts them (fastx.hip): FASTA, every line that starts
// with '>'; FASTQ, every fourth line.  A name is the line behind its first byte, CR / LF stripped.
void scan_record_names(const uint8_t* p, size_t n, bool fastq, std::vector<std::string>& names) {
    size_t line = 0, at = 0;
    while (at < n) {
        const uint8_t* nl = (const uint8_t*)memchr(p + at, '\n', n - at);
        const size_t end = nl ? (size_t)(nl - p) : n;
        if (fastq ? (line & 3) == 0 : p[at] == '>') {
            size_t e = end;
            while (e > at + 1 && (p[e - 1] == '\r' || p[e - 1] == '\n')) --e;
            names.emplace_back((const char*)p + at + 1, e > at + 1 ? e - at - 1 : 0);
        }
        ++line;
        at = end + 1;
    }
}

// a file's sequence bytes and record starts in HBM, its record names on the host
struct ParsedRecords {
    AsyncBuf comp, starts;
    uint64_t len = 0, n_records = 0;
    std::vector<std::string> names;
};
void parse_records_file(const std::string& path, ParsedRecords& out, hipStream_t st) {
    std::vector<uint8_t> host;
    read_whole_file(path, host);
    const uint64_t n = host.size();
    const bool fastq = n && host[0] == '@';
    std::thread namer([&] { scan_record_names(host.data(), host.size(), fastq, out.names); });   // while the bytes go up
    struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } } join{namer};
    AsyncBuf raw((size_t)n + 64, st);
    if (n) hip_check(hipMemcpyAsync(raw.p, host.data(), (size_t)n, hipMemcpyHostToDevice, st), "H2D");
    namer.join();
    out.n_records = out.names.size();
    out.comp.reset((size_t)n + 64, st);
    out.starts.reset((out.n_records + 2) * 8, st);
    const size_t temp_bytes = fastx_records_temp_bytes(n ? n : 1);
    AsyncBuf temp(temp_bytes, st), small(64, st);
    uint8_t h_small[32] = {0};
    h_small[0] = (uint8_t)(fastq ? 3 : 1); h_small[1] = 1;             // the parser's carry; n_kept at byte 8, records at byte 16
    hip_check(hipMemcpyAsync(small.p, h_small, 32, hipMemcpyHostToDevice, st), "H2D");
    hip_check(hipMemsetAsync(out.starts.p, 0, (out.n_records + 2) * 8, st), "memset");
    uint8_t* sc = small.as<uint8_t>();
    hip_check(fastx_compact_launch(raw.as<uint8_t>(), n, fastq ? 1 : 0, sc, nullptr, out.comp.as<uint8_t>(), reinterpret_cast<unsigned long long*>(sc + 8),
                                   reinterpret_cast<unsigned long long*>(sc + 16), temp.p, temp_bytes, st, true,
                                   out.starts.as<unsigned long long>(), out.n_records), "fastx");
    // starts[n_records] = the end of the compacted bytes
    hip_check(hipMemcpyAsync(out.starts.as<uint64_t>() + out.n_records, sc + 8, 8, hipMemcpyDeviceToDevice, st), "D2D");
    hip_check(hipMemcpyAsync(h_small, small.p, 32, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    uint64_t kept = 0, recs = 0;
    memcpy(&kept, h_small + 8, 8); memcpy(&recs, h_small + 16, 8);
    if (recs != out.n_records)
        throw err_internal("record count of the device parser (" + std::to_string(recs) + ") differs from the header lines read on the host (" +
                           std::to_string(out.n_records) + "): " + path);
    out.len = kept;
}

// where the records of a parsed file end: in front of the header byte the parser keeps between two records
void file_record_ends(const ParsedRecords& pr, AsyncBuf& ends, hipStream_t st) {
    ends.reset((pr.n_records + 1) * 8, st);
    hip_check(records_file_ends_launch(pr.starts.as<uint64_t>(), pr.n_records, ends.as<uint64_t>(), st), "record ends");
}

// sketchset_from_records over the records of a file, the rows named after them; the DNA pass takes no ends
SketchSet* sketchset_from_file(const char* path, uint32_t ksize, bool residue, uint32_t hf, bool translate, uint64_t seed, uint64_t scaled,
                               bool want_abunds = false) {
    if (!path) throw err_internal("null path");
    DeviceCtx& ctx = DeviceCtx::get();
    std::lock_guard<std::recursive_mutex> g(ctx.mutex());
    hipStream_t st = ctx.stream();
    ParsedRecords pr;
    parse_records_file(path, pr, st);
    AsyncBuf ends;
    if (residue) file_record_ends(pr, ends, st);
    std::unique_ptr<SketchSet> s(sketchset_from_records(pr.comp.as<uint8_t>(), pr.len, pr.starts.as<uint64_t>(), residue ? ends.as<uint64_t>() : nullptr,
                                                        pr.n_records, ksize, residue, hf, translate, seed, scaled, st, want_abunds));
    for (uint64_t r = 0; r < pr.n_records; ++r) { s->rows[r].name = pr.names[r]; s->rows[r].filename = path; }
    return s.release();
}

// every record of a file as a signature holding every sketch of `cp`: what smgpu_sketch_file_singleton and its residue sibling run
SourmashSignature** file_singleton(const char* path, const ComputeParameters& cp, bool input_is_protein, uintptr_t* n) {
    if (cp.scaled == 0) throw err_internal("smgpu_sketch_file_singleton takes scaled sketches");
    for (uint32_t k : cp.ksizes) {
        if (cp.dna && (k < 1 || k > 88)) throw err_internal("per-record sketches take ksize 1 .. 88, not " + std::to_string(k));
        if ((cp.protein || cp.dayhoff || cp.hp) && (k < 3 || k / 3 > RESIDUE_RECORDS_MAX_K))
            throw err_internal("per-record residue sketches take ksize 1 .. 79 residues, not " + std::to_string(k / 3));
    }
    DeviceCtx& ctx = DeviceCtx::get();
    std::lock_guard<std::recursive_mutex> g(ctx.mutex());
    hipStream_t st = ctx.stream();
    ParsedRecords pr;
    parse_records_file(path, pr, st);
    std::vector<Signature> sigs;
    sigs.reserve(pr.n_records);
    for (uint64_t r = 0; r < pr.n_records; ++r) {
        sigs.push_back(Signature::from_params(cp));
        sigs.back().name = pr.names[r];
        sigs.back().filename = std::string(path);
    }
    // one kernel pass per sketch of the template over the same parsed buffer and the same starts
    const Signature tmpl = Signature::from_params(cp);
    std::vector<uint64_t> off(pr.n_records + 1), hs, as;
    AsyncBuf ends;
    if (cp.protein || cp.dayhoff || cp.hp) file_record_ends(pr, ends, st);
    for (size_t q = 0; q < tmpl.sketches.size(); ++q) {
        const KmerMinHash& t = tmpl.sketches[q];
        const bool dna = t.hash_function == HF_DNA;
        RecordsCsr csr;
        records_csr(pr.comp.as<uint8_t>(), pr.len, pr.starts.as<uint64_t>(), ends.as<uint64_t>(), pr.n_records, dna ? t.ksize : t.ksize / 3, !dna, t.hash_function,
                    !input_is_protein, t.seed, t.max_hash, t.track_abundance, csr, st);
        hs.resize(csr.total); as.resize(t.track_abundance ? csr.total : 0);
        hip_check(hipMemcpyAsync(off.data(), csr.offsets.p, (pr.n_records + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
        if (csr.total) hip_check(hipMemcpyAsync(hs.data(), csr.hashes.p, csr.total * 8, hipMemcpyDeviceToHost, st), "D2H");
        if (csr.total && t.track_abundance) hip_check(hipMemcpyAsync(as.data(), csr.abunds.p, csr.total * 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        for (uint64_t r = 0; r < pr.n_records; ++r) {
            KmerMinHash& mh = sigs[r].sketches[q];
            mh.mins.assign(hs.begin() + (long)off[r], hs.begin() + (long)off[r + 1]);
            if (t.track_abundance) mh.abunds.assign(as.begin() + (long)off[r], as.begin() + (long)off[r + 1]);
            mh.touch();
        }
    }
    return sigs_out(std::move(sigs), n);
}

// ---- a sketch's k-mers in sequences (sketch_find.hip; `sourmash sig kmers`, src/sourmash/sig/__main__.py:1087-1310) ----------

// The query: the merged sketch on the host; its hashes and their bucket directory (find_core.hpp) go to the device when a find
// first needs them, on the library's stream, and stay there for the life of the handle.
struct KmerQuery {
    KmerMinHash mh;
    std::mutex mu;
    bool on_device = false;
    DevBuf d_q, d_dir;
    FindQuery dev{nullptr, nullptr, 0, 0};
};

FindQuery query_on_device(const KmerQuery* cq) {
    KmerQuery* q = const_cast<KmerQuery*>(cq);
    DeviceCtx& ctx = DeviceCtx::get();
    std::lock_guard<std::recursive_mutex> g(ctx.mutex());          // the context first, then the query: the file entry holds the context
    std::lock_guard<std::mutex> own(q->mu);
    if (q->on_device) return q->dev;
    hipStream_t st = ctx.stream();
    const uint64_t n = q->mh.mins.size();
    if (n > FIND_MAX_QUERY) throw err_internal("query of more than 2^32 - 2 hashes");
    const uint32_t shift = find_dir_shift(n, q->mh.max_hash);
    const uint64_t nb = find_dir_buckets(q->mh.max_hash, shift);
    q->d_q.reserve(n * 8 + 16, st);
    q->d_dir.reserve((nb + 1) * 4 + 16, st);
    hip_check(hipMemcpyAsync(q->d_q.p, q->mh.mins.data(), n * 8, hipMemcpyHostToDevice, st), "H2D");
    hip_check(find_dir_launch(q->d_q.as<uint64_t>(), n, shift, nb, q->d_dir.as<uint32_t>(), st), "find_dir");
    hip_check(hipStreamSynchronize(st), "sync");                    // any stream may use it from here on
    q->dev = FindQuery{q->d_q.as<uint64_t>(), q->d_dir.as<uint32_t>(), q->mh.max_hash, shift};
    q->on_device = true;
    return q->dev;
}

// d_result: 4 x u64 -- [0] matched (hash, position) pairs, [1] rows, [2] unused, [3] what is wrong with the starts.
// *exceeded (may be null): instead of raising, report the pairs matched when they outnumber `cap`.
uint64_t find_kmers_run(const KmerQuery* q, const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, uint64_t n_records,
                        uint64_t* d_positions, uint64_t* d_hashes, uint8_t* d_kmers, uint64_t cap, uint64_t* d_offsets, uint64_t* d_result,
                        void* d_ws, uint64_t ws_bytes, hipStream_t st, uint64_t* exceeded) {
    if (!q) throw err_internal("null query");
    const uint32_t ksize = q->mh.ksize;
    if (ksize < 1 || ksize > 88) throw err_internal("k-mer finding takes ksize 1 .. 88, not " + std::to_string(ksize));
    const PassSpec spec{smgpu_find_kmers_workspace_bytes(cap, n_records), "smgpu_find_kmers_workspace_bytes", nullptr, nullptr, false, "matched"};
    return records_pass(
        spec, len, d_starts, n_records, cap, d_result, d_ws, ws_bytes, st, exceeded,
        [&](const PairWorkspace& ws) {
            // the query goes to the device here, behind the verdict on the starts: refused starts upload nothing, and where both
            // are wrong the starts' error is the one raised
            hip_check(find_pairs_launch(d_seq, len, ksize, q->mh.seed, query_on_device(q), ws.d_pair_hash, ws.d_pair_pos, (unsigned long long*)d_result, cap, 0, st),
                      "find_kmers");
        },
        [&](const PairWorkspace& ws, uint64_t n_pairs) {
            hip_check(find_rows_launch(d_seq, len, ws.d_pair_hash, ws.d_pair_pos, n_pairs, d_starts, n_records, ksize, d_positions, d_hashes, d_kmers, d_offsets,
                                       d_result + 1, ws.d_tmp, ws.tmp_bytes, st), "find_rows");
        });
}

// what a file's search leaves on the host
struct KmerMatches {
    uint32_t ksize = 0;
    uint64_t n_records = 0, n_rows = 0, n_bases = 0;
    std::vector<uint64_t> offsets, positions, hashes, starts, lengths;
    std::vector<uint8_t> kmers, seq;                                // seq: the parsed sequence bytes, kept only when there are rows
    std::vector<std::string> names;
};

}  // namespace

extern "C" {

uint64_t smgpu_sketch_records_workspace_bytes(uint64_t pair_capacity, uint64_t n_records) {
    (void)n_records;                                                // (the offsets are the caller's; the scratch depends on the pairs alone)
    return 2 * al256(pair_capacity * 8) + records_csr_temp_bytes(pair_capacity) + 512;
}

uint64_t smgpu_sketch_records_raw(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, uint64_t n_records, uint32_t ksize, uint64_t seed,
                                  uint64_t max_hash, uint64_t* d_hashes, uint64_t* d_abunds, uint64_t capacity, uint64_t* d_offsets,
                                  uint64_t* d_result, void* d_workspace, uint64_t workspace_bytes, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        ret = sketch_records_run(d_seq, len, d_starts, n_records, ksize, seed, max_hash, d_hashes, d_abunds, capacity, d_offsets, d_result,
                                 d_workspace, workspace_bytes, (hipStream_t)stream, nullptr);
    });
    return ret;
}

void smgpu_sketch_records_kernel_raw(const uint8_t* d_seq, uint64_t len, uint32_t ksize, uint64_t seed, uint64_t max_hash, uint64_t* d_hashes,
                                     uint64_t* d_positions, uint64_t capacity, uint64_t* d_count, void* stream) {
    landing_void([&] {
        if (ksize < 1 || ksize > 88) throw err_internal("per-record sketches take ksize 1 .. 88, not " + std::to_string(ksize));
        hip_check(records_pairs_launch(d_seq, len, ksize, seed, max_hash ? max_hash : ~0ull, d_hashes, d_positions, (unsigned long long*)d_count,
                                       capacity, (hipStream_t)stream), "sketch_records");
    });
}

void smgpu_fastx_compact_raw(const uint8_t* d_raw, uint64_t len, int32_t fastq, uint8_t* d_carry, uint8_t* d_out, uint64_t* d_result,
                             uint64_t* d_record_starts, uint64_t record_capacity, int32_t last_piece, void* stream) {
    landing_void([&] {
        if (!d_carry || !d_result || (len && (!d_raw || !d_out))) throw err_internal("smgpu_fastx_compact_raw: null pointer");
        if (reinterpret_cast<uintptr_t>(d_raw) % FASTX_RAW_ALIGN)                  // before anything is launched: the lanes load 16 bytes at a time
            throw err_internal("smgpu_fastx_compact_raw: d_raw must be " + std::to_string(FASTX_RAW_ALIGN) + "-byte aligned");
        hipStream_t st = (hipStream_t)stream;
        const size_t temp_bytes = d_record_starts ? fastx_records_temp_bytes(len ? len : 1) : fastx_temp_bytes(len ? len : 1);
        AsyncBuf temp(temp_bytes, st);
        unsigned long long* res = reinterpret_cast<unsigned long long*>(d_result);
        hip_check(fastx_compact_launch(d_raw, len, fastq ? 1 : 0, d_carry, nullptr, d_out, res, res + 1, temp.p, temp_bytes, st, last_piece != 0,
                                       reinterpret_cast<unsigned long long*>(d_record_starts), record_capacity), "fastx");
    });
}

SmgpuSketchSet* smgpu_sketchset_sketch_records(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, uint64_t n_records, uint32_t ksize,
                                               uint64_t seed, uint64_t scaled) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_from_records(d_seq, len, d_starts, nullptr, n_records, ksize, false, HF_DNA, false, seed, scaled, ctx.stream()));
    });
}

SmgpuSketchSet* smgpu_sketchset_sketch_file(const char* path, uint32_t ksize, uint64_t seed, uint64_t scaled) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_from_file(path, ksize, false, HF_DNA, false, seed, scaled));
    });
}

// the same four with the records' multiplicities kept: abundance sets (track_abundance = 0: the flat entries themselves)
SmgpuSketchSet* smgpu_sketchset_sketch_records_abund(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, uint64_t n_records, uint32_t ksize,
                                                     uint64_t seed, uint64_t scaled, uint32_t track_abundance) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_from_records(d_seq, len, d_starts, nullptr, n_records, ksize, false, HF_DNA, false, seed, scaled, ctx.stream(),
                                                                        track_abundance != 0));
    });
}

SmgpuSketchSet* smgpu_sketchset_sketch_file_abund(const char* path, uint32_t ksize, uint64_t seed, uint64_t scaled, uint32_t track_abundance) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_from_file(path, ksize, false, HF_DNA, false, seed, scaled, track_abundance != 0));
    });
}

SmgpuSketchSet* smgpu_sketchset_sketch_residue_records_abund(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, const uint64_t* d_ends,
                                                             uint64_t n_records, uint32_t ksize, uint32_t hash_function, int32_t translate, uint64_t seed,
                                                             uint64_t scaled, uint32_t track_abundance) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_from_records(d_seq, len, d_starts, d_ends, n_records, ksize, true, hash_function, translate != 0, seed, scaled,
                                                                        ctx.stream(), track_abundance != 0));
    });
}

SmgpuSketchSet* smgpu_sketchset_sketch_residue_file_abund(const char* path, uint32_t ksize, uint32_t hash_function, int32_t translate, uint64_t seed,
                                                          uint64_t scaled, uint32_t track_abundance) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_from_file(path, ksize, true, hash_function, translate != 0, seed, scaled, track_abundance != 0));
    });
}

SourmashSignature** smgpu_sketch_file_singleton(const char* path, const SourmashComputeParameters* params, uintptr_t* n) {
    return landing<SourmashSignature**>([&]() -> SourmashSignature** {
        if (!path || !n) throw err_internal("null argument");
        const ComputeParameters& cp = *CP(params);
        if (!cp.dna || cp.protein || cp.dayhoff || cp.hp) throw err_internal("smgpu_sketch_file_singleton takes DNA parameters");
        return file_singleton(path, cp, false, n);
    });
}

SourmashSignature** smgpu_sketch_file_singleton_residues(const char* path, const SourmashComputeParameters* params, int32_t input_is_protein,
                                                         uintptr_t* n) {
    return landing<SourmashSignature**>([&]() -> SourmashSignature** {
        if (!path || !n) throw err_internal("null argument");
        const ComputeParameters& cp = *CP(params);
        if (input_is_protein && cp.dna) throw err_internal("smgpu_sketch_file_singleton_residues: protein input takes no DNA sketch");
        return file_singleton(path, cp, input_is_protein != 0, n);
    });
}

uint64_t smgpu_sketch_residue_records_workspace_bytes(uint64_t pair_capacity, uint64_t n_records, uint64_t len, int32_t translate) {
    return residue_records_workspace(pair_capacity, n_records, len, translate != 0);
}

uint64_t smgpu_sketch_residue_records_raw(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, const uint64_t* d_ends, uint64_t n_records,
                                          uint32_t ksize, uint32_t hash_function, int32_t translate, uint64_t seed, uint64_t max_hash,
                                          uint64_t* d_hashes, uint64_t* d_abunds, uint64_t capacity, uint64_t* d_offsets, uint64_t* d_result,
                                          void* d_workspace, uint64_t workspace_bytes, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        ret = residue_records_run(d_seq, len, d_starts, d_ends, n_records, ksize, hash_function, translate != 0, seed, max_hash, d_hashes, d_abunds,
                                  capacity, d_offsets, d_result, d_workspace, workspace_bytes, (hipStream_t)stream, nullptr);
    });
    return ret;
}

void smgpu_residue_records_kernel_raw(const uint8_t* d_aa, uint64_t n, const uint64_t* d_n, uint32_t ksize, uint64_t seed, uint64_t max_hash,
                                      uint64_t* d_hashes, uint64_t* d_positions, uint64_t capacity, uint64_t* d_count, void* stream) {
    landing_void([&] {
        if (ksize < 1 || ksize > RESIDUE_RECORDS_MAX_K)
            throw err_internal("per-record residue sketches take ksize 1 .. 79 residues, not " + std::to_string(ksize));
        if (!d_aa || !d_hashes || !d_count || reinterpret_cast<uintptr_t>(d_aa) % 8)
            throw err_internal("smgpu_residue_records_kernel_raw: null pointer or a residue buffer that is not 8-byte aligned");
        const uint64_t thr = max_hash ? max_hash : ~0ull;
        if (d_positions)
            hip_check(residue_pairs_launch(d_aa, n, d_n, ksize, seed, thr, d_hashes, d_positions, (unsigned long long*)d_count, capacity,
                                           (hipStream_t)stream), "residue_pairs");
        else
            hip_check(residue_windows_launch(d_aa, n, ksize, seed, thr, d_hashes, (unsigned long long*)d_count, capacity, false, (hipStream_t)stream),
                      "residue_windows");
    });
}

SmgpuSketchSet* smgpu_sketchset_sketch_residue_records(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, const uint64_t* d_ends,
                                                       uint64_t n_records, uint32_t ksize, uint32_t hash_function, int32_t translate, uint64_t seed,
                                                       uint64_t scaled) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_from_records(d_seq, len, d_starts, d_ends, n_records, ksize, true, hash_function, translate != 0, seed, scaled,
                                                                        ctx.stream()));
    });
}

SmgpuSketchSet* smgpu_sketchset_sketch_residue_file(const char* path, uint32_t ksize, uint32_t hash_function, int32_t translate, uint64_t seed,
                                                    uint64_t scaled) {
    return landing<SmgpuSketchSet*>([&]() -> SmgpuSketchSet* {
        return reinterpret_cast<SmgpuSketchSet*>(sketchset_from_file(path, ksize, true, hash_function, translate != 0, seed, scaled));
    });
}

SmgpuKmerQuery* smgpu_kmerquery_new(const SourmashKmerMinHash* const* mhs, uintptr_t n) {
    return landing<SmgpuKmerQuery*>([&]() -> SmgpuKmerQuery* {
        if (!mhs || n == 0) throw Error(E_EMPTY_SIGNATURE, "no query signatures");
        for (uintptr_t i = 0; i < n; ++i)
            if (!mhs[i]) throw err_internal("null sketch");
        const KmerMinHash& first = *MH(mhs[0]);
        if (first.hash_function != HF_DNA)
            throw Error(E_MISMATCH_DNA_PROT, std::string("k-mer finding takes DNA sketches, not ") + molecule_name(first.hash_function));
        std::unique_ptr<KmerQuery> q(new KmerQuery());
        q->mh = KmerMinHash(first.scaled(), first.ksize, first.hash_function, first.seed, false, first.num);   // copy_and_clear, flat
        q->mh.max_hash = first.max_hash;
        for (uintptr_t i = 0; i < n; ++i) {
            const KmerMinHash& m = *MH(mhs[i]);
            if (m.num != 0 || m.max_hash == 0) throw Error(E_MISMATCH_NUM, "k-mer finding takes scaled sketches, not num sketches");
            q->mh.merge(m);
        }
        if (q->mh.mins.empty()) throw Error(E_EMPTY_SIGNATURE, "no hashes in query signature");
        return reinterpret_cast<SmgpuKmerQuery*>(q.release());
    });
}

void smgpu_kmerquery_free(SmgpuKmerQuery* p) {
    KmerQuery* q = reinterpret_cast<KmerQuery*>(p);
    if (!q) return;
    if (q->on_device) {
        if (DeviceCtx* ctx = DeviceCtx::peek()) {
            std::lock_guard<std::recursive_mutex> g(ctx->mutex());
            delete q;
            return;
        }
    }
    delete q;
}

uint64_t smgpu_kmerquery_len(const SmgpuKmerQuery* p) { return p ? reinterpret_cast<const KmerQuery*>(p)->mh.mins.size() : 0; }

uint64_t smgpu_find_kmers_workspace_bytes(uint64_t pair_capacity, uint64_t n_records) {
    (void)n_records;                                                // (the offsets are the caller's; the scratch depends on the pairs alone)
    return 2 * al256(pair_capacity * 8) + find_rows_temp_bytes(pair_capacity) + 512;
}

uint64_t smgpu_find_kmers_raw(const SmgpuKmerQuery* query, const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, uint64_t n_records,
                              uint64_t* d_positions, uint64_t* d_hashes, uint8_t* d_kmers, uint64_t capacity, uint64_t* d_offsets,
                              uint64_t* d_result, void* d_workspace, uint64_t workspace_bytes, void* stream) {
    uint64_t ret = ~0ull;
    landing_void([&] {
        ret = find_kmers_run(reinterpret_cast<const KmerQuery*>(query), d_seq, len, d_starts, n_records, d_positions, d_hashes, d_kmers, capacity,
                             d_offsets, d_result, d_workspace, workspace_bytes, (hipStream_t)stream, nullptr);
    });
    return ret;
}

void smgpu_find_kmers_kernel_raw(const SmgpuKmerQuery* query, const uint8_t* d_seq, uint64_t len, uint64_t* d_hashes, uint64_t* d_positions,
                                 uint64_t capacity, uint64_t* d_count, uint32_t grid, void* stream) {
    landing_void([&] {
        const KmerQuery* q = reinterpret_cast<const KmerQuery*>(query);
        if (!q) throw err_internal("null query");
        if (q->mh.ksize < 1 || q->mh.ksize > 88) throw err_internal("k-mer finding takes ksize 1 .. 88, not " + std::to_string(q->mh.ksize));
        if (grid > (1u << 20)) throw err_internal("grid above 1048576 workgroups");
        const FindQuery dev = query_on_device(q);
        hip_check(find_pairs_launch(d_seq, len, q->mh.ksize, q->mh.seed, dev, d_hashes, d_positions, (unsigned long long*)d_count, capacity, grid,
                                    (hipStream_t)stream), "find_kmers");
    });
}

SmgpuKmerMatches* smgpu_find_kmers_file(const SmgpuKmerQuery* query, const char* path) {
    return landing<SmgpuKmerMatches*>([&]() -> SmgpuKmerMatches* {
        const KmerQuery* q = reinterpret_cast<const KmerQuery*>(query);
        if (!q || !path) throw err_internal("null argument");
        const uint32_t k = q->mh.ksize;
        if (k < 1 || k > 88) throw err_internal("k-mer finding takes ksize 1 .. 88, not " + std::to_string(k));
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        ParsedRecords pr;
        parse_records_file(path, pr, st);
        std::unique_ptr<KmerMatches> m(new KmerMatches());
        m->ksize = k;
        m->n_records = pr.n_records;
        m->names = std::move(pr.names);
        m->offsets.assign(pr.n_records + 1, 0);
        m->starts.assign(pr.n_records + 1, 0);
        m->lengths.assign(pr.n_records, 0);
        hip_check(hipMemcpyAsync(m->starts.data(), pr.starts.p, (pr.n_records + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
        // pairs the buffer is expected to match: the sketch's share of its positions, never more than the query could place
        AsyncBuf result(64, st), d_offsets((pr.n_records + 1) * 8 + 16, st);
        AsyncBuf d_pos, d_hash, d_kmers;
        m->n_rows = with_pair_capacity(records_pair_estimate(pr.len, q->mh.max_hash), [&](uint64_t cap, uint64_t* exceeded) {
            d_pos.reset(cap * 8 + 16, st); d_hash.reset(cap * 8 + 16, st); d_kmers.reset(cap * k + 16, st);
            const uint64_t ws_bytes = smgpu_find_kmers_workspace_bytes(cap, pr.n_records);
            AsyncBuf ws((size_t)ws_bytes, st);
            return find_kmers_run(q, pr.comp.as<uint8_t>(), pr.len, pr.starts.as<uint64_t>(), pr.n_records, d_pos.as<uint64_t>(), d_hash.as<uint64_t>(),
                                  d_kmers.as<uint8_t>(), cap, d_offsets.as<uint64_t>(), result.as<uint64_t>(), ws.p, ws_bytes, st, exceeded);
        });
        m->positions.resize(m->n_rows); m->hashes.resize(m->n_rows); m->kmers.resize(m->n_rows * k);
        hip_check(hipMemcpyAsync(m->offsets.data(), d_offsets.p, (pr.n_records + 1) * 8, hipMemcpyDeviceToHost, st), "D2H");
        if (m->n_rows) {
            hip_check(hipMemcpyAsync(m->positions.data(), d_pos.p, m->n_rows * 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipMemcpyAsync(m->hashes.data(), d_hash.p, m->n_rows * 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipMemcpyAsync(m->kmers.data(), d_kmers.p, m->n_rows * k, hipMemcpyDeviceToHost, st), "D2H");
            m->seq.resize(pr.len);
            if (pr.len) hip_check(hipMemcpyAsync(m->seq.data(), pr.comp.p, pr.len, hipMemcpyDeviceToHost, st), "D2H");
        }
        hip_check(hipStreamSynchronize(st), "sync");
        // a record's bytes end in front of the next record's separator byte (fastx.hip keeps one per header line)
        for (uint64_t r = 0; r < pr.n_records; ++r) {
            const uint64_t span = m->starts[r + 1] - m->starts[r];
            m->lengths[r] = r + 1 < pr.n_records && span ? span - 1 : span;
            m->n_bases += m->lengths[r];
            for (uint64_t i = m->offsets[r]; i < m->offsets[r + 1]; ++i) m->positions[i] -= m->starts[r];
        }
        return reinterpret_cast<SmgpuKmerMatches*>(m.release());
    });
}

void smgpu_kmermatches_free(SmgpuKmerMatches* p) { delete reinterpret_cast<KmerMatches*>(p); }
uint64_t smgpu_kmermatches_n_records(const SmgpuKmerMatches* p) { return reinterpret_cast<const KmerMatches*>(p)->n_records; }
uint64_t smgpu_kmermatches_n_rows(const SmgpuKmerMatches* p) { return reinterpret_cast<const KmerMatches*>(p)->n_rows; }
uint64_t smgpu_kmermatches_n_bases(const SmgpuKmerMatches* p) { return reinterpret_cast<const KmerMatches*>(p)->n_bases; }
const uint64_t* smgpu_kmermatches_offsets(const SmgpuKmerMatches* p) { return reinterpret_cast<const KmerMatches*>(p)->offsets.data(); }
const uint64_t* smgpu_kmermatches_positions(const SmgpuKmerMatches* p) { return reinterpret_cast<const KmerMatches*>(p)->positions.data(); }
const uint64_t* smgpu_kmermatches_hashes(const SmgpuKmerMatches* p) { return reinterpret_cast<const KmerMatches*>(p)->hashes.data(); }
const uint8_t* smgpu_kmermatches_kmers(const SmgpuKmerMatches* p) { return reinterpret_cast<const KmerMatches*>(p)->kmers.data(); }
const uint64_t* smgpu_kmermatches_record_lengths(const SmgpuKmerMatches* p) { return reinterpret_cast<const KmerMatches*>(p)->lengths.data(); }
SourmashStr smgpu_kmermatches_record_name(const SmgpuKmerMatches* p, uint64_t record) {
    return landing<SourmashStr>([&]() -> SourmashStr {
        const KmerMatches* m = reinterpret_cast<const KmerMatches*>(p);
        if (record >= m->n_records) throw err_internal("record " + std::to_string(record) + " of " + std::to_string(m->n_records));
        return make_str(m->names[record]);
    });
}
const uint8_t* smgpu_kmermatches_record_sequence(const SmgpuKmerMatches* p, uint64_t record, uint64_t* len) {
    const KmerMatches* m = reinterpret_cast<const KmerMatches*>(p);
    if (len) *len = 0;
    if (record >= m->n_records || m->offsets[record] == m->offsets[record + 1] || m->seq.empty()) return nullptr;
    if (len) *len = m->lengths[record];
    return m->seq.data() + m->starts[record];
}

}  // extern "C"
