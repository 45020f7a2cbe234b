// Host emulation of the signature JSON array parser (test-only artefact): sourmash_amd/csrc/sigjson_core.hpp compiled for the CPU
// and walked as sigjson.hip's two kernels walk it -- a wavefront per document in the span scan, a wavefront per array in the
// number parser -- with a lane as a loop index.  The ballots, the __shfl_up prefix sum and the xor reduction are loops here.
// A document is copied into a buffer of exactly its length, the text block into one of exactly its length + SJ_TEXT_PAD at the
// address (mod 16) the caller names, and the chunk buffer is exactly as long as the kernel's LDS array: a read outside any of
// them is a sanitizer report.  tests/test_sigjson_core_cpu.py compares it with the reference of tests/sigjson_cases.py; with
// -DSIGJSON_EMUL_MAIN it is a stand-alone program for the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "../../sourmash_amd/csrc/sigjson_core.hpp"

namespace {

using namespace smg;

template <class Pred>
uint64_t ballot(Pred pred) {
    uint64_t m = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) m |= (uint64_t)(pred(lane) ? 1 : 0) << lane;
    return m;
}

template <class Pred>
uint64_t find_first(uint64_t from, uint64_t len, Pred pred) {
    for (uint64_t p = from; p < len; p += 64) {
        const uint64_t m = ballot([&](uint32_t lane) { return p + lane < len && pred(p + lane); });
        if (m) return p + (uint64_t)__builtin_ctzll(m);
    }
    return len;
}

// sj_spans_kernel, one document
void spans_doc(const uint8_t* t, uint64_t len, SjSpan* spans, uint32_t* doc_flags) {
    uint32_t n = 0, flags = 0;
    uint64_t pos = 0;
    while (pos < len) {
        const uint64_t m = find_first(pos, len, [&](uint64_t i) { return sj_key_at(t, i, len); });
        if (m >= len) break;
        const uint32_t kind = sj_key_kind(t, m);
        const uint64_t s = sj_array_begin(t, m + sj_key_len(kind), len);
        if (s > len) { pos = m + 1; continue; }
        uint64_t e = len;
        SjTally tally = {0, 0, 0};
        for (uint64_t p = s; p < len; p += 64) {
            SjByteClass c[64];
            for (uint32_t lane = 0; lane < 64; ++lane) c[lane] = sj_class_at(t, p + lane, len);
            const uint64_t close = ballot([&](uint32_t l) { return c[l].close; });
            sj_tile_fold(close, ballot([&](uint32_t l) { return c[l].comma; }), ballot([&](uint32_t l) { return c[l].digit; }),
                         ballot([&](uint32_t l) { return c[l].odd; }), tally);
            if (close) { e = p + (uint64_t)__builtin_ctzll(close); break; }
        }
        if (e >= len) { flags |= SJ_DOC_ODD; break; }
        if (n >= SJ_MAX_SPANS) { flags |= SJ_DOC_ODD; break; }
        spans[n] = sj_span_record(s, e, kind, tally);
        ++n;
        pos = e + 1;
    }
    *doc_flags = flags | n;
}

// sj_parse_kernel, one array.  block: the text block at its emulated address; block_addr: that address (only its low 4 bits matter)
void parse_job(const uint8_t* block, uint64_t block_addr, const SjParse& job, uint64_t* values, SjParsed* result, uint64_t keep_max) {
    std::unique_ptr<uint8_t[]> buf(new uint8_t[SJ_BUF_LINES * 16]);   // exactly the kernel's LDS array
    const uint64_t len = job.len;
    uint64_t* out = values + job.value_off;
    uint32_t bad[64] = {0};
    uint64_t index = 0;
    for (uint64_t c0 = 0; c0 < len; c0 += SJ_CHUNK) {
        const uint64_t addr = block_addr + job.text_off + c0;
        const SjChunkGeom g = sj_chunk_geom(addr, c0, len);
        const uint8_t* src = block + job.text_off + c0 - g.shift;     // (in front of the block's first byte when its address is not a line's)
        for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t l = lane; l < g.lines; l += 64u) memcpy(buf.get() + 16 * (size_t)l, src + 16 * (size_t)l, 16);
        const uint8_t* b = buf.get() + g.shift;
        uint32_t commas[64], incl[64];
        for (uint32_t lane = 0; lane < 64; ++lane) incl[lane] = commas[lane] = sj_lane_commas(b, sj_lane_begin(lane), sj_lane_end(lane, g.in_chunk));
        for (int o = 1; o < 64; o <<= 1) {
            uint32_t u[64];
            for (int l = 0; l < 64; ++l) u[l] = incl[l >= o ? l - o : l];                  // __shfl_up
            for (int l = o; l < 64; ++l) incl[l] += u[l];
        }
        const uint32_t chunk_commas = incl[63];
        uint64_t next = index;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const SjChunkIndex ix = sj_chunk_index(index, incl[lane], commas[lane], chunk_commas);
            sj_parse_lane(b, g, lane, c0, len, ix.lane_first, job.n_values, out, bad[lane]);
            next = ix.next;
        }
        index = next;
    }
    uint32_t kept[64] = {0};
    for (uint32_t lane = 0; lane < 64; ++lane) sj_order_lane(out, job.n_values, lane, keep_max, kept[lane], bad[lane]);
    for (int o = 32; o; o >>= 1) {                                    // __shfl_xor
        uint32_t k2[64], b2[64];
        for (int l = 0; l < 64; ++l) { k2[l] = kept[l ^ o]; b2[l] = bad[l ^ o]; }
        for (int l = 0; l < 64; ++l) { kept[l] += k2[l]; bad[l] |= b2[l]; }
    }
    result->n_kept = kept[0];
    result->flags = bad[0] ? SJ_SPAN_ODD : 0u;
}

}  // namespace

// docs: n_docs pairs (off, len) inside text[0, text_len); spans: n_docs * SJ_MAX_SPANS records (those not found are left alone); doc_flags: n_docs
extern "C" void sigjson_emul_spans(const uint8_t* text, uint64_t text_len, const uint64_t* docs, uint32_t n_docs, SjSpan* spans, uint32_t* doc_flags) {
    (void)text_len;
    for (uint32_t d = 0; d < n_docs; ++d) {
        std::vector<uint8_t> copy(text + docs[2 * d], text + docs[2 * d] + docs[2 * d + 1]);   // the scan stops at the document's len
        spans_doc(copy.data(), copy.size(), spans + (size_t)d * SJ_MAX_SPANS, doc_flags + d);
    }
}

// The text block as if its first byte stood at an address that is base_mod16 modulo 16, with SJ_TEXT_PAD bytes behind it.  On the
// device a block's allocation begins on a line, so the bytes between that line's start and the text exist: base_mod16 of them here.
extern "C" void sigjson_emul_parse(const uint8_t* text, uint64_t text_len, uint32_t base_mod16, const SjParse* jobs, uint32_t n_jobs, uint64_t* values,
                                   SjParsed* results, uint64_t keep_max) {
    base_mod16 &= 15u;
    const size_t size = (size_t)base_mod16 + text_len + SJ_TEXT_PAD;
    std::unique_ptr<uint8_t[]> blk(new uint8_t[size]);               // exactly: a read in front of or behind it is out of bounds
    memset(blk.get(), 0, size);
    memcpy(blk.get() + base_mod16, text, text_len);
    for (uint32_t j = 0; j < n_jobs; ++j) parse_job(blk.get() + base_mod16, base_mod16, jobs[j], values, results + j, keep_max);
}

#ifdef SIGJSON_EMUL_MAIN
// sigjson_emul CASEFILE: records of
//   u64 text_len, n_docs, base_mod16, keep_max, n_jobs, n_values,
//   text[text_len], docs[2 * n_docs] u64, want_spans[n_docs * SJ_MAX_SPANS], want_flags[n_docs] u32, jobs[n_jobs], want_values[n_values] u64,
//   want_parsed[n_jobs]                                                                             (every array padded to 8 bytes)
// Spans and values start out as bytes 0xA5, as the wanted ones did; the value array holds exactly n_values entries.
// Exit status 0 when every record agrees, 1 at the first that does not.
static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t h[6];
    unsigned long done = 0;
    while (fread(h, 1, sizeof(h), f) == sizeof(h)) {
        const uint64_t text_len = h[0], n_docs = h[1], base_mod16 = h[2], keep_max = h[3], n_jobs = h[4], n_values = h[5];
        std::vector<uint8_t> text(pad8(text_len));
        std::vector<uint64_t> docs(2 * n_docs), want_values(n_values);
        std::vector<SjSpan> want_spans(n_docs * SJ_MAX_SPANS), spans(n_docs * SJ_MAX_SPANS);
        std::vector<uint32_t> want_flags(pad8(n_docs * 4) / 4), flags(n_docs);
        std::vector<SjParse> jobs(n_jobs);
        std::vector<SjParsed> want_parsed(n_jobs), parsed(n_jobs);
        if (!rd(f, text.data(), text.size()) || !rd(f, docs.data(), docs.size() * 8) || !rd(f, want_spans.data(), want_spans.size() * sizeof(SjSpan)) ||
            !rd(f, want_flags.data(), want_flags.size() * 4) || !rd(f, jobs.data(), n_jobs * sizeof(SjParse)) || !rd(f, want_values.data(), n_values * 8) ||
            !rd(f, want_parsed.data(), n_jobs * sizeof(SjParsed))) { fprintf(stderr, "case %lu: truncated case file\n", done); return 2; }
        std::unique_ptr<uint8_t[]> exact_text(new uint8_t[text_len]);
        if (text_len) memcpy(exact_text.get(), text.data(), text_len);
        if (!spans.empty()) memset(spans.data(), 0xA5, spans.size() * sizeof(SjSpan));
        sigjson_emul_spans(exact_text.get(), text_len, docs.data(), (uint32_t)n_docs, spans.data(), flags.data());
        std::unique_ptr<uint64_t[]> values(new uint64_t[n_values]);  // exactly n_values entries: a write behind them is out of bounds
        if (n_values) memset(values.get(), 0xA5, n_values * 8);
        sigjson_emul_parse(exact_text.get(), text_len, (uint32_t)base_mod16, jobs.data(), (uint32_t)n_jobs, values.get(), parsed.data(), keep_max);
        const bool ok = (spans.empty() || memcmp(spans.data(), want_spans.data(), spans.size() * sizeof(SjSpan)) == 0) &&
                        (!n_docs || memcmp(flags.data(), want_flags.data(), n_docs * 4) == 0) &&
                        (!n_values || memcmp(values.get(), want_values.data(), n_values * 8) == 0) &&
                        (!n_jobs || memcmp(parsed.data(), want_parsed.data(), n_jobs * sizeof(SjParsed)) == 0);
        if (!ok) { fprintf(stderr, "case %lu differs\n", done); return 1; }
        ++done;
    }
    fclose(f);
    printf("sigjson ok: %lu cases\n", done);
    return 0;
}
#endif
