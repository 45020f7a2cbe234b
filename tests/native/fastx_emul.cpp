// Host emulation of the FASTA / FASTQ parser (test-only artefact): sourmash_amd/csrc/fastx_core.hpp compiled for the CPU and walked as
// fastx.hip's three kernels walk it -- summary, offsets, scatter -- with a lane as a loop index, a wavefront as 64 of them and a
// block as 256.  The scans keep the kernels' shapes: shuffles inside a wavefront and a fold over the four wave totals in a block;
// 1,024 spans of per = ceil(n_blocks / 1024) blocks and Hillis-Steele steps in the offsets walk.  tests/test_fastx_core_cpu.py
// compares it with a per-line reference; with -DFASTX_EMUL_MAIN it is a stand-alone program for the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "../../sourmash_amd/csrc/fastx_core.hpp"

namespace {

using namespace smg;

// block_excl: the exclusive scan of a block's 256 lane values and the inclusive value of the last lane
template <bool LASTNZ>
uint32_t block_excl(const uint32_t (&v)[FX_THREADS], uint32_t (&excl)[FX_THREADS]) {
    uint32_t incl[FX_THREADS], s_wave[FX_THREADS / 64];
    for (int t = 0; t < FX_THREADS; ++t) incl[t] = v[t];
    for (int w = 0; w < FX_THREADS / 64; ++w) {
        for (int d = 1; d < 64; d <<= 1) {
            uint32_t o[64];
            for (int l = 0; l < 64; ++l) o[l] = incl[w * 64 + (l >= d ? l - d : l)];        // __shfl_up
            for (int l = d; l < 64; ++l) incl[w * 64 + l] = fx_fold<LASTNZ>(o[l], incl[w * 64 + l]);
        }
        s_wave[w] = incl[w * 64 + 63];
    }
    uint32_t all = 0;
    for (int w = 0; w < FX_THREADS / 64; ++w) all = fx_fold<LASTNZ>(all, s_wave[w]);
    for (int t = 0; t < FX_THREADS; ++t) {
        const int lane = t & 63, wave = t >> 6;
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w) before = fx_fold<LASTNZ>(before, s_wave[w]);
        const uint32_t prev = lane ? incl[t - 1] : 0u;
        excl[t] = fx_fold<LASTNZ>(before, prev);
    }
    return all;
}

uint32_t block_sum(const uint32_t (&v)[FX_THREADS]) {
    uint32_t t = 0;
    for (int i = 0; i < FX_THREADS; ++i) t += v[i];
    return t;
}

struct Lane { LaneBits b; uint8_t bytes[FX_PER_THREAD]; };

void load_block(const uint8_t* raw, uint64_t n, uint64_t block, uint8_t prev_nl_at_0, Lane (&L)[FX_THREADS]) {
    for (int t = 0; t < FX_THREADS; ++t) {
        const uint64_t base = block * FX_BLOCK_BYTES + (uint64_t)t * FX_PER_THREAD;
        L[t].b = lane_bits(raw, base, n, prev_nl_at_0, L[t].bytes);
    }
}

void summary_block(const uint8_t* raw, uint64_t n, int fastq, const uint8_t* carry, uint64_t block, BlockSum* sums) {
    static Lane L[FX_THREADS];
    load_block(raw, n, block, carry[1], L);
    BlockSum out{};
    uint32_t v[FX_THREADS], ex[FX_THREADS];
    if (!fastq) {
        uint32_t m1[FX_THREADS], m2[FX_THREADS], local[FX_THREADS], pre[FX_THREADS], h[FX_THREADS];
        for (int t = 0; t < FX_THREADS; ++t) fasta_masks(L[t].b, &m1[t], &m2[t], &v[t]);
        out.last_kind = block_excl<true>(v, ex);
        for (int t = 0; t < FX_THREADS; ++t) {
            local[t] = ex[t] == 1 ? fx_popc(m1[t]) : fx_popc(m2[t]);
            pre[t] = ex[t] == 0 ? fx_popc(m1[t] & ~m2[t]) : 0u;
            h[t] = fx_popc(L[t].b.ls & L[t].b.gt);
        }
        out.cnt[0] = block_sum(local); out.cnt[1] = block_sum(pre); out.hdr[0] = block_sum(h);
    } else {
        static uint32_t M[FX_THREADS][4];
        for (int t = 0; t < FX_THREADS; ++t) { fastq_classes(L[t].b, M[t]); v[t] = fx_popc(L[t].b.ls); }
        out.starts = block_excl<false>(v, ex);
        for (uint32_t p = 0; p < 4; ++p) {
            uint32_t c[FX_THREADS], h[FX_THREADS];
            for (int t = 0; t < FX_THREADS; ++t) {
                uint32_t hm;
                c[t] = fx_popc(fastq_keep(L[t].b, M[t], (p + ex[t]) & 3u, &hm));
                h[t] = fx_popc(hm);
            }
            out.cnt[p] = block_sum(c); out.hdr[p] = block_sum(h);
        }
    }
    sums[block] = out;
}

// Hillis-Steele inclusive scan over the 1,024 spans, every step reading the values of the step before (the barriers)
template <class T, class F>
void hillis_steele(T (&a)[FX_SPANS], F fold) {
    T nxt[FX_SPANS];
    for (int d = 1; d < FX_SPANS; d <<= 1) {
        for (int t = 0; t < FX_SPANS; ++t) nxt[t] = fold(t >= d ? a[t - d] : (T)0, a[t]);
        memcpy(a, nxt, sizeof(a));
    }
}

void offsets_walk(const BlockSum* sums, unsigned n_blocks, int fastq, const uint8_t* raw, uint64_t n, const uint8_t* carry, uint8_t* carry_out,
                  uint8_t* entry, unsigned long long* block_off, unsigned long long* total, unsigned long long* n_records,
                  unsigned long long* block_rec) {
    static unsigned long long part[FX_SPANS], kept[FX_SPANS], recs[FX_SPANS];
    static uint32_t st[FX_SPANS];
    const unsigned per = (n_blocks + FX_SPANS - 1) / FX_SPANS;
    auto lo_of = [&](unsigned t) { return t * per; };
    auto hi_of = [&](unsigned t) { return t * per + per < n_blocks ? t * per + per : n_blocks; };
    for (unsigned t = 0; t < (unsigned)FX_SPANS; ++t) {
        uint32_t eff = 0;
        for (unsigned i = lo_of(t); i < hi_of(t); ++i) {
            if (fastq) eff = fx_fold<false>(eff, sums[i].starts);
            else eff = fx_fold<true>(eff, sums[i].last_kind);
        }
        st[t] = eff;
    }
    if (fastq) hillis_steele(st, [](uint32_t v, uint32_t mine) { return fx_fold<false>(v, mine); });
    else hillis_steele(st, [](uint32_t v, uint32_t mine) { return fx_fold<true>(v, mine); });
    for (unsigned t = 0; t < (unsigned)FX_SPANS; ++t) {
        const unsigned lo = lo_of(t), hi = hi_of(t);
        uint32_t e = fx_entry_state(fastq, carry, t ? st[t - 1] : 0u);
        kept[t] = recs[t] = 0;
        for (unsigned i = lo; i < hi; ++i) {
            const BlockSum* s = sums + i;
            entry[i] = (uint8_t)e;
            if (fastq) fx_block_step<true>(s, e, kept[t], recs[t]); else fx_block_step<false>(s, e, kept[t], recs[t]);
        }
        if (hi == n_blocks && lo < hi) {
            carry_out[0] = (uint8_t)e;
            carry_out[1] = fx_ended_on_lf(raw[n - 1]);
        }
    }
    auto add = [](unsigned long long v, unsigned long long mine) { return mine + v; };
    memcpy(part, kept, sizeof(part));
    hillis_steele(part, add);
    for (unsigned t = 0; t < (unsigned)FX_SPANS; ++t) {
        unsigned long long run = t ? part[t - 1] : 0;
        for (unsigned i = lo_of(t); i < hi_of(t); ++i) {
            block_off[i] = run;
            run += fx_block_kept(sums + i, fastq, entry[i]);
        }
    }
    *total = part[FX_SPANS - 1];
    memcpy(part, recs, sizeof(part));
    for (int d = FX_SPANS / 2; d > 0; d >>= 1)
        for (int t = 0; t < d; ++t) part[t] += part[t + d];
    if (part[0]) *n_records += part[0];
    if (!block_rec) return;
    memcpy(part, recs, sizeof(part));
    hillis_steele(part, add);
    for (unsigned t = 0; t < (unsigned)FX_SPANS; ++t) {
        unsigned long long ord = t ? part[t - 1] : 0;
        for (unsigned i = lo_of(t); i < hi_of(t); ++i) {
            block_rec[i] = ord;
            ord += fx_block_records(sums + i, fastq, entry + i);
        }
    }
}

void scatter_block(const uint8_t* raw, uint64_t n, int fastq, const uint8_t* carry, const uint8_t* entry, const unsigned long long* block_off,
                   uint8_t* out, const unsigned long long* block_rec, unsigned long long* rec_starts, uint64_t rec_cap, uint64_t block) {
    static Lane L[FX_THREADS];
    static uint8_t s_out[FX_BLOCK_BYTES];
    load_block(raw, n, block, carry[1], L);
    const uint32_t e = entry[block];
    uint32_t mask[FX_THREADS], hdr[FX_THREADS], v[FX_THREADS], ex[FX_THREADS], pos[FX_THREADS], hpos[FX_THREADS];
    if (!fastq) {
        uint32_t m1[FX_THREADS], m2[FX_THREADS];
        for (int t = 0; t < FX_THREADS; ++t) fasta_masks(L[t].b, &m1[t], &m2[t], &v[t]);
        block_excl<true>(v, ex);
        for (int t = 0; t < FX_THREADS; ++t) {
            mask[t] = (ex[t] ? ex[t] : e) == 1u ? m1[t] : m2[t];
            hdr[t] = L[t].b.ls & L[t].b.gt;
        }
    } else {
        static uint32_t M[FX_THREADS][4];
        for (int t = 0; t < FX_THREADS; ++t) { fastq_classes(L[t].b, M[t]); v[t] = fx_popc(L[t].b.ls); }
        block_excl<false>(v, ex);
        for (int t = 0; t < FX_THREADS; ++t) mask[t] = fastq_keep(L[t].b, M[t], (e + ex[t]) & 3u, &hdr[t]);
    }
    for (int t = 0; t < FX_THREADS; ++t) v[t] = fx_popc(mask[t]);
    const uint32_t total = block_excl<false>(v, pos);
    if (rec_starts) {
        for (int t = 0; t < FX_THREADS; ++t) v[t] = fx_popc(hdr[t]);
        block_excl<false>(v, hpos);
        for (int t = 0; t < FX_THREADS; ++t) {
            unsigned long long ord = block_rec[block] + hpos[t];
            const unsigned long long at = block_off[block] + pos[t];
            for (uint32_t h = hdr[t]; h; h &= h - 1u, ++ord) {
                const uint32_t below = (h & (0u - h)) - 1u;
                if (ord < rec_cap) rec_starts[ord] = fx_record_start(at, mask[t], below);
            }
        }
    }
    for (int t = 0; t < FX_THREADS; ++t) {
        unsigned p = pos[t];
        for (int j = 0; j < FX_PER_THREAD; ++j)
            if (mask[t] & (1u << j)) s_out[p++] = L[t].bytes[j];
    }
    memcpy(out + block_off[block], s_out, total);
}

// fastx_compact_launch: carry[0, 2) in, carry[2, 4) out, copied forward unless last_piece; an empty piece only zeroes *n_out
void compact(const uint8_t* raw, uint64_t n, int fastq, uint8_t* carry, uint8_t* out, unsigned long long* n_out, unsigned long long* n_records,
             bool last_piece, unsigned long long* rec_starts, uint64_t rec_cap) {
    if (n == 0) { *n_out = 0; return; }
    const uint64_t n_blocks = (n + FX_BLOCK_BYTES - 1) / FX_BLOCK_BYTES;
    std::vector<BlockSum> sums(n_blocks);
    std::vector<uint8_t> entry(n_blocks);
    std::vector<unsigned long long> block_off(n_blocks), block_rec(n_blocks);
    for (uint64_t b = 0; b < n_blocks; ++b) summary_block(raw, n, fastq, carry, b, sums.data());
    offsets_walk(sums.data(), (unsigned)n_blocks, fastq, raw, n, carry, carry + 2, entry.data(), block_off.data(), n_out, n_records,
                 rec_starts ? block_rec.data() : nullptr);
    for (uint64_t b = 0; b < n_blocks; ++b)
        scatter_block(raw, n, fastq, carry, entry.data(), block_off.data(), out, block_rec.data(), rec_starts, rec_cap, b);
    if (!last_piece) memcpy(carry, carry + 2, 2);
}

}  // namespace

// One piece.  carry: 4 bytes, [0, 2) in; behind the call [0, 2) is the carry for the next piece (an empty piece leaves it alone).
// out: room for n bytes; starts: room for `cap` entries (may be null with cap 0); result: {kept, records seen by this piece}.
extern "C" void fastx_emul_piece(const uint8_t* raw, uint64_t n, int fastq, uint8_t* carry, uint8_t* out, uint64_t* starts, uint64_t cap,
                                 uint64_t* result) {
    unsigned long long kept = 0, recs = 0;
    // the parser never reads outside the piece: a copy of exactly n bytes, so that a sanitizer sees a read in front of or behind it
    std::vector<uint8_t> copy(raw, raw + n);
    compact(copy.data(), n, fastq, carry, out, &kept, &recs, false, reinterpret_cast<unsigned long long*>(starts), cap);
    result[0] = kept; result[1] = recs;
}

// A file cut at the given offsets (cuts[0] = 0 < ... <= cuts[n_cuts - 1] = n; equal neighbours make an empty piece), the carry
// chained: bytes concatenated into out, every piece's starts shifted by the bytes in front of it, the records summed.
extern "C" void fastx_emul_pieces(const uint8_t* raw, uint64_t n, int fastq, const uint64_t* cuts, uint64_t n_cuts, uint8_t* carry, uint8_t* out,
                                  uint64_t* starts, uint64_t cap, uint64_t* result) {
    uint64_t at = 0, recs = 0;
    std::vector<uint64_t> piece_starts;
    for (uint64_t c = 0; c + 1 < n_cuts; ++c) {
        const uint64_t len = cuts[c + 1] - cuts[c];
        uint64_t r[2] = {0, 0};
        piece_starts.assign(len + 1, 0);
        fastx_emul_piece(raw + cuts[c], len, fastq, carry, out + at, piece_starts.data(), len + 1, r);
        for (uint64_t j = 0; j < r[1]; ++j)
            if (recs + j < cap) starts[recs + j] = piece_starts[j] + at;
        at += r[0]; recs += r[1];
    }
    (void)n;
    result[0] = at; result[1] = recs;
}

#ifdef FASTX_EMUL_MAIN
// fastx_emul CASEFILE: records of
//   u64 n, u64 fastq, u64 n_cuts, u64 cap, u64 want_kept, u64 want_records, u8 want_carry[2] + 6 pad,
//   raw[n], cuts[n_cuts] u64, want_bytes[want_kept], want_starts[min(cap, want_records)] u64      (every array padded to 8 bytes)
// n_cuts == 0: the file as one piece.  The starts array holds exactly `cap` entries; those at and behind want_records must stay as they were.
// Exit status 0 when every record agrees, 1 at the first that does not.
static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }
static size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t h[7];
    unsigned long done = 0;
    while (rd(f, h, sizeof(h))) {
        const uint64_t n = h[0], fastq = h[1], n_cuts = h[2], cap = h[3], want_kept = h[4], want_recs = h[5];
        uint8_t want_carry[2];
        memcpy(want_carry, &h[6], 2);
        const uint64_t n_starts = cap < want_recs ? cap : want_recs;
        std::vector<uint8_t> raw(pad8(n)), want(pad8(want_kept)), out(n);
        std::vector<uint64_t> cuts(n_cuts), want_starts(n_starts);
        if (!rd(f, raw.data(), raw.size()) || !rd(f, cuts.data(), n_cuts * 8) || !rd(f, want.data(), want.size()) ||
            !rd(f, want_starts.data(), n_starts * 8)) { fprintf(stderr, "case %lu: truncated case file\n", done); return 2; }
        raw.resize(n);
        uint8_t carry[4] = {(uint8_t)(fastq ? 3 : 1), 1, 0, 0};
        uint64_t r[2] = {0, 0};
        std::unique_ptr<uint64_t[]> exact(new uint64_t[cap]);                        // exactly `cap` entries: a write behind them is out of bounds
        for (uint64_t j = 0; j < cap; ++j) exact[j] = 0xA5A5A5A5A5A5A5A5ull;
        if (n_cuts) fastx_emul_pieces(raw.data(), n, (int)fastq, cuts.data(), n_cuts, carry, out.data(), exact.get(), cap, r);
        else fastx_emul_piece(raw.data(), n, (int)fastq, carry, out.data(), exact.get(), cap, r);
        bool ok = r[0] == want_kept && r[1] == want_recs && carry[0] == want_carry[0] && carry[1] == want_carry[1];
        ok = ok && (!want_kept || memcmp(out.data(), want.data(), want_kept) == 0) && (!n_starts || memcmp(exact.get(), want_starts.data(), n_starts * 8) == 0);
        for (uint64_t j = n_starts; j < cap; ++j) ok = ok && exact[j] == 0xA5A5A5A5A5A5A5A5ull;
        if (!ok) {
            fprintf(stderr, "case %lu differs: kept %llu (want %llu), records %llu (want %llu), carry {%u, %u} (want {%u, %u})\n", done,
                    (unsigned long long)r[0], (unsigned long long)want_kept, (unsigned long long)r[1], (unsigned long long)want_recs, carry[0], carry[1],
                    want_carry[0], want_carry[1]);
            return 1;
        }
        ++done;
    }
    fclose(f);
    printf("fastx ok: %lu cases\n", done);
    return 0;
}
#endif
