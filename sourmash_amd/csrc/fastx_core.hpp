// fastx_core.hpp -- the per-lane and per-block rules of the FASTA / FASTQ parser (fastx.hip), host + device.
//
// The format statement and the three kernels are in fastx.hip.  What is here has no thread index in it: what a lane makes of its 32
// bytes, how two neighbouring spans' effects on the line state fold into one, what a block does to the state that enters it, and
// the two values a piece leaves behind.  On the device a lane is a thread; tests/native/fastx_emul.cpp walks the same functions
// with lanes as loop indices.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef SMG_HD
#if defined(__HIPCC__)
#define SMG_HD __host__ __device__ __forceinline__
#else
#define SMG_HD inline
#endif
#endif

namespace smg {

constexpr int FX_THREADS = 256;
constexpr int FX_PER_THREAD = 32;                              // consecutive bytes per lane (two 16-byte loads)
constexpr int FX_BLOCK_BYTES = FX_THREADS * FX_PER_THREAD;     // 8 KiB per workgroup
constexpr int FX_SPANS = 1024;                                 // threads of fx_offsets_kernel: each owns a span of consecutive blocks

SMG_HD uint32_t fx_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}
SMG_HD int fx_clz(uint32_t v) {                                // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz(v);
#else
    return __builtin_clz(v);
#endif
}

// what a block does to the state that enters it, and what it keeps as a function of that state
struct BlockSum {
    uint32_t cnt[4];     // FASTA: [0] kept bytes whatever enters, [1] more if a sequence line enters; FASTQ: kept bytes by entry phase
    uint32_t hdr[4];     // FASTA: [0] header lines; FASTQ: header lines by entry phase
    uint32_t starts;     // FASTQ: line starts in the block
    uint32_t last_kind;  // FASTA: kind of the block's last line start (0: none)
};

// a lane's 32 bytes, all of them inside the piece; raw + base is 16-byte aligned on the device (fastx_api.hpp)
SMG_HD void fx_load_lane(const uint8_t* __restrict__ raw, uint64_t base, uint8_t* bytes) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 r0 = *reinterpret_cast<const uint4*>(raw + base), r1 = *reinterpret_cast<const uint4*>(raw + base + 16);
    memcpy(bytes, &r0, 16); memcpy(bytes + 16, &r1, 16);
#else
    memcpy(bytes, raw + base, FX_PER_THREAD);
#endif
}

// A lane's 32 bytes.  ls / nl / gt: bit j = byte j starts a line / is CR or LF / is '>'; bits at and above the lane's valid bytes are 0.
struct LaneBits { uint32_t ls, nl, gt, valid; };
SMG_HD LaneBits lane_bits(const uint8_t* __restrict__ raw, uint64_t base, uint64_t n, uint8_t prev_nl_at_0, uint8_t* bytes) {
    LaneBits b{0, 0, 0, 0};
    if (base >= n) return b;
    if (base + FX_PER_THREAD <= n) {
        fx_load_lane(raw, base, bytes);
        b.valid = 0xffffffffu;
    } else {
        const int lim = (int)(n - base);
        for (int j = 0; j < FX_PER_THREAD; ++j) bytes[j] = j < lim ? raw[base + j] : (uint8_t)'\n';
        b.valid = (1u << lim) - 1u;                              // lim in 1 .. 31
    }
    bool prev_nl = base ? raw[base - 1] == '\n' : prev_nl_at_0 != 0;
#pragma unroll
    for (int j = 0; j < FX_PER_THREAD; ++j) {
        const uint8_t c = bytes[j];
        b.ls |= prev_nl ? (1u << j) : 0u;
        b.nl |= (c == '\n' || c == '\r') ? (1u << j) : 0u;
        b.gt |= c == '>' ? (1u << j) : 0u;
        prev_nl = c == '\n';
    }
    b.ls &= b.valid; b.nl &= b.valid; b.gt &= b.valid;
    return b;
}

// FASTA: keep masks of a lane if a header line (m2) / a sequence line (m1) enters it; kind of its last line start (0: none)
SMG_HD void fasta_masks(const LaneBits& b, uint32_t* m1, uint32_t* m2, uint32_t* last_kind) {
    uint32_t keep = 0, on_seq = 0;
    bool seq = false;                                              // entering on a header line: nothing kept before the first line start
#pragma unroll
    for (int j = 0; j < FX_PER_THREAD; ++j) {
        const uint32_t bit = 1u << j;
        if (b.ls & bit) seq = !(b.gt & bit);
        on_seq |= seq ? bit : 0u;
    }
    const uint32_t hs = b.ls & b.gt;
    keep = hs | (on_seq & ~b.nl & b.valid);
    const uint32_t before_first = b.ls ? ((b.ls & (0u - b.ls)) - 1u) : 0xffffffffu;    // bits below the first line start
    *m2 = keep;
    *m1 = keep | (before_first & ~b.nl & b.valid);
    *last_kind = b.ls ? ((hs >> (31 - fx_clz(b.ls))) & 1u ? 2u : 1u) : 0u;
}

// FASTQ: M[t] = bytes whose line number within the lane is t mod 4 (counting the lane's own line starts up to and including the byte)
SMG_HD void fastq_classes(const LaneBits& b, uint32_t (&M)[4]) {
    M[0] = M[1] = M[2] = M[3] = 0;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < FX_PER_THREAD; ++j) {
        const uint32_t bit = 1u << j;
        c += (b.ls >> j) & 1u;
        const uint32_t t = c & 3u;
        M[0] |= t == 0 ? bit : 0u; M[1] |= t == 1 ? bit : 0u; M[2] |= t == 2 ? bit : 0u; M[3] |= t == 3 ? bit : 0u;
    }
}
// keep mask / header starts of a lane entered in phase q (the state of the byte in front of it, mod 4)
SMG_HD uint32_t fastq_keep(const LaneBits& b, const uint32_t (&M)[4], uint32_t q, uint32_t* headers) {
    const uint32_t hl = M[(4u - q) & 3u], sl = M[(5u - q) & 3u];       // header line: q + t = 0, sequence line: q + t = 1 (mod 4)
    *headers = hl & b.ls;
    return (hl & b.ls) | (sl & ~b.nl & b.valid);
}

// The two fold rules: the effect on the line state of a span followed by another.  FASTA (LASTNZ): the kind of the last line
// start, so the later span's if it has one; FASTQ: the number of line starts, a sum (taken mod 4 where it is used).
template <bool LASTNZ>
SMG_HD uint32_t fx_fold(uint32_t earlier, uint32_t later) { return LASTNZ ? (later ? later : earlier) : earlier + later; }

// the state in front of a span: the carry's state with the effect of everything before the span folded in
// (carry[0] is read only where it is needed: a FASTA span behind a line start does not depend on it)
SMG_HD uint32_t fx_entry_state(int fastq, const uint8_t* carry, uint32_t before) {
    return fastq ? (uint32_t)((carry[0] + before) & 3u) : (before ? before : (uint32_t)carry[0]);
}

// The per-block step of the offsets walk: the state e that enters block *s -> what the block keeps, its records, the state behind
// it (fx_block_step); the first two again by themselves for the passes that know e already.
// (the summary is indexed in memory: a local copy indexed by the phase lands in scratch)
SMG_HD uint32_t fx_block_kept(const BlockSum* s, int fastq, uint32_t e) {
    return fastq ? s->cnt[e & 3u] : s->cnt[0] + (e == 1u ? s->cnt[1] : 0u);
}
// (*e is read only for FASTQ)
SMG_HD uint32_t fx_block_records(const BlockSum* s, int fastq, const uint8_t* e) { return fastq ? s->hdr[*e & 3u] : s->hdr[0]; }
template <bool FASTQ>
SMG_HD void fx_block_step(const BlockSum* s, uint32_t& e, unsigned long long& kept, unsigned long long& recs) {
    if (FASTQ) { kept += s->cnt[e & 3u]; recs += s->hdr[e & 3u]; e = (e + s->starts) & 3u; }
    else { const uint32_t lk = s->last_kind; kept += s->cnt[0] + (e == 1u ? s->cnt[1] : 0u); recs += s->hdr[0]; e = lk ? lk : e; }
}

// where the record of a kept header byte starts: just behind that byte.  at: output offset of the lane's first kept byte; mask: the
// lane's kept bytes; below: the bits below the header byte
SMG_HD unsigned long long fx_record_start(unsigned long long at, uint32_t mask, uint32_t below) { return at + fx_popc(mask & below) + 1u; }

// the second byte of the carry: the piece ended on LF, so the next piece's first byte starts a line
SMG_HD uint8_t fx_ended_on_lf(uint8_t last_byte) { return last_byte == '\n'; }

}  // namespace smg
