// Per-lane DNA k-mer -> canonical -> murmur -> keep logic of the sketch kernel.
//
// Replaces, for one run of P consecutive k-mer start positions:
//   src/core/src/signature.rs:189-233  SeqToHashes::new   (upper-casing, :214)
//   src/core/src/signature.rs:246-306  SeqToHashes::next  (revcomp :263, VALID scan :271-286,
//                                      canonical = min(kmer, krc) on ASCII :302-304, murmur)
//   src/core/src/encodings.rs:85-101,370-377  COMPLEMENT / VALID tables
//   src/core/src/signature.rs:38-58    add_sequence: skip hash 0, add the rest
//   src/core/src/sketch/minhash.rs:319  keep rule h <= max_hash
//
// Formulation (MI355X-first, nothing like the reference's byte loops):
// a lane owns P consecutive start positions and holds the P+K-1 ASCII bytes it
// needs as little-endian dwords in registers.  MurmurHash3 consumes the k-mer
// as little-endian 64-bit words, so
//   * the FORWARD k-mer's hash words are just byte-shifted views of the input
//     registers: one v_alignbyte_b32 per dword (none when the position is
//     dword aligned);
//   * the REVERSE-COMPLEMENT k-mer's words are byte-reversed views of the
//     complemented registers: one v_perm_b32 per dword does shift + reverse;
//   * complement and validity come from a 2-bit code ((c >> 1) & 3 maps
//     A,C,T,G -> 0,1,2,3 for both cases) fed to v_perm_b32 as a 4-entry LUT;
//   * canonical choice = big-endian compare of the first 8 bytes (2 bswaps a
//     side + one 64-bit compare); later bytes are looked at only if some lane
//     of the wave ties, which happens with probability 4^-8 per k-mer.
// No 2-bit packing, no per-base loops, no LDS traffic beyond the initial
// window read.  The murmur multiplies dominate (12 x 64-bit per k-mer).
//
// The same source compiles for the host (perm/alignbyte emulated) so the byte
// plumbing is checked against the oracle on CPU (tests/test_kmer_core_cpu.py)
// before it ever runs on a GPU.
#pragma once
#include "murmur3.hpp"
#include <utility>

namespace smg {

// ---- byte-permute primitives ------------------------------------------------
// perm_b32(hi, lo, sel): byte i of the result = byte sel.byte[i] of the 8-byte
// value {hi:lo} (0-3 -> lo, 4-7 -> hi); selector 0x0c yields 0x00.
SMG_HD uint32_t perm_b32(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = (sel >> (8 * i)) & 0xff;
        uint32_t b;
        if (s < 8) b = (uint32_t)(v >> (8 * s)) & 0xff;
        else if (s == 0x0c) b = 0;
        else b = 0xff;  // other special selectors are never used here
        r |= b << (8 * i);
    }
    return r;
#endif
}

// ({hi:lo} >> 8*n) truncated to 32 bits, n in 0..3
SMG_HD uint32_t alignbyte_b32(uint32_t hi, uint32_t lo, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, n);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * n));
#endif
}

SMG_HD bool any_lane(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(p) != 0ull;
#else
    return p;
#endif
}

// bitwise select: mask ? b : c  (v_bitop3_b32 is full rate on gfx950, v_cndmask_b32 is not)
SMG_HD uint32_t bitselect(uint32_t mask, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(mask, b, c, 0xCA);
#else
    return (mask & b) | (~mask & c);
#endif
}

// Make a value opaque to the optimiser at this point (keeps rare-path work inside its branch).
SMG_HD uint32_t opaque(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(x));
#endif
    return x;
}

SMG_HD uint32_t bswap32(uint32_t x) { return perm_b32(0u, x, 0x00010203u); }

// LUTs indexed by code = (ascii >> 1) & 3 :  A -> 0, C -> 1, T -> 2, G -> 3
constexpr uint32_t LUT_SELF = 'A' | ('C' << 8) | ('T' << 16) | ((uint32_t)'G' << 24);
constexpr uint32_t LUT_COMP = 'T' | ('G' << 8) | ('A' << 16) | ((uint32_t)'C' << 24);

template <int K, int P>
struct LaneGeom {
    static constexpr int NBYTES = P + K - 1;        // bytes a lane touches
    static constexpr int NW = (NBYTES + 3) / 4;     // dwords holding them
    static constexpr int NWK = (K + 3) / 4;         // dwords of one k-mer
    static constexpr int NCH = (K + 7) / 8;         // 8-byte chunks of one k-mer
    static constexpr uint32_t LAST_MASK = (K % 4) ? ((1u << (8 * (K % 4))) - 1u) : 0xffffffffu;
    // The last key dword holds K % 4 bytes.  Where a caller asks for the late mask (PosOps<.., LATE>), both strands' last
    // dwords are built whole and the chosen one is masked once, behind the strand select -- if there is a mask at all and the
    // last dword is no part of the first-8-bytes compare.
    static constexpr bool LATE_MASK_OK = (K % 4) != 0 && NWK > 2;
};

// selector for "4 bytes starting at byte a of {hi:lo}, reversed"
constexpr uint32_t rev_sel(int a) {
    return (uint32_t)(a + 3) | ((uint32_t)(a + 2) << 8) | ((uint32_t)(a + 1) << 16) | ((uint32_t)a << 24);
}
// selector for "nb (1..3) bytes starting at byte a, reversed, zero padded"
constexpr uint32_t rev_sel_partial(int a, int nb) {
    uint32_t s = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t b = (i < nb) ? (uint32_t)(a + nb - 1 - i) : 0x0cu;
        s |= b << (8 * i);
    }
    return s;
}

// One start position `O` (compile time) of the lane window.  LATE: the last key dword is masked behind the strand select (below);
// the same keys and hashes either way.  A kernel that would lose a wave per SIMD to it keeps the early mask, as with PLAIN.
template <int K, int P, int O, bool LATE = false>
struct PosOps {
    using G = LaneGeom<K, P>;
    static constexpr bool LATE_MASK = LATE && G::LATE_MASK_OK;

    // forward k-mer dword d: bytes O+4d .. O+4d+3 of the window
    template <int D>
    static SMG_HD uint32_t fwd(const uint32_t* U) {
        constexpr int q = (O >> 2) + D, a = O & 3;
        uint32_t v;
        if constexpr (a == 0) v = U[q];
        else if constexpr (q + 1 < G::NW) v = alignbyte_b32(U[q + 1], U[q], a);
        else v = U[q] >> (8 * a);
        if constexpr (D == G::NWK - 1 && !LATE_MASK) v &= G::LAST_MASK;
        return v;
    }

    // reverse-complement k-mer dword d: rc[j] = comp(win[O + K-1 - j]), j = 4d..4d+3
    // The last dword of a K % 4 != 0 holds nb < 4 bytes.  Under LATE_MASK it is taken whole where its 4 bytes lie inside the
    // window -- O + K - 4 D - 4 >= 0: the bytes in front of the k-mer fill its top, and that whole dword is one another position
    // of the lane builds anyway -- and hash_open masks it behind the select; a position whose whole dword would start in front
    // of the window keeps the zero-filling selector.
    template <int D>
    static SMG_HD uint32_t rev(const uint32_t* C) {
        constexpr int nbk = (K - 4 * D) >= 4 ? 4 : (K - 4 * D);  // valid bytes in this dword
        constexpr int nb = (LATE_MASK && O + K - 4 * D - 4 >= 0) ? 4 : nbk;
        constexpr int s = O + K - 4 * D - nb;                    // first window byte of the group
        constexpr int q = s >> 2, a = s & 3;
        constexpr uint32_t sel = (nb == 4) ? rev_sel(a) : rev_sel_partial(a, nb);
        if constexpr (q + 1 < G::NW) return perm_b32(C[q + 1], C[q], sel);
        else return perm_b32(0u, C[q], sel);
    }

    template <int CH>
    static SMG_HD uint64_t be_chunk(const uint32_t* W) {
        uint64_t v = (uint64_t)bswap32(W[2 * CH]) << 32;
        if constexpr (2 * CH + 1 < G::NWK) v |= bswap32(W[2 * CH + 1]);
        return v;
    }

    // (under LATE_MASK the strands' last dwords are unmasked: this path compares whole keys and masks its own copies)
    template <int D>
    static SMG_HD uint32_t key_dword_opaque(const uint32_t* W) {
        const uint32_t v = opaque(W[D]);
        if constexpr (D == G::NWK - 1 && LATE_MASK) return v & G::LAST_MASK;
        else return v;
    }
    template <int CH>
    static SMG_HD uint64_t be_chunk_opaque(const uint32_t* W) {
        uint64_t v = (uint64_t)bswap32(key_dword_opaque<2 * CH>(W)) << 32;
        if constexpr (2 * CH + 1 < G::NWK) v |= bswap32(key_dword_opaque<2 * CH + 1>(W));
        return v;
    }

    // Rare path (some lane's first 8 bytes tie): the operands are laundered through `opaque` so
    // the compiler cannot hoist these byte swaps out of the branch and run them for every k-mer.
    template <int CH>
    static SMG_HD void tie_break(const uint32_t* F, const uint32_t* R, bool& tie, bool& gt) {
        if constexpr (CH < G::NCH) {
            const uint64_t bf = be_chunk_opaque<CH>(F), br = be_chunk_opaque<CH>(R);
            gt = gt || (tie && bf > br);
            tie = tie && (bf == br);
            tie_break<CH + 1>(F, R, tie, gt);
        }
    }

    template <int... D>
    static SMG_HD void build(const uint32_t* U, const uint32_t* C, uint32_t* F, uint32_t* R,
                             std::integer_sequence<int, D...>) {
        ((F[D] = fwd<D>(U)), ...);
        ((R[D] = rev<D>(C)), ...);
    }

    // hash of the canonical k-mer at this position, last fmix64 multiplies left open (murmur3.hpp)
    template <bool PLAIN = false>
    static SMG_HD Mmh3Open hash_open(const uint32_t* U, const uint32_t* C, uint64_t seed) {
        uint32_t F[G::NWK], R[G::NWK];
        build(U, C, F, R, std::make_integer_sequence<int, G::NWK>{});
        const uint64_t bf = be_chunk<0>(F), br = be_chunk<0>(R);
        bool gt = bf > br;          // forward string > revcomp string -> take revcomp
        bool tie = bf == br;
        if (G::NCH > 1 && any_lane(tie)) tie_break<1>(F, R, tie, gt);
        uint32_t W[G::NWK];
        const uint32_t m = gt ? 0xffffffffu : 0u;
#pragma unroll
        for (int d = 0; d < G::NWK; ++d) W[d] = bitselect(m, R[d], F[d]);
        if constexpr (LATE_MASK) W[G::NWK - 1] &= G::LAST_MASK;    // one mask for both strands
        return mmh3_open_words<K, PLAIN>(W, seed);
    }
};

// Expand a nonzero-byte pattern of a dword into 4 bits (bit i = byte i != 0).
SMG_HD uint32_t nonzero_bytes4(uint32_t x) {
    uint32_t t = x | (x >> 4);
    t |= t >> 2;
    t |= t >> 1;
    t &= 0x01010101u;
    return (t * 0x01020408u) >> 24 & 0xfu;
}

// The early reject of process_lane.  The top dword t of a kept hash satisfies t <= thr >> 32 = thr_hi, and the open form knows
// s in {t - 1, t, t + 1} (mod 2^32, mmh3_close_hi_sum).  (s + 1) mod 2^32 is then t, t + 1 or t + 2: at most thr_hi + 2 whenever
// t <= thr_hi (t = 0 with s = 2^32 - 1 wraps to 0, which passes).  Where thr_hi + 2 would wrap every k-mer is finished.
SMG_HD uint32_t early_limit(uint64_t thr) {
    const uint32_t thr_hi = (uint32_t)(thr >> 32);
    return thr_hi >= 0xfffffffdu ? 0xffffffffu : thr_hi + 2u;
}
// false only if mmh3_close(open) > thr
SMG_HD bool early_may_keep(Mmh3Open open, uint32_t lim) { return (uint32_t)(mmh3_close_hi_sum(open) + 1u) <= lim; }

// Process the P start positions of one lane: the one copy of the validity and position code, behind process_lane and
// process_lane_staged below.
//   STAGED == false: raw[NW] holds the lane's window bytes as little-endian dwords (any case, any junk; bytes past the end of the
//                    sequence must be non-ACGT, e.g. 0); they are upper-cased, complemented and checked here.
//   STAGED == true : raw is the window already upper-cased, comp its complement (stage_chunk, where the tile is staged); `dirty`
//                    says whether the tile holds an invalid byte at all, and only then is the window checked.
//   thr      : keep iff 1 <= h <= thr   (thr = max_hash, or 2^64-1 for num sketches)
//   emit(o,h): called for every kept k-mer (o = position within the lane's run)
// The two prologues and the positions sit in ONE function on purpose: with the prologue in one function and the positions in
// another the compiler pairs the window's LDS reads differently, and sketch_dna_kernel<18, 16, false> (96 -> 98 VGPRs) and
// hll_dna_kernel<19, 16, true> (80 -> 82) each lose a wave per SIMD.
template <int K, int P, bool EARLY, bool PLAIN, bool STAGED, bool LATE, class Emit, int... O>
SMG_HD void process_window(const uint32_t* raw, const uint32_t* comp, bool dirty, uint64_t seed, uint64_t thr, Emit&& emit,
                           std::integer_sequence<int, O...>) {
    using G = LaneGeom<K, P>;
    const uint32_t lim = early_limit(thr);
    uint32_t Ubuf[STAGED ? 1 : G::NW], Cbuf[STAGED ? 1 : G::NW];
    const uint32_t* U = STAGED ? raw : Ubuf;
    const uint32_t* C = STAGED ? comp : Cbuf;
    uint32_t anybad = 0;
    if constexpr (!STAGED) {
#pragma unroll
        for (int i = 0; i < G::NW; ++i) {
            const uint32_t u = raw[i] & 0xdfdfdfdfu;             // upper-case (signature.rs:214)
            const uint32_t code = (u >> 1) & 0x03030303u;
            Ubuf[i] = u;
            Cbuf[i] = perm_b32(0u, LUT_COMP, code);              // encodings.rs:85-101
            uint32_t bad = perm_b32(0u, LUT_SELF, code) ^ u;     // != 0 where byte not in ACGT (encodings.rs:370-377)
            if (i == G::NW - 1 && (G::NBYTES % 4) != 0)          // ignore slack bytes past the lane's window
                bad &= (1u << (8 * (G::NBYTES % 4))) - 1u;
            anybad |= bad;
        }
    }
    // bit b of (badlo, badhi, badtop) = window byte b is invalid (192 bits: k <= 128 at P = 16 ... 64).  Rare: built only if needed.
    uint64_t badlo = 0, badhi = 0, badtop = 0;
    if (!STAGED || dirty) {                                      // (dirty MUST be wave-uniform on the device)
        if constexpr (STAGED) {
#pragma unroll
            for (int i = 0; i < G::NW; ++i) {
                const uint32_t u = U[i];
                uint32_t bad = perm_b32(0u, LUT_SELF, (u >> 1) & 0x03030303u) ^ u;
                if (i == G::NW - 1 && (G::NBYTES % 4) != 0)      // ignore slack bytes past the lane's window
                    bad &= (1u << (8 * (G::NBYTES % 4))) - 1u;
                anybad |= bad;
            }
        }
        if (anybad != 0) {
#pragma unroll
            for (int i = 0; i < G::NW; ++i) {
                const uint32_t u = U[i];
                const uint32_t code = (u >> 1) & 0x03030303u;
                uint32_t bad = perm_b32(0u, LUT_SELF, code) ^ u;
                if (i == G::NW - 1 && (G::NBYTES % 4) != 0) bad &= (1u << (8 * (G::NBYTES % 4))) - 1u;
                const uint64_t nib = nonzero_bytes4(bad);
                if (4 * i < 64) badlo |= nib << (4 * i);
                else if (4 * i < 128) badhi |= nib << (4 * i - 64);
                else badtop |= nib << (4 * i - 128);
            }
        }
    }
    static_assert(G::NBYTES <= 192 && K <= 128 && P <= 64, "window too long for the 192-bit validity mask");
    (
        [&] {
            const Mmh3Open open = PosOps<K, P, O, LATE>::template hash_open<PLAIN>(U, C, seed);
            if constexpr (EARLY) {
                if (!any_lane(early_may_keep(open, lim))) return;
            }
            const uint64_t h = mmh3_close<PLAIN>(open);
            bool ok = (h - 1) < thr;                          // h != 0 (signature.rs:50) and h <= thr (minhash.rs:319)
            if (anybad != 0) {
                // any invalid byte in [O, O+K) kills the k-mer (signature.rs:271-286, force=true)
                uint64_t lo, hi;                              // bits [O, O+128) of the mask (O < 64: P <= 64)
                if constexpr (O == 0) { lo = badlo; hi = badhi; }
                else { lo = (badlo >> O) | (badhi << (64 - O)); hi = (badhi >> O) | (badtop << (64 - O)); }
                const uint64_t mlo = K >= 64 ? ~0ull : ((1ull << K) - 1);
                const uint64_t mhi = K >= 128 ? ~0ull : K > 64 ? ((1ull << (K - 64)) - 1) : 0;
                if ((lo & mlo) | (hi & mhi)) ok = false;
            }
            if (ok) emit(O, h);
        }(),
        ...);
}

// A lane's raw window.  EARLY: test the top dword of the hash first and finish it only when some lane of the wave may keep its
// k-mer (1 wave-step in 16 at scaled = 1000); the result is the same either way.  Dense callers (every hash wanted) turn it off.
// PLAIN: the 64-bit constant multiplies of the hash as plain products (murmur3.hpp, mul_c64); the same values.
template <int K, int P, bool EARLY = true, bool PLAIN = false, class Emit>
SMG_HD void process_lane(const uint32_t* raw, uint64_t seed, uint64_t thr, Emit&& emit) {
    process_window<K, P, EARLY, PLAIN, false, false>(raw, nullptr, false, seed, thr, static_cast<Emit&&>(emit),
                                              std::make_integer_sequence<int, P>{});
}
// A staged window: U upper-cased, C its complement.  `dirty` (the tile's flag) MUST be wave-uniform on the device.
// LATE: the last key dword masked once, behind the strand select (PosOps); the same hashes.
template <int K, int P, bool EARLY = true, bool PLAIN = false, bool LATE = false, class Emit>
SMG_HD void process_lane_staged(const uint32_t* U, const uint32_t* C, bool dirty, uint64_t seed, uint64_t thr, Emit&& emit) {
    process_window<K, P, EARLY, PLAIN, true, LATE>(U, C, dirty, seed, thr, static_cast<Emit&&>(emit), std::make_integer_sequence<int, P>{});
}

// ---- the tile walk: what every DNA k-mer kernel does around its per-position code ---------------------------------------------
// A workgroup of BLOCK lanes takes tiles of BLOCK x P start positions.  It stages the tile and its halo into LDS as 16-byte
// chunks (stage_tile over load_chunk), each lane reads its window back as whole 16-byte groups (read_window) and hashes it, and
// kept values wait in LDS for one global atomic per flush (LdsSink).
//
// STAGED, the per-byte work done once (the appending form of sketch_kernel.hpp): a lane window is 46 bytes at k = 31 for 16 new
// ones, so upper-casing, complement and validity per lane treat every staged byte about 2.9 times.  Here the lane that stages a
// 16-byte chunk does them for the chunk, the tile goes to LDS twice -- upper-cased and complemented -- and a flag per tile says
// whether any staged byte is invalid.  A lane of a clean tile reads U and C as they are and does no validity work at all; a lane
// of a dirty tile rebuilds its bad-byte mask from U (process_window).

// Geometry of one tile: R consecutive windows ("rounds") of BLOCK lanes x P positions, staged together with one halo behind the
// last of them.  What is staged, and what a lane reads back: in round r the lane tid reads the window of lane index
// tid + r * BLOCK.  R = 1 is the tile every kernel but the appending staged sketch kernel walks.
template <int K, int P, int BLOCK, int R = 1>
struct TileGeom {
    using G = LaneGeom<K, P>;
    static constexpr int WINDOW = BLOCK * P;                        // start positions per round
    static constexpr int TILE = R * WINDOW;                         // start positions per tile
    static constexpr int LANE_RD = ((G::NW + 3) / 4) * 4;           // dwords each lane reads (whole 16-byte reads)
    // 16-byte chunks to stage for a tile of `rounds` rounds: the dwords up to the end of the last lane's read
    static constexpr int chunks(int rounds) { return ((rounds * BLOCK - 1) * (P / 4) + LANE_RD + 3) / 4; }
    static constexpr int IN_DW = (R * BLOCK - 1) * (P / 4) + LANE_RD;   // dwords the tile needs in LDS
    static constexpr int IN_CHUNKS = chunks(R);                     // 16-byte chunks to stage
};

// How many rounds a tile of the appending sketch kernel gets (sketch_kernel.hpp): r_max, unless the hashes a tile of r_max rounds
// is expected to keep -- its positions times thr / 2^64 -- are more than a quarter of the cap entries its sink holds between two
// flush checks; then 1, as for small `scaled` values and for num sketches (thr = 2^64 - 1).  window = positions per round.
SMG_HD uint32_t sk_tile_rounds(uint64_t thr, uint32_t r_max, uint32_t window, uint32_t cap) {
    if (r_max <= 1) return 1;
    const uint64_t positions = (uint64_t)r_max * window;            // < 2^32
    const uint64_t expected = (positions * (thr >> 32)) >> 32;      // floor(positions * floor(thr / 2^32) / 2^32)
    return expected + 1 > cap / 4 ? 1u : r_max;
}

// Which tiles a workgroup of the appending sketch kernel walks when they are handed out by tickets (sketch_kernel.hpp): its first
// tile is its own index, without a ticket; the tile behind ticket t of the launch's counter (0, 1, 2, .. in the order the
// workgroups ask) is grid + t; a workgroup is done at the first index that is no tile.  Every tile of [0, n_tiles) is then walked
// once whatever the order of the tickets, and each workgroup that had a tile takes exactly one ticket that fails.
SMG_HD uint64_t tile_first(uint32_t workgroup) { return workgroup; }
SMG_HD uint64_t tile_from_ticket(uint32_t grid, uint64_t ticket) { return (uint64_t)grid + ticket; }
SMG_HD bool tile_end(uint64_t tile, uint64_t n_tiles) { return tile >= n_tiles; }

// The 16 bytes at seq + off as 4 little-endian dwords: zero past `len`, and the first `skip` (< 16) bytes of the buffer blanked.
// seq + off is 16-byte aligned.
SMG_HD void load_chunk(const uint8_t* seq, uint64_t off, uint64_t len, uint32_t skip, uint32_t* w) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (off + 16 <= len) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 v = *reinterpret_cast<const uint4*>(seq + off);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#else
        for (int b = 0; b < 16; ++b) w[b >> 2] |= (uint32_t)seq[off + b] << (8 * (b & 3));
#endif
    } else if (off < len) {
        for (uint64_t b = off; b < len; ++b) w[(b - off) >> 2] |= (uint32_t)seq[b] << (8 * ((b - off) & 3));
    }
    if (off == 0 && skip) {                      // blank the alignment prefix
        for (uint32_t b = 0; b < skip; ++b) w[b >> 2] &= ~(0xffu << (8 * (b & 3)));
    }
}

// One chunk in place: w becomes its upper-cased bytes, c their complements; returns nonzero iff a byte is not ACGT
// (the zero fill and the blanked prefix are such bytes).
SMG_HD uint32_t stage_chunk(uint32_t* w, uint32_t* c) {
    uint32_t anybad = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t u = w[j] & 0xdfdfdfdfu;              // upper-case (signature.rs:214)
        const uint32_t code = (u >> 1) & 0x03030303u;
        w[j] = u;
        c[j] = perm_b32(0u, LUT_COMP, code);                 // encodings.rs:85-101
        anybad |= perm_b32(0u, LUT_SELF, code) ^ u;          // encodings.rs:370-377
    }
    return anybad;
}

SMG_HD void store_chunk(uint32_t* dst, const uint32_t* w) {      // dst is 16-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
#else
    dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2]; dst[3] = w[3];
#endif
}

// Stage the IN_CHUNKS chunks of the tile at seq + base into s_in: on the device chunk c by lane c mod BLOCK of the workgroup (the
// callers put a barrier on either side), on the host all of them.  STAGED: s_in upper-cased, s_comp its complement byte for
// byte, and *s_dirty set where a staged byte is not ACGT (the caller has zeroed it in front of the barrier).  The unstaged forms of
// sketch_dna_kernel and hll_dna_kernel keep the unstaged loop inline, for their registers' sake: sketch_kernel.hpp, hll_kernel.hpp.
// n_chunks (<= IN_CHUNKS, which sizes the arrays): the chunks of this launch's tile where its rounds are a run-time value.
//
// BATCH (staged form, a caller's choice per instantiation): a tile of all IN_CHUNKS chunks that lies wholly inside the buffer
// (stage_batch_ok) is staged by stage_lane_batched -- a lane's loads all issued first, then the per-byte work and the stores in
// load order -- so that a tile pays one round trip to memory, not one per trip of the loop below.  Every other tile -- the last
// one, the first one behind an alignment prefix, and every tile of a launch that walks fewer rounds than IN_CHUNKS was sized
// for (n_chunks < IN_CHUNKS: whole trips of the batch would serve no chunk) -- takes the loop, which keeps the one
// implementation of the zero fill and the prefix blanking.  The choice is the same for every lane of the workgroup.  On the
// host the function stages all chunks by the loop, whatever BATCH.
SMG_HD bool stage_batch_ok(uint64_t base, uint64_t len, uint32_t skip, int n_chunks, int in_chunks) {
    return n_chunks == in_chunks && base + 16ull * (uint64_t)n_chunks <= len && !(base == 0 && skip != 0);
}

// The chunks lane + j * BLOCK (< IN_CHUNKS) of a tile for which stage_batch_ok holds, staged: what the loop of stage_tile does
// for them, with every load in front of the first use.  In the last trip the lanes without a chunk (all but the few that take
// the stray chunks of the halo) take the tile's last chunk once more.  THE DUPLICATE STORES ARE RELIED ON TO BE IDEMPOTENT:
// such a lane loads, stages and stores exactly what that chunk's own lane does -- the same bytes to the same words of s_in and
// s_comp, the same 1 to *s_dirty -- so whichever store lands last, the words hold the same value.
template <int IN_CHUNKS, int BLOCK>
SMG_HD void stage_lane_batched(const uint8_t* seq, uint64_t base, int lane, uint32_t* s_in, uint32_t* s_comp, unsigned int* s_dirty,
                               int n_chunks = IN_CHUNKS) {
    // n_chunks: IN_CHUNKS, which the device caller passes as the run-time value it compared with it -- with the constant the
    // compiler holds the last load back behind a wait for the first two
    constexpr int TRIPS = (IN_CHUNKS + BLOCK - 1) / BLOCK;
    uint32_t w[TRIPS][4];
    // So the batch is straight-line code without a lane mask.  With a branch per load the compiler joins a load's block with
    // the block of its use and waits for memory once per trip again.
#pragma unroll
    for (int j = 0; j < TRIPS; ++j) {
        const int c = lane + j * BLOCK < n_chunks ? lane + j * BLOCK : n_chunks - 1;
        const uint64_t off = base + (uint64_t)c * 16;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 v = *reinterpret_cast<const uint4*>(seq + off);
        w[j][0] = v.x; w[j][1] = v.y; w[j][2] = v.z; w[j][3] = v.w;
#else
        w[j][0] = w[j][1] = w[j][2] = w[j][3] = 0;
        for (int b = 0; b < 16; ++b) w[j][b >> 2] |= (uint32_t)seq[off + b] << (8 * (b & 3));
#endif
    }
#pragma unroll
    for (int j = 0; j < TRIPS; ++j) {
        const int c = lane + j * BLOCK < n_chunks ? lane + j * BLOCK : n_chunks - 1;
        uint32_t cw[4];
        if (stage_chunk(w[j], cw)) *s_dirty = 1;
        store_chunk(&s_comp[c * 4], cw);
        store_chunk(&s_in[c * 4], w[j]);
    }
}

template <int IN_CHUNKS, bool STAGED, int BLOCK, bool BATCH = false>
SMG_HD void stage_tile(const uint8_t* seq, uint64_t base, uint64_t len, uint32_t skip, uint32_t* s_in, uint32_t* s_comp,
                       unsigned int* s_dirty, int n_chunks = IN_CHUNKS) {
    static_assert(!BATCH || STAGED, "the batch is a form of the staged tile");
#if defined(__HIP_DEVICE_COMPILE__)
    int first = threadIdx.x;
    const int step = BLOCK;
    if constexpr (BATCH) {
        // The lane index and the chunk count pass through an empty asm: what is derived from them -- the lane's addresses in
        // memory and in LDS, the batch's bounds -- is then computed here, per tile, where the window's registers are dead.
        // Otherwise they are invariants of the caller's tile loop, and the compiler keeps two dozen of them in registers across
        // the hash loop (k = 31: 120 -> 141 vector registers, a wave per SIMD).  The lever is the compiler's to honour and no
        // test sees it fail: after a compiler change compare the registers with tools/kernel_resources.py (118 at k = 31,
        // profiles/stage_batch_kernel_resources.txt).
        asm volatile("" : "+v"(first));
        asm volatile("" : "+s"(n_chunks));
        if (stage_batch_ok(base, len, skip, n_chunks, IN_CHUNKS)) {
            stage_lane_batched<IN_CHUNKS, BLOCK>(seq, base, first, s_in, s_comp, s_dirty, n_chunks);
            return;
        }
    }
#else
    const int first = 0, step = 1;
#endif
    for (int c = first; c < n_chunks; c += step) {
        uint32_t w[4];
        load_chunk(seq, base + (uint64_t)c * 16, len, skip, w);
        if constexpr (STAGED) {
            uint32_t cw[4];
            if (stage_chunk(w, cw)) *s_dirty = 1;
            store_chunk(&s_comp[c * 4], cw);
        }
        store_chunk(&s_in[c * 4], w);
    }
}

// The window of lane `tid`: LANE_RD dwords of the staged tile s from dword tid * P / 4 on, read as whole 16-byte groups where
// the lane's run starts on one (P = 16, 32), as dwords otherwise.
template <int LANE_RD, int P>
SMG_HD void read_window(const uint32_t* s, int tid, uint32_t* out) {
    static_assert(P % 4 == 0 && LANE_RD % 4 == 0, "lane runs must start dword aligned");
    const uint32_t* p = &s[tid * (P / 4)];
#pragma unroll
    for (int i = 0; i < LANE_RD / 4; ++i) {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr ((P / 4) % 4 == 0) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[i];
            out[4 * i] = v.x; out[4 * i + 1] = v.y; out[4 * i + 2] = v.z; out[4 * i + 3] = v.w;
            continue;
        }
#endif
        out[4 * i] = p[4 * i]; out[4 * i + 1] = p[4 * i + 1]; out[4 * i + 2] = p[4 * i + 2]; out[4 * i + 3] = p[4 * i + 3];
    }
}

#if defined(__HIPCC__)
// Where a workgroup of BLOCK lanes keeps its kept values: entries of NV u64 values each (a hash; a hash and its position) wait in
// LDS, CAP of them, and go out with one global atomic per flush, so that the output counter sees a few thousand atomics per launch
// instead of one per kept value.  The output is unordered; *out_count keeps counting past out_cap, entries past it are dropped.
// The kernel declares the LDS (s_val[j][CAP], s_cnt, s_base) and zeroes *s_cnt in front of its first barrier.
template <int CAP, int BLOCK, int NV = 1>
struct LdsSink {
    uint64_t* s_val[NV];
    unsigned int* s_cnt;
    unsigned long long* s_base;
    uint64_t* out[NV];
    unsigned long long* out_count;
    uint64_t out_cap;
    // The staging store names its address space.  As a generic pointer it has the type of the spill's store to HBM, and with
    // NV = 2 the optimiser then merges the last store of the two branches into one flat store through a selected pointer.
    using lds_u64 = __attribute__((address_space(3))) uint64_t;

    template <class... V>
    __device__ __forceinline__ void append(V... v) const {
        static_assert(sizeof...(V) == NV, "one value per array");
        const uint64_t e[NV] = {(uint64_t)v...};
        const unsigned int idx = atomicAdd(s_cnt, 1u);
        if (idx < (unsigned)CAP) {
#pragma unroll
            for (int j = 0; j < NV; ++j) ((lds_u64*)s_val[j])[idx] = e[j];
        } else {  // pathological density (e.g. scaled == 1): spill straight to HBM
            const unsigned long long g = atomicAdd(out_count, 1ull);
            if (g < out_cap) {
#pragma unroll
                for (int j = 0; j < NV; ++j) out[j][g] = e[j];
            }
        }
    }
    // Write the buffer out if it holds at least `at_least` entries: CAP / 2 between tiles, 1 at the end.  Called by every thread
    // of the workgroup, behind a barrier.
    __device__ __forceinline__ void flush(unsigned int at_least) const {
        const unsigned int cnt = *s_cnt;                      // workgroup-uniform
        if (cnt < at_least) return;
        const unsigned int n = cnt < (unsigned)CAP ? cnt : (unsigned)CAP;
        if (threadIdx.x == 0) *s_base = atomicAdd(out_count, (unsigned long long)n);
        __syncthreads();
        const unsigned long long b = *s_base;
        for (unsigned int i = threadIdx.x; i < n; i += BLOCK) {
            if (b + i < out_cap) {
#pragma unroll
                for (int j = 0; j < NV; ++j) out[j][b + i] = s_val[j][i];
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) *s_cnt = 0;
    }
};
#endif

}  // namespace smg
