// sigwrite_core.hpp -- the rules of the signature writer (sigwrite.hip), host + device.
//
// What the kernels do and why is in sigwrite.hip.  What is here has no thread index in it: how many decimal digits a hash has and
// which, the MD5 of a row's message (the decimal text of ksize and of every hash, no separators: minhash.rs:290-307) as ONE lane
// computes it through a 128-byte ring, the literal code of the deflate blocks with its block header, which bytes of a chunk a
// lane packs and what it ORs where.  On the device a lane is a thread, the ring and the chunk's words are LDS and the prefix sum
// is the block's; tests/native/sigwrite_emul.cpp walks the same functions with lanes as loop indices.
#pragma once
#include <stdint.h>

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

// ---- decimal text ------------------------------------------------------------------------------------------------------------
constexpr uint32_t SW_MAX_DIGITS = 20;                              // 2^64 - 1 = 18446744073709551615

SMG_HD uint32_t sw_digit_count(uint64_t v) {
    uint32_t n = 1;
    if (v >= 10000000000000000ull) { n += 16; v /= 10000000000000000ull; }
    if (v >= 100000000ull) { n += 8; v /= 100000000ull; }
    if (v >= 10000ull) { n += 4; v /= 10000ull; }
    if (v >= 100ull) { n += 2; v /= 100ull; }
    if (v >= 10ull) n += 1;
    return n;
}

// the nd = sw_digit_count(v) digits of v, most significant first, through put(index, byte)
template <class Put>
SMG_HD void sw_put_decimal(uint64_t v, uint32_t nd, Put put) {
    for (uint32_t j = nd; j-- > 0;) { put(j, (uint8_t)('0' + (uint32_t)(v % 10u))); v /= 10u; }
}

// ---- MD5 of a row, one lane ----------------------------------------------------------------------------------------------------
// A lane's ring is 128 bytes = 32 words; word i of the lane is base[i * stride] (on the device the words of the 64 lanes of a
// wave are interleaved, stride 64: a wave's access to word i is one row of LDS banks).
struct SwRing {
    uint32_t* base;
    uint32_t stride;
    SMG_HD void put(uint64_t at, uint8_t b) const {
        const uint32_t i = (uint32_t)at & 127u;
        reinterpret_cast<uint8_t*>(base + (i >> 2) * stride)[i & 3u] = b;
    }
    SMG_HD uint32_t word(uint32_t i) const { return base[i * stride]; }
};

struct SwMd5 { uint32_t a, b, c, d; };

SMG_HD uint32_t sw_rol(uint32_t x, uint32_t s) { return (x << s) | (x >> (32u - s)); }

// one 64-byte block (RFC 1321): the words of half `half` of the ring
SMG_HD void sw_md5_block(SwMd5& s, const SwRing& r, uint32_t half) {
    uint32_t x[16];
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) x[i] = r.word(half * 16u + i);
    uint32_t a = s.a, b = s.b, c = s.c, d = s.d;
#define SW_STEP(f, a, b, c, d, xi, t, sh) a = b + sw_rol(a + f(b, c, d) + xi + t, sh)
#define SW_F(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define SW_G(x, y, z) ((y) ^ ((z) & ((x) ^ (y))))
#define SW_H(x, y, z) ((x) ^ (y) ^ (z))
#define SW_I(x, y, z) ((y) ^ ((x) | ~(z)))
    SW_STEP(SW_F, a, b, c, d, x[0], 0xd76aa478u, 7);   SW_STEP(SW_F, d, a, b, c, x[1], 0xe8c7b756u, 12);
    SW_STEP(SW_F, c, d, a, b, x[2], 0x242070dbu, 17);  SW_STEP(SW_F, b, c, d, a, x[3], 0xc1bdceeeu, 22);
    SW_STEP(SW_F, a, b, c, d, x[4], 0xf57c0fafu, 7);   SW_STEP(SW_F, d, a, b, c, x[5], 0x4787c62au, 12);
    SW_STEP(SW_F, c, d, a, b, x[6], 0xa8304613u, 17);  SW_STEP(SW_F, b, c, d, a, x[7], 0xfd469501u, 22);
    SW_STEP(SW_F, a, b, c, d, x[8], 0x698098d8u, 7);   SW_STEP(SW_F, d, a, b, c, x[9], 0x8b44f7afu, 12);
    SW_STEP(SW_F, c, d, a, b, x[10], 0xffff5bb1u, 17); SW_STEP(SW_F, b, c, d, a, x[11], 0x895cd7beu, 22);
    SW_STEP(SW_F, a, b, c, d, x[12], 0x6b901122u, 7);  SW_STEP(SW_F, d, a, b, c, x[13], 0xfd987193u, 12);
    SW_STEP(SW_F, c, d, a, b, x[14], 0xa679438eu, 17); SW_STEP(SW_F, b, c, d, a, x[15], 0x49b40821u, 22);
    SW_STEP(SW_G, a, b, c, d, x[1], 0xf61e2562u, 5);   SW_STEP(SW_G, d, a, b, c, x[6], 0xc040b340u, 9);
    SW_STEP(SW_G, c, d, a, b, x[11], 0x265e5a51u, 14); SW_STEP(SW_G, b, c, d, a, x[0], 0xe9b6c7aau, 20);
    SW_STEP(SW_G, a, b, c, d, x[5], 0xd62f105du, 5);   SW_STEP(SW_G, d, a, b, c, x[10], 0x02441453u, 9);
    SW_STEP(SW_G, c, d, a, b, x[15], 0xd8a1e681u, 14); SW_STEP(SW_G, b, c, d, a, x[4], 0xe7d3fbc8u, 20);
    SW_STEP(SW_G, a, b, c, d, x[9], 0x21e1cde6u, 5);   SW_STEP(SW_G, d, a, b, c, x[14], 0xc33707d6u, 9);
    SW_STEP(SW_G, c, d, a, b, x[3], 0xf4d50d87u, 14);  SW_STEP(SW_G, b, c, d, a, x[8], 0x455a14edu, 20);
    SW_STEP(SW_G, a, b, c, d, x[13], 0xa9e3e905u, 5);  SW_STEP(SW_G, d, a, b, c, x[2], 0xfcefa3f8u, 9);
    SW_STEP(SW_G, c, d, a, b, x[7], 0x676f02d9u, 14);  SW_STEP(SW_G, b, c, d, a, x[12], 0x8d2a4c8au, 20);
    SW_STEP(SW_H, a, b, c, d, x[5], 0xfffa3942u, 4);   SW_STEP(SW_H, d, a, b, c, x[8], 0x8771f681u, 11);
    SW_STEP(SW_H, c, d, a, b, x[11], 0x6d9d6122u, 16); SW_STEP(SW_H, b, c, d, a, x[14], 0xfde5380cu, 23);
    SW_STEP(SW_H, a, b, c, d, x[1], 0xa4beea44u, 4);   SW_STEP(SW_H, d, a, b, c, x[4], 0x4bdecfa9u, 11);
    SW_STEP(SW_H, c, d, a, b, x[7], 0xf6bb4b60u, 16);  SW_STEP(SW_H, b, c, d, a, x[10], 0xbebfbc70u, 23);
    SW_STEP(SW_H, a, b, c, d, x[13], 0x289b7ec6u, 4);  SW_STEP(SW_H, d, a, b, c, x[0], 0xeaa127fau, 11);
    SW_STEP(SW_H, c, d, a, b, x[3], 0xd4ef3085u, 16);  SW_STEP(SW_H, b, c, d, a, x[6], 0x04881d05u, 23);
    SW_STEP(SW_H, a, b, c, d, x[9], 0xd9d4d039u, 4);   SW_STEP(SW_H, d, a, b, c, x[12], 0xe6db99e5u, 11);
    SW_STEP(SW_H, c, d, a, b, x[15], 0x1fa27cf8u, 16); SW_STEP(SW_H, b, c, d, a, x[2], 0xc4ac5665u, 23);
    SW_STEP(SW_I, a, b, c, d, x[0], 0xf4292244u, 6);   SW_STEP(SW_I, d, a, b, c, x[7], 0x432aff97u, 10);
    SW_STEP(SW_I, c, d, a, b, x[14], 0xab9423a7u, 15); SW_STEP(SW_I, b, c, d, a, x[5], 0xfc93a039u, 21);
    SW_STEP(SW_I, a, b, c, d, x[12], 0x655b59c3u, 6);  SW_STEP(SW_I, d, a, b, c, x[3], 0x8f0ccc92u, 10);
    SW_STEP(SW_I, c, d, a, b, x[10], 0xffeff47du, 15); SW_STEP(SW_I, b, c, d, a, x[1], 0x85845dd1u, 21);
    SW_STEP(SW_I, a, b, c, d, x[8], 0x6fa87e4fu, 6);   SW_STEP(SW_I, d, a, b, c, x[15], 0xfe2ce6e0u, 10);
    SW_STEP(SW_I, c, d, a, b, x[6], 0xa3014314u, 15);  SW_STEP(SW_I, b, c, d, a, x[13], 0x4e0811a1u, 21);
    SW_STEP(SW_I, a, b, c, d, x[4], 0xf7537e82u, 6);   SW_STEP(SW_I, d, a, b, c, x[11], 0xbd3af235u, 10);
    SW_STEP(SW_I, c, d, a, b, x[2], 0x2ad7d2bbu, 15);  SW_STEP(SW_I, b, c, d, a, x[9], 0xeb86d391u, 21);
#undef SW_STEP
#undef SW_F
#undef SW_G
#undef SW_H
#undef SW_I
    s.a += a; s.b += b; s.c += c; s.d += d;
}

// The message goes through the ring number by number.  A number has at most 20 digits, so it completes at most one 64-byte
// half; the half that filled is compressed before anything is written to it again (the other half takes the overflow).
struct SwMd5Stream {
    SwMd5 s;
    uint64_t total;
    SwRing ring;
    SMG_HD void init(const SwRing& r) {
        s.a = 0x67452301u; s.b = 0xefcdab89u; s.c = 0x98badcfeu; s.d = 0x10325476u;
        total = 0; ring = r;
    }
    SMG_HD void advance(uint32_t n) {                               // n <= 64 bytes were put at [total, total + n)
        const uint64_t next = total + n;
        if ((next >> 6) != (total >> 6)) sw_md5_block(s, ring, (uint32_t)(total >> 6) & 1u);
        total = next;
    }
    SMG_HD void number(uint64_t v) {
        const uint32_t nd = sw_digit_count(v);
        const uint64_t at = total;
        const SwRing r = ring;
        sw_put_decimal(v, nd, [&](uint32_t j, uint8_t b) { r.put(at + j, b); });
        advance(nd);
    }
    SMG_HD void finish(uint8_t* out16) {                            // RFC 1321 padding: 0x80, zeros to 56 mod 64, the bit count
        const uint64_t bits = total * 8u;
        ring.put(total, 0x80); advance(1);
        while ((total & 63u) != 56u) { ring.put(total, 0); advance(1); }
        for (uint32_t i = 0; i < 8; ++i) ring.put(total + i, (uint8_t)(bits >> (8u * i)));
        advance(8);
        const uint32_t w[4] = {s.a, s.b, s.c, s.d};
        for (uint32_t i = 0; i < 16; ++i) out16[i] = (uint8_t)(w[i >> 2] >> (8u * (i & 3u)));
    }
};

// the digest of str(ksize) || str(h[0]) || ... || str(h[n - 1])
SMG_HD void sw_md5_row(const SwRing& ring, uint32_t ksize, const uint64_t* h, uint64_t n, uint8_t* out16) {
    SwMd5Stream m;
    m.init(ring);
    m.number(ksize);
    for (uint64_t i = 0; i < n; ++i) m.number(h[i]);
    m.finish(out16);
}

// bytes of a row's message, and of the padded message (what a lane compresses)
SMG_HD uint64_t sw_md5_padded_len(uint64_t msg_len) { return (msg_len + 9u + 63u) & ~63ull; }

// ---- the literal code ----------------------------------------------------------------------------------------------------------
// One constant prefix code over the 256 byte values and end-of-block (symbol 256), for dynamic-Huffman blocks that hold
// literals only.  Hash text is uniformly random digits: LZ matching finds nothing in it, so entropy coding the bytes is all there
// is to win.  The lengths are those of an optimal code limited to 15 bits (package-merge) for the byte counts of a signature
// document of 5,000 uniform hashes below max_hash(scaled = 1000), x 200, plus 1 for every symbol, which gives every symbol a
// code and makes the code complete (Kraft sum 1).  tools/make_sigwrite_table.py derives them.
constexpr uint32_t SW_SYMBOLS = 257, SW_EOB = 256, SW_MAX_CODE_LEN = 15;
static constexpr uint8_t SW_CODE_LEN[SW_SYMBOLS] = {
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    11, 15, 8, 15, 15, 15, 15, 15, 15, 15, 15, 15, 5, 13, 11, 15, 4, 3, 3, 3, 3, 4, 4, 3, 4, 4, 10, 15, 15, 15, 15, 15,
    15, 13, 15, 11, 13, 13, 13, 12, 15, 15, 15, 13, 15, 12, 12, 15, 15, 15, 15, 13, 15, 15, 15, 15, 15, 15, 15, 12, 15, 12, 15, 11,
    15, 10, 13, 10, 11, 9, 11, 11, 11, 10, 15, 13, 11, 10, 10, 10, 13, 15, 10, 9, 11, 10, 12, 15, 13, 15, 12, 12, 15, 12, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15,
};

// entry of the packer's table: the code as it enters the stream (first bit in bit 0) | length << 16
SMG_HD uint32_t sw_entry_code(uint32_t e) { return e & 0xffffu; }
SMG_HD uint32_t sw_entry_len(uint32_t e) { return e >> 16; }

// ---- the packer ----------------------------------------------------------------------------------------------------------------
// A chunk of a document (at most SW_MAX_CHUNK bytes) is packed by one block: lane l of n_lanes takes the bytes
// [sw_lane_lo, sw_lane_hi), adds up their code lengths, a prefix sum over the lanes gives the bit its first code begins at, and
// the lane ORs its codes into the chunk's words.  Word 0 of the chunk's words is the output word that holds the chunk's first
// bit, so bit 0 of the chunk sits at bit (out_bit & 31) of word 0 and the words go out as they are: whole words inside, OR at
// both ends (a neighbouring chunk shares those words; the output begins as zeros).
constexpr uint32_t SW_MAX_CHUNK = 4096;
constexpr uint32_t SW_CHUNK_WORDS = (31u + (SW_MAX_CHUNK + 1u) * SW_MAX_CODE_LEN + 31u) / 32u + 1u;
constexpr uint32_t SW_CHUNK_LAST = 1;                               // chunk flags: the member's last chunk (end-of-block follows / BFINAL)

struct SwChunk {
    uint64_t in_off;                                                // the chunk's bytes inside the text block
    uint64_t out_bit;                                               // literal blocks: first bit of its codes; stored blocks: 8 x the byte of its block header
    uint32_t in_len, flags;
};
struct SwMember {                                                   // a gzip member inside the output block
    uint64_t out_off, out_len;                                      // its bytes: 10 of header, the deflate stream, 8 of trailer
    uint32_t crc, isize;
};

SMG_HD uint32_t sw_lane_lo(uint32_t len, uint32_t lane, uint32_t n_lanes) {
    const uint32_t per = (len + n_lanes - 1u) / n_lanes, lo = lane * per;
    return lo < len ? lo : len;
}
SMG_HD uint32_t sw_lane_hi(uint32_t len, uint32_t lane, uint32_t n_lanes) { return sw_lane_lo(len, lane + 1u, n_lanes); }

// code bits of the lane's bytes; the last lane of a member's last chunk adds end-of-block
SMG_HD uint32_t sw_lane_bits(const uint8_t* text, uint32_t lo, uint32_t hi, const uint32_t* table, bool eob) {
    uint32_t bits = 0;
    for (uint32_t i = lo; i < hi; ++i) bits += sw_entry_len(table[text[i]]);
    if (eob) bits += sw_entry_len(table[SW_EOB]);
    return bits;
}

// the lane's codes from bit `bit_at` of the chunk's words on, through or_word(word index, value)
template <class Or>
SMG_HD void sw_lane_pack(const uint8_t* text, uint32_t lo, uint32_t hi, const uint32_t* table, bool eob, uint32_t bit_at, Or or_word) {
    uint64_t acc = 0;
    uint32_t n = bit_at & 31u, w = bit_at >> 5;
    for (uint32_t i = lo; i < hi + (eob ? 1u : 0u); ++i) {
        const uint32_t e = table[i < hi ? (uint32_t)text[i] : SW_EOB];
        acc |= (uint64_t)sw_entry_code(e) << n;
        n += sw_entry_len(e);
        if (n >= 32u) { or_word(w++, (uint32_t)acc); acc >>= 32; n -= 32u; }
    }
    if (n && acc) or_word(w, (uint32_t)acc);
}

// words the chunk's bits reach into, from the word of its first bit
SMG_HD uint32_t sw_chunk_words(uint64_t out_bit, uint32_t chunk_bits) { return (uint32_t)(((out_bit & 31u) + chunk_bits + 31u) >> 5); }

constexpr uint32_t SW_STORED_MAX = 65535;                           // bytes of a stored block (BTYPE 00)
constexpr uint32_t SW_GZIP_HEADER = 10, SW_GZIP_TRAILER = 8;

// the 10-byte member header: deflate, no flags, mtime 0, OS unknown -- a set always writes the same bytes
SMG_HD uint8_t sw_gzip_header_byte(uint32_t i) { return i == 0 ? 0x1f : i == 1 ? 0x8b : i == 2 ? 8 : i == 9 ? 0xff : 0; }

}  // namespace smg

// ---- host only: the code words, the block header ------------------------------------------------------------------------------
#include <vector>
namespace smg {

// canonical codes of SW_CODE_LEN (RFC 1951 3.2.2), bit-reversed so that a code's first bit is bit 0
inline void sw_build_table(uint32_t table[SW_SYMBOLS]) {
    uint32_t count[SW_MAX_CODE_LEN + 2] = {0}, next[SW_MAX_CODE_LEN + 2] = {0};
    for (uint32_t s = 0; s < SW_SYMBOLS; ++s) count[SW_CODE_LEN[s]]++;
    uint32_t code = 0;
    for (uint32_t l = 1; l <= SW_MAX_CODE_LEN; ++l) { code = (code + count[l - 1]) << 1; next[l] = code; }
    for (uint32_t s = 0; s < SW_SYMBOLS; ++s) {
        const uint32_t l = SW_CODE_LEN[s], c = next[l]++;
        uint32_t r = 0;
        for (uint32_t b = 0; b < l; ++b) r |= ((c >> b) & 1u) << (l - 1u - b);
        table[s] = r | (l << 16);
    }
}

// The header of a final dynamic-Huffman block that uses this code: BFINAL 1, BTYPE 10, 257 literal / length codes, one distance
// code of no bits (no distance codes are used: RFC 1951 3.2.7), and a code-length code that gives each of the lengths 0 .. 15
// four bits (complete: 16 / 2^4), so the 258 lengths follow as 4-bit fields.  -> the bits, LSB first in bytes; returns their count.
inline uint32_t sw_build_block_header(std::vector<uint8_t>& bytes) {
    bytes.clear();
    uint32_t nbits = 0;
    auto put = [&](uint32_t v, uint32_t n) {
        for (uint32_t b = 0; b < n; ++b, ++nbits) {
            if ((nbits & 7u) == 0) bytes.push_back(0);
            bytes.back() |= (uint8_t)(((v >> b) & 1u) << (nbits & 7u));
        }
    };
    auto put_code4 = [&](uint32_t sym) {                            // canonical 4-bit code of length `sym`: the value itself, first bit = its top bit
        uint32_t r = 0;
        for (uint32_t b = 0; b < 4; ++b) r |= ((sym >> b) & 1u) << (3u - b);
        put(r, 4);
    };
    put(1, 1); put(2, 2);
    put(SW_SYMBOLS - 257u, 5); put(0, 5); put(19 - 4, 4);
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (uint32_t i = 0; i < 19; ++i) put(order[i] < 16 ? 4u : 0u, 3);
    for (uint32_t s = 0; s < SW_SYMBOLS; ++s) put_code4(SW_CODE_LEN[s]);
    put_code4(0);                                                   // the distance code
    return nbits;
}

}  // namespace smg
