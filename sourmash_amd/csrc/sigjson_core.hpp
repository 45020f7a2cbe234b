// sigjson_core.hpp -- the rules of the signature JSON array parser (sigjson.hip), host + device.
//
// What the two kernels do and why is in sigjson.hip.  What is here has no thread index and no wave primitive in it: which bytes
// are white space, where a key that opens an array stands, what one 64-byte tile of the span scan adds to an array's tallies,
// what a span record says, how an array is cut into chunks and a chunk into lanes, how one number is read and when it is
// refused, which index a lane's first number has, and what a lane makes of the written values afterwards.  On the device a lane
// is a thread and the ballots, the prefix sum and the reduction are the wavefront's; tests/native/sigjson_emul.cpp walks the same
// functions with lanes as loop indices and supplies loop versions of those three.
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

constexpr uint32_t SJ_MAX_SPANS = 8;        // arrays looked at per document; a document with more is the host's
constexpr uint32_t SJ_MINS = 0, SJ_ABUND = 1;
constexpr uint32_t SJ_SPAN_ODD = 1;         // an array holds something the device does not parse
constexpr uint32_t SJ_DOC_ODD = 0x80000000u;   // doc_flags: this bit, or the number of arrays found in the low bits

struct SjDoc { uint64_t off, len; };        // a document's text inside the text block
struct SjSpan {
    uint64_t begin, end;                    // the array's bytes between '[' and ']', relative to the document
    uint32_t n_values, kind, flags, pad;
};
struct SjParse {                            // one `mins` array to turn into numbers
    uint64_t text_off, len;                 // its bytes (inside the text block)
    uint64_t value_off;                     // where its values go
    uint64_t n_values;
};
struct SjParsed { uint32_t n_kept, flags; };    // values <= keep_max (they come first: the array ascends); SJ_SPAN_ODD: not ascending / not plain numbers

// The parse kernel walks an array SJ_CHUNK bytes at a time and reads SJ_AHEAD bytes beyond the chunk, so that a number which
// begins in the chunk's last bytes still ends inside what was read.  Every chunk is loaded in 16-byte lines from the line it
// begins in: SJ_BUF_LINES lines hold the most that can be wanted (15 bytes of shift + chunk + look-ahead), and the last line of
// an array's last chunk reaches up to 15 bytes past the array -- past the text block by up to SJ_TEXT_PAD - 2 bytes when the
// array's ']' is the block's last byte.  That many bytes must be readable behind a text block.
constexpr uint32_t SJ_CHUNK = 4096, SJ_AHEAD = 64, SJ_LANE_BYTES = SJ_CHUNK / 64;
constexpr uint32_t SJ_BUF_LINES = (SJ_CHUNK + SJ_AHEAD + 16) / 16 + 1;
constexpr uint32_t SJ_TEXT_PAD = 16;

SMG_HD bool sj_is_ws(uint32_t c) { return c == ' ' || c == '\n' || c == '\r' || c == '\t'; }
SMG_HD bool sj_is_digit(uint32_t c) { return c >= '0' && c <= '9'; }

// ---- the span scan ----

SMG_HD bool sj_starts_with(const uint8_t* t, uint64_t i, uint64_t len, const char* key, uint32_t klen) {
    if (i + klen > len) return false;
    for (uint32_t k = 0; k < klen; ++k) if (t[i + k] != (uint8_t)key[k]) return false;
    return true;
}

// does a key that may open an array we take begin at t[i]: "mins" or "abundances", quotes included
SMG_HD bool sj_key_at(const uint8_t* t, uint64_t i, uint64_t len) {
    return t[i] == '"' && (sj_starts_with(t, i, len, "\"mins\"", 6) || sj_starts_with(t, i, len, "\"abundances\"", 12));
}
SMG_HD uint32_t sj_key_kind(const uint8_t* t, uint64_t m) { return t[m + 1] == 'm' ? SJ_MINS : SJ_ABUND; }
SMG_HD uint32_t sj_key_len(uint32_t kind) { return kind == SJ_MINS ? 6u : 12u; }

// behind a key that ends in front of t[q]: ws* ':' ws* '[' -> the position behind the '[', or len + 1 when something else
// stands there (a string value, null, an object) or the document ends first
SMG_HD uint64_t sj_array_begin(const uint8_t* t, uint64_t q, uint64_t len) {
    while (q < len && sj_is_ws(t[q])) ++q;
    if (q >= len || t[q] != ':') return len + 1;
    ++q;
    while (q < len && sj_is_ws(t[q])) ++q;
    if (q >= len || t[q] != '[') return len + 1;                      // (abundances may be null)
    return q + 1;
}

// a byte of an array by class; a position at or behind the document's end counts as the closing bracket
struct SjByteClass { bool close, comma, digit, odd; };
SMG_HD SjByteClass sj_class_at(const uint8_t* t, uint64_t i, uint64_t len) {
    const uint32_t c = i < len ? t[i] : (uint32_t)']';
    SjByteClass k;
    k.close = c == ']';
    k.comma = c == ',';
    k.digit = sj_is_digit(c);
    k.odd = !(c == ',' || sj_is_digit(c) || sj_is_ws(c) || c == ']');
    return k;
}

// what an array holds up to its closing bracket
struct SjTally { uint32_t commas, digits, odd; };

// one 64-byte tile: bit l of each mask is the class of byte p + l.  Only the bytes in front of the tile's first ']' count; the
// array ends in this tile, at the lowest bit of `close`, when close != 0
SMG_HD void sj_tile_fold(uint64_t close, uint64_t comma, uint64_t digit, uint64_t oddm, SjTally& t) {
    const uint64_t upto = close ? (1ull << __builtin_ctzll(close)) - 1ull : ~0ull;     // lanes in front of the first ']'
    t.commas += (uint32_t)__builtin_popcountll(comma & upto);
    t.digits |= (digit & upto) != 0ull;
    t.odd |= (oddm & upto) != 0ull;
}

// the record of an array of bytes [s, e) of its document: values = commas + 1 if it holds a digit at all; odd if it holds a byte
// the parser does not take, or commas and no digit
SMG_HD SjSpan sj_span_record(uint64_t s, uint64_t e, uint32_t kind, const SjTally& t) {
    SjSpan sp;
    sp.begin = s; sp.end = e;
    sp.n_values = t.digits ? t.commas + 1u : 0u;
    sp.kind = kind;
    sp.flags = (t.odd ? SJ_SPAN_ODD : 0u) | (!t.digits && t.commas ? SJ_SPAN_ODD : 0u);
    sp.pad = 0;
    return sp;
}

// ---- the number parser ----

// the chunk that begins at byte c0 of an array of len bytes, whose byte c0 has the address addr
struct SjChunkGeom {
    uint32_t shift;       // addr mod 16: the chunk's first byte inside the first line loaded
    uint32_t want;        // bytes of the array read: the chunk and the look-ahead, or what is left of the array
    uint32_t lines;       // 16-byte lines that hold them
    uint32_t in_chunk;    // bytes whose commas this chunk owns
};
SMG_HD SjChunkGeom sj_chunk_geom(uint64_t addr, uint64_t c0, uint64_t len) {
    SjChunkGeom g;
    const uint64_t avail = len - c0;                                  // bytes of the array from c0 on
    g.shift = (uint32_t)(addr & 15u);
    g.want = (uint32_t)(avail < SJ_CHUNK + SJ_AHEAD ? avail : SJ_CHUNK + SJ_AHEAD);
    g.lines = (g.shift + g.want + 15u) / 16u;
    g.in_chunk = (uint32_t)(avail < SJ_CHUNK ? avail : SJ_CHUNK);
    return g;
}

// lane l owns bytes [p0, p1) of the chunk
SMG_HD uint32_t sj_lane_begin(uint32_t lane) { return lane * SJ_LANE_BYTES; }
SMG_HD uint32_t sj_lane_end(uint32_t lane, uint32_t in_chunk) {
    const uint32_t p0 = lane * SJ_LANE_BYTES;
    return p0 + SJ_LANE_BYTES < in_chunk ? p0 + SJ_LANE_BYTES : in_chunk;
}
SMG_HD uint32_t sj_lane_commas(const uint8_t* b, uint32_t p0, uint32_t p1) {
    uint32_t commas = 0;
    for (uint32_t i = p0; i < p1; ++i) commas += b[i] == ',';
    return commas;
}

// `index` numbers begin in front of the chunk; incl = the commas of lanes 0 .. l of the chunk, commas = lane l's own
struct SjChunkIndex {
    uint64_t lane_first;  // commas in front of this lane's bytes = index of the number open there
    uint64_t next;        // numbers that begin in front of the next chunk
};
SMG_HD SjChunkIndex sj_chunk_index(uint64_t index, uint32_t incl, uint32_t commas, uint32_t chunk_commas) {
    SjChunkIndex r;
    r.lane_first = index + (incl - commas);
    r.next = index + chunk_commas;
    return r;
}

// The number that begins at b[from] (white space allowed around it); b[i] = byte c0 + i of the array, i < want.  It must end at
// a comma, or at the end of the array -- not at the end of what was read.  bad is set for: no digit, more than 20, a value
// beyond 2^64 - 1, another byte in front of the comma, the end of what was read with more of the array behind it.
SMG_HD uint64_t sj_number(const uint8_t* b, uint32_t want, uint32_t from, uint64_t c0, uint64_t len, uint32_t& bad) {
    uint32_t i = from;
    while (i < want && sj_is_ws(b[i])) ++i;
    uint64_t v = 0;
    uint32_t nd = 0;
    while (i < want && b[i] >= '0' && b[i] <= '9') {
        if (nd >= 19 && (v > 1844674407370955161ull || (v == 1844674407370955161ull && b[i] > '5'))) bad = 1;   // beyond 2^64 - 1
        v = v * 10 + (uint64_t)(b[i] - '0');
        ++nd;
        ++i;
    }
    while (i < want && sj_is_ws(b[i])) ++i;
    if (nd == 0 || nd > 20) bad = 1;
    if (i < want ? b[i] != ',' : c0 + i < len) bad = 1;
    return v;
}

// what a lane does with a chunk: the array's first number is lane 0's in the first chunk, every other number belongs to the lane
// that holds the comma in front of it
SMG_HD void sj_parse_lane(const uint8_t* b, const SjChunkGeom& g, uint32_t lane, uint64_t c0, uint64_t len, uint64_t lane_first,
                          uint64_t n_values, uint64_t* out, uint32_t& bad) {
    const uint32_t p0 = sj_lane_begin(lane), p1 = sj_lane_end(lane, g.in_chunk);
    uint64_t k = lane_first;
    if (c0 == 0 && lane == 0 && n_values) {
        const uint64_t v = sj_number(b, g.want, 0, c0, len, bad);
        out[0] = v;
    }
    for (uint32_t i = p0; i < p1; ++i)
        if (b[i] == ',') {
            ++k;
            const uint64_t v = sj_number(b, g.want, i + 1, c0, len, bad);
            if (k < n_values) out[k] = v;
        }
}

// order (ascending, no repeats: minhash.rs:161-171 would sort -- such an array is the host's) and the down-sampling count, over
// the values lane, lane + 64, ...
SMG_HD void sj_order_lane(const uint64_t* out, uint64_t n_values, uint32_t lane, uint64_t keep_max, uint32_t& kept, uint32_t& bad) {
    for (uint64_t i = lane; i < n_values; i += 64u) {
        const uint64_t v = out[i];
        kept += v <= keep_max;
        if (i + 1 < n_values && out[i + 1] <= v) bad = 1;
    }
}

}  // namespace smg
