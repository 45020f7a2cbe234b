// translate_records_core.hpp -- the six-frame translation of many records into one residue buffer (protein_records.hip), host +
// device.
//
// Reference: src/core/src/signature.rs:257-261, 307-351 -- frames 0..2 of a record, forward and on the reverse complement OF
// THAT RECORD, a trailing partial codon dropped (encodings.rs to_aa), no validity test.
//
// Layout: record r (records_core.hpp: the bytes [starts[r], ends[r])) owns the block [block_starts[r], block_starts[r + 1]) of
// the output, translated_block_bytes(len_r) bytes: the six segments of translate_layout(len_r), each followed by a 0xFF
// separator, exactly what translate_kernel writes for one record.  block_starts is the exclusive prefix sum of the block sizes
// over n_records + 1 entries, so block_starts[n_records] is the size of the buffer.  A block is never empty (six separators),
// no window crosses a separator and every block ends in one: the block of a window's start is its record.
#pragma once
#include <stdint.h>
#include "records_core.hpp"
#include "translate_core.hpp"

namespace smg {

SMG_HD uint64_t translated_block_bytes(uint64_t len) { return translate_layout(len).start[6]; }
// never below the sum of the block sizes of n_records records that hold `len` bytes in all: a segment of frame f holds at most
// len_r / 3 residues, so a block at most 2 len_r + 6 bytes
SMG_HD uint64_t translated_records_bound(uint64_t len, uint64_t n_records) { return 2 * len + 6 * n_records; }

// block of output byte o: the last one that starts at or before it (o < block_starts[n_records])
SMG_HD uint64_t translate_block_of(const uint64_t* block_starts, uint64_t n_records, uint64_t o) {
    uint64_t lo = 0, hi = n_records;                     // first index with block_starts[index] > o, among 1 .. n_records
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (block_starts[mid + 1] <= o) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// A lane owns one aligned 8-byte WORD of the output, bytes 8 G .. 8 G + 7: one search for the block of its first byte, then
// byte by byte by the definition (translate_one), stepping into the next block where the word crosses.  -> the eight bytes,
// little-endian; bytes at or behind block_starts[n_records] are 0.
SMG_HD uint64_t translate_records_word(const uint8_t* seq, const uint64_t* starts, const uint64_t* ends, const uint64_t* block_starts,
                                       uint64_t n_records, const TranslateTables& T, uint64_t G) {
    const uint64_t total = block_starts[n_records];
    uint64_t o = 8 * G;
    if (o >= total) return 0;
    uint64_t r = translate_block_of(block_starts, n_records, o);
    TranslateLayout L = translate_layout(rec_len(starts, ends, r));
    uint64_t out = 0;
    for (int j = 0; j < 8 && o < total; ++j, ++o) {
        if (o >= block_starts[r + 1]) {
            ++r;
            L = translate_layout(rec_len(starts, ends, r));
        }
        out |= (uint64_t)translate_one(seq + starts[r], L, T, o - block_starts[r]) << (8 * j);
    }
    return out;
}

}  // namespace smg
