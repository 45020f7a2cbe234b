// Internal launchers of sigwrite.hip: signature JSON, MD5 identities and gzip members written on the device (raw device pointers).
// The rules are in sigwrite_core.hpp; sigwrite.hpp is the host side that strings the launches together.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "sigwrite_core.hpp"

namespace smg {

struct SwRow {                  // where a row's document goes and where its head comes from
    uint64_t doc_off;           // first byte of the head in the text block
    uint64_t head_off;          // the head's bytes in the heads block
    uint32_t head_len, flags;   // SW_ROW_CLOSE: a ']' behind the tail
};
constexpr uint32_t SW_ROW_CLOSE = 1;

// Every launcher takes a run of rows of a CSR: offsets[0 .. n_rows] are the rows' absolute positions in `hashes`, and
// h0 = offsets[0], n_hashes = offsets[n_rows] - h0 are known to the host.

// pos[j], j = 0 .. n_hashes: the bytes of "digits," of the hashes h0 .. h0 + j - 1 (an exclusive scan of digit count + 1)
size_t sw_positions_temp_bytes(uint64_t n_hashes);
hipError_t sw_positions_launch(const uint64_t* d_hashes, uint64_t h0, uint64_t n_hashes, uint64_t* d_pos, void* d_tmp, size_t tmp_bytes, hipStream_t stream);
// text_len[r]: bytes of the row's `mins` text (digits and commas); msg_len[r]: bytes of its MD5 message (ksize digits + hash digits)
hipError_t sw_row_lengths_launch(const uint64_t* d_offsets, uint64_t n_rows, const uint64_t* d_pos, uint32_t ksize_digits, uint64_t* d_text_len,
                                 uint64_t* d_msg_len, hipStream_t stream);
// md5[16 r .. 16 r + 16) for the rows r = order[0 .. n_order): a lane per row, 64 consecutive entries of `order` per wave
hipError_t sw_md5_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, const uint32_t* d_order, uint64_t n_order, uint32_t ksize,
                         uint8_t* d_md5, hipStream_t stream);
// the digits and commas of every hash at its place in its row's document
hipError_t sw_text_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n_rows, uint64_t n_hashes, const uint64_t* d_pos,
                          const SwRow* d_rows, uint8_t* d_text, hipStream_t stream);
// heads copied, tails written: d_tail[0 .. tail_len) with the 32 hex digits of the row's md5 at md5_at
hipError_t sw_frame_rows_launch(const SwRow* d_rows, uint64_t n_rows, const uint64_t* d_text_len, const uint8_t* d_heads, const uint8_t* d_tail,
                                uint32_t tail_len, uint32_t md5_at, const uint8_t* d_md5, uint8_t* d_text, hipStream_t stream);

// bits[c]: the code bits of chunk c (end-of-block included in a member's last chunk).  d_table: SW_SYMBOLS entries of sw_build_table.
hipError_t sw_chunk_bits_launch(const uint8_t* d_text, const SwChunk* d_chunks, uint32_t n_chunks, const uint32_t* d_table, uint32_t* d_bits,
                                hipStream_t stream);
// the codes of every chunk ORed into d_out (32-bit words, zeroed by the caller; nothing is written at or beyond out_words)
hipError_t sw_pack_launch(const uint8_t* d_text, const SwChunk* d_chunks, uint32_t n_chunks, const uint32_t* d_table, uint32_t* d_out, uint64_t out_words,
                          hipStream_t stream);
// stored blocks (BTYPE 00): chunk c's 5-byte block header at byte out_bit / 8, its bytes behind it
hipError_t sw_stored_launch(const uint8_t* d_text, const SwChunk* d_chunks, uint32_t n_chunks, uint8_t* d_out, hipStream_t stream);
// gzip header and trailer of every member; hdr_bits > 0: the block header's bits behind the gzip header (run after sw_pack_launch:
// the header's last, partial byte is ORed onto the first codes)
hipError_t sw_frame_members_launch(const SwMember* d_members, uint32_t n_members, const uint8_t* d_hdr, uint32_t hdr_bits, uint8_t* d_out,
                                   hipStream_t stream);

}  // namespace smg
