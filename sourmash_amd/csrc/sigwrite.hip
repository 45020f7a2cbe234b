// sigwrite.hip -- a SketchSet's rows turned into signature JSON, MD5 identities and gzip members on the device.
//
// What the reference does here: SaveSignatures_SigFile / _ZipFile (src/sourmash/save_load.py:406-540) serialise one signature at a
// time -- serde_json writes the hashes as decimal text, md5 runs over the same digits once more (minhash.rs:290-307), zlib level 1
// compresses the document.  All of it is per hash or per row and independent, so for a CSR resident in HBM:
//   sw_positions        an exclusive scan of (digit count + 1) over the hashes: where every number's text begins in its row
//   sw_row_lengths      a lane per row: bytes of its `mins` text and of its MD5 message, from the scan's values at the row's ends
//   sw_md5_kernel       a lane per row, rows handed out in order of size so that a wave's 64 rows are of similar length: the
//                       message streams through a 128-byte ring per lane in LDS (the 64 rings interleaved word by word), 64
//                       compression rounds per block in registers                                  (VALU; the rounds of a row are serial)
//   sw_text_kernel      a lane per hash: its row by binary search in the offsets, its digits and comma at the scanned place
//   sw_frame_rows       a wave per row: the head the host built (metadata, escaped by json::write_string), the tail with the md5's hex
//   sw_chunk_bits       a block per chunk of a document: the sum of its bytes' code lengths
//   sw_pack_kernel      a block per chunk: lanes own stretches of the chunk, a prefix sum of their bit counts, codes composed in
//                       registers and ORed into the chunk's words in LDS, whole words stored (OR only at the two seams)
//   sw_stored_kernel    compression 0: stored blocks of up to 65,535 bytes
//   sw_frame_members    gzip header, block header bits, CRC-32 and ISIZE of every member
// The CRC-32 is gunzip.hip's gz_crc_kernel.  The rules (digits, MD5, the code, a lane's share of a chunk) are in
// sigwrite_core.hpp, which also compiles for the host: tests/native/sigwrite_emul.cpp walks them with lanes as loop indices.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "sigwrite_api.hpp"

namespace smg {

namespace {

struct SwDigitsPlusComma {
    const uint64_t* h;
    uint64_t n;
    __host__ __device__ uint64_t operator()(uint64_t j) const { return j < n ? (uint64_t)sw_digit_count(h[j]) + 1u : 0u; }
};

__global__ __launch_bounds__(256) void sw_row_lengths_kernel(const uint64_t* __restrict__ offsets, uint64_t n_rows, const uint64_t* __restrict__ pos,
                                                             uint32_t ksize_digits, uint64_t* __restrict__ text_len, uint64_t* __restrict__ msg_len) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t h0 = offsets[0], a = offsets[r] - h0, b = offsets[r + 1] - h0;
    const uint64_t with_commas = pos[b] - pos[a];                   // every number with a comma behind it
    text_len[r] = b > a ? with_commas - 1u : 0u;
    msg_len[r] = ksize_digits + with_commas - (b - a);
}

__global__ __launch_bounds__(64) void sw_md5_kernel(const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ offsets,
                                                    const uint32_t* __restrict__ order, uint64_t n_order, uint32_t ksize, uint8_t* __restrict__ md5) {
    __shared__ uint32_t rings[32 * 64];
    const uint32_t lane = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * 64u + lane;
    if (i >= n_order) return;
    const uint32_t r = order[i];
    const uint64_t a = offsets[r], b = offsets[r + 1];
    const SwRing ring{rings + lane, 64u};
    sw_md5_row(ring, ksize, hashes + a, b - a, md5 + 16ull * r);
}

__global__ __launch_bounds__(256) void sw_text_kernel(const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ offsets, uint64_t n_rows,
                                                      uint64_t n_hashes, const uint64_t* __restrict__ pos, const SwRow* __restrict__ rows,
                                                      uint8_t* __restrict__ text) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n_hashes) return;
    const uint64_t h0 = offsets[0], i = h0 + j;
    uint64_t lo = 0, hi = n_rows;                                   // the last row r with offsets[r] <= i (empty rows in front of it share its offset)
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const SwRow row = rows[lo];
    const uint64_t v = hashes[i];
    const uint32_t nd = sw_digit_count(v);
    uint8_t* dst = text + row.doc_off + row.head_len + (pos[j] - pos[offsets[lo] - h0]);
    sw_put_decimal(v, nd, [&](uint32_t k, uint8_t b) { dst[k] = b; });
    if (i + 1 < offsets[lo + 1]) dst[nd] = ',';
}

__global__ __launch_bounds__(64) void sw_frame_rows_kernel(const SwRow* __restrict__ rows, uint64_t n_rows, const uint64_t* __restrict__ text_len,
                                                           const uint8_t* __restrict__ heads, const uint8_t* __restrict__ tail, uint32_t tail_len,
                                                           uint32_t md5_at, const uint8_t* __restrict__ md5, uint8_t* __restrict__ text) {
    const uint64_t r = blockIdx.x;
    if (r >= n_rows) return;
    const SwRow row = rows[r];
    const uint32_t lane = threadIdx.x;
    uint8_t* doc = text + row.doc_off;
    for (uint32_t i = lane; i < row.head_len; i += 64u) doc[i] = heads[row.head_off + i];
    uint8_t* t = doc + row.head_len + text_len[r];
    for (uint32_t i = lane; i < tail_len; i += 64u) {
        uint8_t b = tail[i];
        if (i >= md5_at && i < md5_at + 32u) {
            const uint32_t k = i - md5_at;
            const uint32_t nib = (md5[16ull * r + (k >> 1)] >> ((k & 1u) ? 0u : 4u)) & 15u;
            b = (uint8_t)(nib < 10u ? '0' + nib : 'a' + nib - 10u);
        }
        t[i] = b;
    }
    if (lane == 0 && (row.flags & SW_ROW_CLOSE)) t[tail_len] = ']';
}

__global__ __launch_bounds__(256) void sw_chunk_bits_kernel(const uint8_t* __restrict__ text, const SwChunk* __restrict__ chunks,
                                                            const uint32_t* __restrict__ table_g, uint32_t* __restrict__ bits_out) {
    __shared__ uint32_t table[SW_SYMBOLS];
    __shared__ uint32_t part[4];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < SW_SYMBOLS; i += 256u) table[i] = table_g[i];
    __syncthreads();
    const SwChunk c = chunks[blockIdx.x];
    const uint8_t* p = text + c.in_off;
    uint32_t bits = 0;
    for (uint32_t i = t; i < c.in_len; i += 256u) bits += sw_entry_len(table[p[i]]);
    if (t == 0 && (c.flags & SW_CHUNK_LAST)) bits += sw_entry_len(table[SW_EOB]);
#pragma unroll
    for (int o = 32; o; o >>= 1) bits += __shfl_xor(bits, o);
    if ((t & 63u) == 0) part[t >> 6] = bits;
    __syncthreads();
    if (t == 0) bits_out[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void sw_pack_kernel(const uint8_t* __restrict__ text, const SwChunk* __restrict__ chunks,
                                                      const uint32_t* __restrict__ table_g, uint32_t* __restrict__ out, uint64_t out_words) {
    __shared__ uint32_t table[SW_SYMBOLS];
    __shared__ uint32_t words[SW_CHUNK_WORDS];
    __shared__ uint32_t txt4[SW_MAX_CHUNK / 4];
    __shared__ uint32_t part[4];
    uint8_t* txt = reinterpret_cast<uint8_t*>(txt4);
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const SwChunk c = chunks[blockIdx.x];
    if (c.in_len > SW_MAX_CHUNK) return;                            // (the host never makes one)
    for (uint32_t i = t; i < SW_SYMBOLS; i += 256u) table[i] = table_g[i];
    for (uint32_t i = t; i < SW_CHUNK_WORDS; i += 256u) words[i] = 0u;
    const uint8_t* p = text + c.in_off;
    for (uint32_t i = t; i < c.in_len; i += 256u) txt[i] = p[i];
    __syncthreads();
    const uint32_t lo = sw_lane_lo(c.in_len, t, 256u), hi = sw_lane_hi(c.in_len, t, 256u);
    const bool eob = (c.flags & SW_CHUNK_LAST) && t == 255u;
    const uint32_t bits = sw_lane_bits(txt, lo, hi, table, eob);
    // exclusive prefix sum over the block's 256 lanes
    uint32_t incl = bits;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if (lane >= (uint32_t)o) incl += u; }
    if (lane == 63u) part[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) { const uint32_t s = part[w]; if (w < wave) before += s; total += s; }
    const uint32_t bit0 = (uint32_t)(c.out_bit & 31u);
    sw_lane_pack(txt, lo, hi, table, eob, bit0 + before + incl - bits, [&](uint32_t w, uint32_t v) { atomicOr(&words[w], v); });
    __syncthreads();
    const uint32_t nw = sw_chunk_words(c.out_bit, total);
    const uint64_t w0 = c.out_bit >> 5;
    for (uint32_t w = t; w < nw; w += 256u) {
        if (w0 + w >= out_words) break;
        const uint32_t v = words[w];
        if (w == 0 || w == nw - 1u) { if (v) atomicOr(&out[w0 + w], v); }
        else out[w0 + w] = v;
    }
}

__global__ __launch_bounds__(256) void sw_stored_kernel(const uint8_t* __restrict__ text, const SwChunk* __restrict__ chunks, uint8_t* __restrict__ out) {
    const SwChunk c = chunks[blockIdx.x];
    const uint32_t t = threadIdx.x;
    uint8_t* o = out + (c.out_bit >> 3);
    if (t == 0) o[0] = (c.flags & SW_CHUNK_LAST) ? 1 : 0;          // BFINAL, BTYPE 00
    if (t == 1) o[1] = (uint8_t)c.in_len;
    if (t == 2) o[2] = (uint8_t)(c.in_len >> 8);
    if (t == 3) o[3] = (uint8_t)~c.in_len;
    if (t == 4) o[4] = (uint8_t)(~c.in_len >> 8);
    const uint8_t* p = text + c.in_off;
    for (uint32_t i = t; i < c.in_len; i += 256u) o[5 + i] = p[i];
}

__global__ __launch_bounds__(64) void sw_frame_members_kernel(const SwMember* __restrict__ members, const uint8_t* __restrict__ hdr, uint32_t hdr_bits,
                                                              uint8_t* __restrict__ out) {
    const SwMember m = members[blockIdx.x];
    const uint32_t t = threadIdx.x;
    uint8_t* o = out + m.out_off;
    if (t < SW_GZIP_HEADER) o[t] = sw_gzip_header_byte(t);
    const uint32_t hdr_bytes = (hdr_bits + 7u) >> 3;
    for (uint32_t i = t; i < hdr_bytes; i += 64u) {
        if (i * 8u + 8u <= hdr_bits) o[SW_GZIP_HEADER + i] = hdr[i];
        else o[SW_GZIP_HEADER + i] |= hdr[i];                       // the first codes share this byte (this lane alone touches it here)
    }
    uint8_t* tr = o + m.out_len - SW_GZIP_TRAILER;
    if (t < 4) tr[t] = (uint8_t)(m.crc >> (8u * t));
    else if (t < 8) tr[t] = (uint8_t)(m.isize >> (8u * (t - 4u)));
}

}  // namespace

size_t sw_positions_temp_bytes(uint64_t n_hashes) {
    size_t bytes = 0;
    auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), SwDigitsPlusComma{nullptr, 0});
    (void)rocprim::exclusive_scan(nullptr, bytes, in, (uint64_t*)nullptr, (uint64_t)0, (size_t)n_hashes + 1, rocprim::plus<uint64_t>(), (hipStream_t)0);
    return bytes ? bytes : 8;
}

hipError_t sw_positions_launch(const uint64_t* d_hashes, uint64_t h0, uint64_t n_hashes, uint64_t* d_pos, void* d_tmp, size_t tmp_bytes, hipStream_t stream) {
    auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), SwDigitsPlusComma{d_hashes + h0, n_hashes});
    return rocprim::exclusive_scan(d_tmp, tmp_bytes, in, d_pos, (uint64_t)0, (size_t)n_hashes + 1, rocprim::plus<uint64_t>(), stream);
}

hipError_t sw_row_lengths_launch(const uint64_t* d_offsets, uint64_t n_rows, const uint64_t* d_pos, uint32_t ksize_digits, uint64_t* d_text_len,
                                 uint64_t* d_msg_len, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    const uint64_t blocks = (n_rows + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_row_lengths_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_offsets, n_rows, d_pos, ksize_digits, d_text_len, d_msg_len);
    return hipGetLastError();
}

hipError_t sw_md5_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, const uint32_t* d_order, uint64_t n_order, uint32_t ksize, uint8_t* d_md5,
                         hipStream_t stream) {
    if (n_order == 0) return hipSuccess;
    const uint64_t blocks = (n_order + 63) / 64;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_md5_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, d_hashes, d_offsets, d_order, n_order, ksize, d_md5);
    return hipGetLastError();
}

hipError_t sw_text_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n_rows, uint64_t n_hashes, const uint64_t* d_pos,
                          const SwRow* d_rows, uint8_t* d_text, hipStream_t stream) {
    if (n_hashes == 0 || n_rows == 0) return hipSuccess;
    const uint64_t blocks = (n_hashes + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_text_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_hashes, d_offsets, n_rows, n_hashes, d_pos, d_rows, d_text);
    return hipGetLastError();
}

hipError_t sw_frame_rows_launch(const SwRow* d_rows, uint64_t n_rows, const uint64_t* d_text_len, const uint8_t* d_heads, const uint8_t* d_tail,
                                uint32_t tail_len, uint32_t md5_at, const uint8_t* d_md5, uint8_t* d_text, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    if (n_rows > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_frame_rows_kernel, dim3((unsigned)n_rows), dim3(64), 0, stream, d_rows, n_rows, d_text_len, d_heads, d_tail, tail_len, md5_at, d_md5,
                       d_text);
    return hipGetLastError();
}

hipError_t sw_chunk_bits_launch(const uint8_t* d_text, const SwChunk* d_chunks, uint32_t n_chunks, const uint32_t* d_table, uint32_t* d_bits,
                                hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(sw_chunk_bits_kernel, dim3(n_chunks), dim3(256), 0, stream, d_text, d_chunks, d_table, d_bits);
    return hipGetLastError();
}

hipError_t sw_pack_launch(const uint8_t* d_text, const SwChunk* d_chunks, uint32_t n_chunks, const uint32_t* d_table, uint32_t* d_out, uint64_t out_words,
                          hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(sw_pack_kernel, dim3(n_chunks), dim3(256), 0, stream, d_text, d_chunks, d_table, d_out, out_words);
    return hipGetLastError();
}

hipError_t sw_stored_launch(const uint8_t* d_text, const SwChunk* d_chunks, uint32_t n_chunks, uint8_t* d_out, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(sw_stored_kernel, dim3(n_chunks), dim3(256), 0, stream, d_text, d_chunks, d_out);
    return hipGetLastError();
}

hipError_t sw_frame_members_launch(const SwMember* d_members, uint32_t n_members, const uint8_t* d_hdr, uint32_t hdr_bits, uint8_t* d_out,
                                   hipStream_t stream) {
    if (n_members == 0) return hipSuccess;
    hipLaunchKernelGGL(sw_frame_members_kernel, dim3(n_members), dim3(64), 0, stream, d_members, d_hdr, hdr_bits, d_out);
    return hipGetLastError();
}

}  // namespace smg
