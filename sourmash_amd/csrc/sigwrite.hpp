// sigwrite.hpp -- the host side of the signature writer: a SketchSet's rows written as .sig / .sig.gz / .zip from the device.
//
// The counterpart of sigload.hpp, and of the reference's SaveSignatures_SigFile / SaveSignatures_ZipFile
// (src/sourmash/save_load.py:406-540).  Rows are taken in batches bounded by bytes of text (SW_BATCH_BYTES); for a batch
//   lengths   sw_positions + sw_row_lengths: where every number's text begins, how long every row's text and MD5 message are
//   md5       sw_md5_kernel over the rows in order of message length; rows above the long-row bound go to md5.hpp on a worker
//             thread while the kernel runs
//   text      the host builds every row's head (metadata, escaped by json::write_string) and lays the documents out; sw_text_kernel
//             and sw_frame_rows write them
//   crc       gunzip.hip's CRC-32 kernel over 64 KB pieces, joined per document (inflate_core.hpp: crc_join)
//   pack      a sum of code lengths per chunk, the chunks' first bits by a running sum per member, sw_pack_kernel (compression 0:
//             stored blocks), gzip header and trailer of every member
// and the bytes leave through the pinned ring of hostxfer.hpp.  What stays on the host: the heads, the lay-out (a running sum per
// row and per chunk), the zip records, the manifest (collection.hpp: manifest_to_csv, deflated by zlib as the reference does)
// and the duplicate rule of ZipStorage._generate_filename (sbt_storage.py:242-265).
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <exception>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "collection.hpp"
#include "device_ctx.hpp"
#include "gunzip_api.hpp"
#include "hostxfer.hpp"
#include "inflate_core.hpp"
#include "md5.hpp"
#include "signature_host.hpp"
#include "sigwrite_api.hpp"

namespace smg {

// A block of the message is about 3,000 instructions for a lane (the digits of ~4 hashes by division, the byte stores into the ring,
// 64 rounds): about 7 us when the wave has its SIMD to itself.  A message of 256 KiB (~15,000 hashes) keeps its lane -- and the wave
// it sits in, and the batch that waits for it -- for about 30 ms; the host's md5.hpp does ~500 MB/s, 0.5 ms for the same row, and
// runs while the kernel does the rest.  Below the bound the device wins through numbers, above it rows are rare and one of them
// would be the whole batch's time (a sketch of 10^7 hashes would hold one lane for 20 seconds).  DESIGN 4.14.
constexpr uint64_t SW_MD5_HOST_BOUND = (uint64_t)256 << 10;
constexpr uint64_t SW_BATCH_BYTES = (uint64_t)128 << 20;           // text of a batch of rows (a single larger row is a batch of its own)
constexpr uint32_t SW_PACK_CHUNK = SW_MAX_CHUNK;
constexpr uint64_t SW_DOC_ALIGN = 16;                               // documents and members begin on 16-byte lines (the CRC kernel loads 16 bytes a lane)

struct SwStats {
    double lengths_ms = 0, md5_ms = 0, text_ms = 0, crc_ms = 0, pack_ms = 0, d2h_ms = 0, write_ms = 0;
    uint64_t rows = 0, hashes = 0, text_bytes = 0, out_bytes = 0, md5_host_rows = 0;
};
// (the counters and the tables below are used under the device context's lock, which every entry of the writer takes, the raw ones too)
inline SwStats& sigwrite_stats() { static SwStats s; return s; }

// rows [0, n) of a CSR in HBM and what their signatures say besides the hashes
struct SwSource {
    const uint64_t* d_hashes = nullptr;
    const uint64_t* d_offsets = nullptr;
    const uint64_t* h_offsets = nullptr;                            // the same offsets on the host
    uint64_t n = 0;
    uint32_t ksize = 0, hash_function = HF_DNA;                     // ksize as the set holds it (amino acids for protein sketches)
    uint64_t seed = 42, max_hash = 0, num = 0;
    const std::vector<ManifestRow>* rows = nullptr;                 // names / file names; may be missing or empty
    const char* const* names = nullptr;                             // the caller's, in front of the manifest rows'
    const char* const* filenames = nullptr;
    uint32_t json_ksize() const { return ksize * (hash_function == HF_DNA ? 1u : 3u); }
    std::string name(uint64_t r) const { return names ? std::string(names[r] ? names[r] : "") : rows && r < rows->size() ? (*rows)[r].name : std::string(); }
    std::string filename(uint64_t r) const {
        return filenames ? std::string(filenames[r] ? filenames[r] : "") : rows && r < rows->size() ? (*rows)[r].filename : std::string();
    }
};

namespace swdetail {

using clk = std::chrono::steady_clock;
inline double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }
inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// the code table and the block header, in HBM for as long as the library lives
struct Tables {
    uint32_t* d_table = nullptr;
    uint8_t* d_hdr = nullptr;
    std::vector<uint8_t> hdr;
    uint32_t hdr_bits = 0;
    uint32_t table[SW_SYMBOLS];
};
inline Tables& tables(hipStream_t st) {
    static Tables* t = nullptr;
    if (!t) {
        std::unique_ptr<Tables> n(new Tables());
        sw_build_table(n->table);
        n->hdr_bits = sw_build_block_header(n->hdr);
        void* p = nullptr;
        hip_check(arena_alloc(&p, sizeof(n->table) + n->hdr.size() + 64, st), "arena_alloc");
        n->d_table = static_cast<uint32_t*>(p);
        n->d_hdr = static_cast<uint8_t*>(p) + sizeof(n->table);
        hip_check(hipMemcpyAsync(n->d_table, n->table, sizeof(n->table), hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipMemcpyAsync(n->d_hdr, n->hdr.data(), n->hdr.size(), hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipStreamSynchronize(st), "sync");
        t = n.release();
    }
    return *t;
}

template <class T>
inline void upload(AsyncBuf& buf, const std::vector<T>& v, hipStream_t st) {
    buf.reset(v.size() * sizeof(T) + 16, st);
    if (!v.empty()) hip_check(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st), "H2D");
}

// CRC-32 of data[off[i], off[i] + len[i]) for every i (off: multiples of 16)
inline std::vector<uint32_t> crc_docs(const uint8_t* d_data, const std::vector<uint64_t>& off, const std::vector<uint64_t>& len, hipStream_t st) {
    std::vector<GzChunk> chunks;
    std::vector<size_t> first(off.size() + 1, 0);
    for (size_t i = 0; i < off.size(); ++i) {
        first[i] = chunks.size();
        for (uint64_t f = 0; f < len[i]; f += 65536) chunks.push_back(GzChunk{off[i] + f, (uint32_t)std::min<uint64_t>(65536, len[i] - f), 0});
    }
    first[off.size()] = chunks.size();
    if (chunks.size() > 0x7fffffffull) throw err_internal("sigwrite: too many CRC pieces in one batch");
    std::vector<uint32_t> part(chunks.size()), out(off.size(), 0);
    if (!chunks.empty()) {
        AsyncBuf d_chunks, d_crc(chunks.size() * 4 + 8, st);
        upload(d_chunks, chunks, st);
        hip_check(gz_crc_launch(d_data, d_chunks.as<GzChunk>(), (uint32_t)chunks.size(), d_crc.as<uint32_t>(), st), "gz_crc");
        hip_check(hipMemcpyAsync(part.data(), d_crc.p, part.size() * 4, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
    }
    const uint32_t x64k = inf::crc_xpow8(65536);
    for (size_t i = 0; i < off.size(); ++i) {
        uint32_t c = 0;
        for (size_t k = first[i]; k < first[i + 1]; ++k)
            c = k == first[i] ? part[k]                              // (nothing in front: a million one-piece documents need no polynomial powers)
              : chunks[k].len == 65536u ? inf::crc_join(c, part[k], x64k) : inf::crc_join(c, part[k], inf::crc_xpow8(chunks[k].len));
        out[i] = c;
    }
    return out;
}

}  // namespace swdetail

// ---- MD5 of the rows of a CSR ----------------------------------------------------------------------------------------------------
// d_md5[16 r ..): the digest of row r, r < n.  msg_len: every row's message length.  Rows above `bound` bytes are the host's.
// -> rows the host did.
inline uint64_t sw_md5_rows(const uint64_t* d_hashes, const uint64_t* d_offsets, const uint64_t* h_offsets, uint64_t n, uint32_t ksize,
                            const std::vector<uint64_t>& msg_len, uint64_t bound, uint8_t* d_md5, hipStream_t st) {
    if (n == 0) return 0;
    if (n > 0xffffffffull) throw err_internal("sigwrite: more than 2^32 rows in one batch");
    // the device's rows, longest first (a counting sort by 64-byte blocks; a wave's 64 lanes get neighbours of this order)
    std::vector<uint32_t> order, longs;
    uint64_t max_blocks = 0;
    for (uint64_t r = 0; r < n; ++r)
        if (msg_len[r] <= bound) max_blocks = std::max(max_blocks, sw_md5_padded_len(msg_len[r]) / 64);
    std::vector<uint64_t> start(max_blocks + 2, 0);
    for (uint64_t r = 0; r < n; ++r) {
        if (msg_len[r] > bound) longs.push_back((uint32_t)r);
        else start[max_blocks - sw_md5_padded_len(msg_len[r]) / 64 + 1]++;
    }
    for (size_t b = 1; b < start.size(); ++b) start[b] += start[b - 1];
    order.resize(n - longs.size());
    for (uint64_t r = 0; r < n; ++r)
        if (msg_len[r] <= bound) order[start[max_blocks - sw_md5_padded_len(msg_len[r]) / 64]++] = (uint32_t)r;
    // the long rows' hashes come down first; a worker thread hashes them while this thread uploads the order, launches the
    // kernel and waits for it
    std::vector<std::vector<uint64_t>> long_hashes(longs.size());
    for (size_t i = 0; i < longs.size(); ++i) {
        const uint64_t a = h_offsets[longs[i]], b = h_offsets[longs[i] + 1];
        long_hashes[i].resize(b - a);
        HostXfer::get().device_to_host(long_hashes[i].data(), d_hashes + a, (b - a) * 8, st);
    }
    std::vector<uint8_t> digests(longs.size() * 16);
    std::exception_ptr failed;
    std::thread worker;
    struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } } join{worker};     // (also when the launch below throws)
    if (!longs.empty())
        worker = std::thread([&] {
            try {
                for (size_t i = 0; i < longs.size(); ++i) {
                    Md5 m;
                    m.update_decimal(ksize);
                    for (uint64_t h : long_hashes[i]) m.update_decimal(h);
                    const std::string hex = m.hexdigest();
                    auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
                    for (int k = 0; k < 16; ++k) digests[i * 16 + k] = (uint8_t)(nib(hex[2 * k]) << 4 | nib(hex[2 * k + 1]));
                }
            } catch (...) { failed = std::current_exception(); }
        });
    AsyncBuf d_order;
    swdetail::upload(d_order, order, st);
    hip_check(sw_md5_launch(d_hashes, d_offsets, d_order.as<uint32_t>(), order.size(), ksize, d_md5, st), "sw_md5");
    hip_check(hipStreamSynchronize(st), "sync");                    // (the order's host copy is done with; the kernel is through)
    if (worker.joinable()) worker.join();
    if (failed) std::rethrow_exception(failed);
    for (size_t i = 0; i < longs.size(); ++i)
        hip_check(hipMemcpyAsync(d_md5 + 16ull * longs[i], &digests[i * 16], 16, hipMemcpyHostToDevice, st), "H2D");
    hip_check(hipStreamSynchronize(st), "sync");
    return longs.size();
}

// ---- the documents of a run of rows --------------------------------------------------------------------------------------------
struct SwBatch {
    AsyncBuf text;                                                  // the documents
    uint64_t text_bytes = 0;                                        // the block's extent
    std::vector<uint64_t> doc_off, doc_len;                         // per row
    std::vector<uint8_t> md5;                                       // 16 bytes per row
};

// the pieces of a document that do not depend on the row's hashes, cut from Signature::to_json of an empty sketch
struct SwTemplate {
    std::string before_filename, before_mins, tail;                 // {"class":...,"filename":  |  ,"license":...,"mins":[  |  ],"md5sum":"...
    uint32_t md5_at = 0;
    explicit SwTemplate(const SwSource& src) {
        Signature sig;
        KmerMinHash mh(0, src.json_ksize(), src.hash_function, src.seed, false, (uint32_t)src.num);
        mh.max_hash = src.max_hash;
        sig.sketches.push_back(mh);
        std::string s;
        sig.to_json(s);
        const size_t f = s.find("\"filename\":null"), m = s.find("\"mins\":["), t = s.find("\"md5sum\":\"");
        if (f == std::string::npos || m == std::string::npos || t == std::string::npos) throw err_internal("sigwrite: unexpected signature layout");
        before_filename = s.substr(0, f + 11);
        before_mins = s.substr(f + 15, m + 8 - (f + 15));
        tail = s.substr(m + 8);
        md5_at = (uint32_t)(t + 10 - (m + 8));
    }
    void head(std::string& out, const std::string& name, const std::string& filename) const {
        out += before_filename;
        if (filename.empty()) out += "null"; else json::write_string(out, filename);
        if (!name.empty()) { out += ",\"name\":"; json::write_string(out, name); }
        out += before_mins;
    }
};

// Rows [r0, r1) of the source.  per_doc: every row a document of its own, `[{...}]`, on a 16-byte line; otherwise the rows
// follow each other as the elements of one array, '[' in front of the first row if `open`, ']' behind the last if `close`.
inline void sw_build_batch(const SwSource& src, uint64_t r0, uint64_t r1, bool per_doc, bool open, bool close, uint64_t md5_bound, SwBatch& out,
                           hipStream_t st) {
    using namespace swdetail;
    SwStats& stats = sigwrite_stats();
    const uint64_t n = r1 - r0;
    const uint64_t h0 = src.h_offsets[r0], nh = src.h_offsets[r1] - h0;
    const uint64_t* d_off = src.d_offsets + r0;
    out.doc_off.assign(n, 0); out.doc_len.assign(n, 0); out.md5.assign(n * 16, 0);
    out.text_bytes = 0;
    if (n == 0) return;
    if (n > 0x7fffffffull) throw err_internal("sigwrite: too many rows in one batch");
    // ---- lengths ----
    auto t0 = clk::now();
    const size_t tmp_bytes = sw_positions_temp_bytes(nh);
    AsyncBuf d_pos((nh + 2) * 8, st), d_tmp(tmp_bytes, st), d_text_len(n * 8, st), d_msg_len(n * 8, st), d_md5(n * 16, st);
    hip_check(sw_positions_launch(src.d_hashes, h0, nh, d_pos.as<uint64_t>(), d_tmp.p, tmp_bytes, st), "sw_positions");
    hip_check(sw_row_lengths_launch(d_off, n, d_pos.as<uint64_t>(), sw_digit_count(src.json_ksize()), d_text_len.as<uint64_t>(), d_msg_len.as<uint64_t>(), st),
              "sw_row_lengths");
    std::vector<uint64_t> text_len(n), msg_len(n);
    hip_check(hipMemcpyAsync(text_len.data(), d_text_len.p, n * 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipMemcpyAsync(msg_len.data(), d_msg_len.p, n * 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    stats.lengths_ms += ms_since(t0);
    // ---- md5 ----
    t0 = clk::now();
    stats.md5_host_rows += sw_md5_rows(src.d_hashes, d_off, src.h_offsets + r0, n, src.json_ksize(), msg_len, md5_bound, d_md5.as<uint8_t>(), st);
    hip_check(hipMemcpyAsync(out.md5.data(), d_md5.p, n * 16, hipMemcpyDeviceToHost, st), "D2H");
    stats.md5_ms += ms_since(t0);
    // ---- heads and lay-out ----
    t0 = clk::now();
    const SwTemplate tpl(src);
    std::string heads;
    std::vector<SwRow> rows(n);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i) {
        SwRow& row = rows[i];
        row.head_off = heads.size();
        heads += per_doc ? '[' : (i == 0 && open) ? '[' : ',';
        tpl.head(heads, src.name(r0 + i), src.filename(r0 + i));
        row.head_len = (uint32_t)(heads.size() - row.head_off);
        row.flags = per_doc || (close && i + 1 == n) ? SW_ROW_CLOSE : 0u;
        if (per_doc) at = align_up(at, SW_DOC_ALIGN);
        row.doc_off = at;
        out.doc_off[i] = at;
        out.doc_len[i] = row.head_len + text_len[i] + tpl.tail.size() + (row.flags & SW_ROW_CLOSE ? 1 : 0);
        at += out.doc_len[i];
    }
    out.text_bytes = at;
    const uint64_t tail_off = heads.size();
    heads += tpl.tail;
    out.text.reset(at + 64, st);
    AsyncBuf d_heads(heads.size() + 16, st), d_rows;
    hip_check(hipMemcpyAsync(d_heads.p, heads.data(), heads.size(), hipMemcpyHostToDevice, st), "H2D");
    upload(d_rows, rows, st);
    if (per_doc) hip_check(hipMemsetAsync(out.text.p, 0, at + 64, st), "memset");          // (the gaps between documents)
    hip_check(sw_text_launch(src.d_hashes, d_off, n, nh, d_pos.as<uint64_t>(), d_rows.as<SwRow>(), out.text.as<uint8_t>(), st), "sw_text");
    hip_check(sw_frame_rows_launch(d_rows.as<SwRow>(), n, d_text_len.as<uint64_t>(), d_heads.as<uint8_t>(), d_heads.as<uint8_t>() + tail_off,
                                   (uint32_t)tpl.tail.size(), tpl.md5_at, d_md5.as<uint8_t>(), out.text.as<uint8_t>(), st), "sw_frame_rows");
    hip_check(hipStreamSynchronize(st), "sync");
    stats.text_ms += ms_since(t0);
    stats.rows += n; stats.hashes += nh; stats.text_bytes += at;
}

// ---- gzip members of documents -------------------------------------------------------------------------------------------------
struct SwPacked {
    AsyncBuf out;
    uint64_t out_bytes = 0;
    std::vector<uint64_t> off, len;                                 // the members
    std::vector<uint32_t> text_crc;
};

struct SwLayout {
    std::vector<SwChunk> chunks;
    std::vector<size_t> first;                                      // first[d] .. first[d + 1]: the chunks of document d
};
inline void sw_cut_chunks(const std::vector<uint64_t>& off, const std::vector<uint64_t>& len, uint32_t csize, SwLayout& lay) {
    lay.chunks.clear(); lay.first.assign(off.size() + 1, 0);
    for (size_t d = 0; d < off.size(); ++d) {
        lay.first[d] = lay.chunks.size();
        uint64_t o = 0;
        do {                                                        // (a document of no bytes has one chunk of no bytes: it carries the end-of-block)
            SwChunk c;
            c.in_off = off[d] + o; c.in_len = (uint32_t)std::min<uint64_t>(csize, len[d] - o);
            c.flags = o + csize >= len[d] ? SW_CHUNK_LAST : 0u; c.out_bit = 0;
            lay.chunks.push_back(c);
            o += csize;
        } while (o < len[d]);
    }
    lay.first[off.size()] = lay.chunks.size();
    if (lay.chunks.size() > 0x7fffffffull) throw err_internal("sigwrite: too many chunks in one batch");
}

// every document [off[d], off[d] + len[d]) of d_text as a gzip member of its own: compression 0 stored blocks, otherwise one
// dynamic-Huffman block of literals packed `chunk` bytes a workgroup
inline void sw_deflate_docs(const uint8_t* d_text, const std::vector<uint64_t>& off, const std::vector<uint64_t>& len, int compression, uint32_t chunk,
                            SwPacked& out, hipStream_t st) {
    using namespace swdetail;
    SwStats& stats = sigwrite_stats();
    const size_t n = off.size();
    out.off.assign(n, 0); out.len.assign(n, 0); out.out_bytes = 0;
    if (n == 0) return;
    if (chunk == 0 || chunk > SW_MAX_CHUNK) throw err_internal("sigwrite: the chunk size must be 1 .. " + std::to_string(SW_MAX_CHUNK));
    auto t0 = clk::now();
    out.text_crc = crc_docs(d_text, off, len, st);
    stats.crc_ms += ms_since(t0);
    t0 = clk::now();
    Tables& tab = tables(st);
    SwLayout lay;
    sw_cut_chunks(off, len, compression ? chunk : SW_STORED_MAX, lay);
    AsyncBuf d_chunks;
    std::vector<uint32_t> bits(lay.chunks.size(), 0);
    if (compression) {
        upload(d_chunks, lay.chunks, st);
        AsyncBuf d_bits(bits.size() * 4 + 8, st);
        hip_check(sw_chunk_bits_launch(d_text, d_chunks.as<SwChunk>(), (uint32_t)lay.chunks.size(), tab.d_table, d_bits.as<uint32_t>(), st), "sw_chunk_bits");
        hip_check(hipMemcpyAsync(bits.data(), d_bits.p, bits.size() * 4, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
    }
    std::vector<SwMember> members(n);
    uint64_t at = 0;
    for (size_t d = 0; d < n; ++d) {
        at = align_up(at, SW_DOC_ALIGN);
        const uint64_t begin = at + SW_GZIP_HEADER;
        uint64_t end;
        if (compression) {
            uint64_t bit = begin * 8 + tab.hdr_bits;
            for (size_t c = lay.first[d]; c < lay.first[d + 1]; ++c) { lay.chunks[c].out_bit = bit; bit += bits[c]; }
            end = (bit + 7) / 8;
        } else {
            uint64_t byte = begin;
            for (size_t c = lay.first[d]; c < lay.first[d + 1]; ++c) { lay.chunks[c].out_bit = byte * 8; byte += 5 + lay.chunks[c].in_len; }
            end = byte;
        }
        members[d] = SwMember{at, end + SW_GZIP_TRAILER - at, out.text_crc[d], (uint32_t)len[d]};
        out.off[d] = at; out.len[d] = members[d].out_len;
        at = end + SW_GZIP_TRAILER;
    }
    out.out_bytes = at;
    const uint64_t out_words = (at + 3) / 4 + 1;
    out.out.reset(out_words * 4 + 64, st);
    hip_check(hipMemsetAsync(out.out.p, 0, out_words * 4 + 64, st), "memset");
    AsyncBuf d_members;
    upload(d_chunks, lay.chunks, st);
    upload(d_members, members, st);
    if (compression)
        hip_check(sw_pack_launch(d_text, d_chunks.as<SwChunk>(), (uint32_t)lay.chunks.size(), tab.d_table, out.out.as<uint32_t>(), out_words, st), "sw_pack");
    else
        hip_check(sw_stored_launch(d_text, d_chunks.as<SwChunk>(), (uint32_t)lay.chunks.size(), out.out.as<uint8_t>(), st), "sw_stored");
    hip_check(sw_frame_members_launch(d_members.as<SwMember>(), (uint32_t)n, tab.d_hdr, compression ? tab.hdr_bits : 0u, out.out.as<uint8_t>(), st),
              "sw_frame_members");
    hip_check(hipStreamSynchronize(st), "sync");
    stats.pack_ms += ms_since(t0);
}

// One gzip member whose text arrives in pieces (the batches of an array): every piece continues the deflate stream at the bit
// where the piece before ended; the host writes the member's header in front of the first piece and the trailer behind the last.
struct SwGzStream {
    int compression = 1;
    bool started = false;
    uint32_t carry_bits = 0;                                        // bits of the stream's last byte that are taken (0: the stream ends on a byte)
    uint8_t carry_byte = 0;
    uint32_t crc = 0;
    uint64_t isize = 0;

    // -> the bytes that are complete now
    void add(const uint8_t* d_text, uint64_t len, bool last, std::vector<uint8_t>& bytes, hipStream_t st) {
        using namespace swdetail;
        SwStats& stats = sigwrite_stats();
        auto t0 = clk::now();
        const uint32_t c = crc_docs(d_text, {0}, {len}, st)[0];
        crc = inf::crc_join(crc, c, inf::crc_xpow8(len));
        isize += len;
        stats.crc_ms += ms_since(t0);
        t0 = clk::now();
        Tables& tab = tables(st);
        SwLayout lay;
        sw_cut_chunks({0}, {len}, compression ? SW_PACK_CHUNK : SW_STORED_MAX, lay);
        if (!last) lay.chunks.back().flags = 0;
        const uint64_t begin = started ? 0 : SW_GZIP_HEADER;
        AsyncBuf d_chunks;
        uint64_t end_bit;
        if (compression) {
            std::vector<uint32_t> bits(lay.chunks.size(), 0);
            upload(d_chunks, lay.chunks, st);
            AsyncBuf d_bits(bits.size() * 4 + 8, st);
            hip_check(sw_chunk_bits_launch(d_text, d_chunks.as<SwChunk>(), (uint32_t)lay.chunks.size(), tab.d_table, d_bits.as<uint32_t>(), st), "sw_chunk_bits");
            hip_check(hipMemcpyAsync(bits.data(), d_bits.p, bits.size() * 4, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
            uint64_t bit = started ? carry_bits : begin * 8 + tab.hdr_bits;
            for (size_t k = 0; k < lay.chunks.size(); ++k) { lay.chunks[k].out_bit = bit; bit += bits[k]; }
            end_bit = bit;
        } else {
            uint64_t byte = begin;
            for (SwChunk& k : lay.chunks) { k.out_bit = byte * 8; byte += 5 + k.in_len; }
            end_bit = byte * 8;
        }
        const uint64_t n_bytes = (end_bit + 7) / 8, out_words = (n_bytes + 3) / 4 + 1;
        AsyncBuf d_out(out_words * 4 + 64, st);
        hip_check(hipMemsetAsync(d_out.p, 0, out_words * 4 + 64, st), "memset");
        upload(d_chunks, lay.chunks, st);
        if (compression)
            hip_check(sw_pack_launch(d_text, d_chunks.as<SwChunk>(), (uint32_t)lay.chunks.size(), tab.d_table, d_out.as<uint32_t>(), out_words, st), "sw_pack");
        else
            hip_check(sw_stored_launch(d_text, d_chunks.as<SwChunk>(), (uint32_t)lay.chunks.size(), d_out.as<uint8_t>(), st), "sw_stored");
        hip_check(hipStreamSynchronize(st), "sync");
        stats.pack_ms += ms_since(t0);
        t0 = clk::now();
        bytes.assign(n_bytes + SW_GZIP_TRAILER, 0);
        HostXfer::get().device_to_host(bytes.data(), d_out.p, n_bytes, st);
        stats.d2h_ms += ms_since(t0);
        bytes.resize(n_bytes);
        if (!started) {
            for (uint32_t i = 0; i < SW_GZIP_HEADER; ++i) bytes[i] = sw_gzip_header_byte(i);
            if (compression) for (size_t i = 0; i < tab.hdr.size(); ++i) bytes[SW_GZIP_HEADER + i] |= tab.hdr[i];
            started = true;
        } else if (carry_bits) bytes[0] |= carry_byte;
        carry_bits = (uint32_t)(end_bit & 7u);
        if (last) {
            for (int i = 0; i < 4; ++i) bytes.push_back((uint8_t)(crc >> (8 * i)));
            for (int i = 0; i < 4; ++i) bytes.push_back((uint8_t)(isize >> (8 * i)));
        } else if (carry_bits) {
            carry_byte = bytes.back();
            bytes.pop_back();
        }
    }
};

// ---- files ----------------------------------------------------------------------------------------------------------------------
// Written under a temporary name next to the target and renamed when complete: a failed write leaves no half-written file.
class SwFile {
  public:
    explicit SwFile(const std::string& path) : path_(path), tmp_(path + ".tmp.XXXXXX") {
        fd_ = ::mkstemp(&tmp_[0]);                                  // a name of its own next to the target, created exclusively
        if (fd_ < 0) throw Error(E_IO, "cannot create " + path + ": " + strerror(errno));
        const mode_t mask = ::umask(0);
        ::umask(mask);
        (void)::fchmod(fd_, 0666 & ~mask);                          // (mkstemp makes 0600: the file gets the mode open() would give it)
    }
    ~SwFile() { discard(); }
    SwFile(const SwFile&) = delete;
    SwFile& operator=(const SwFile&) = delete;
    void write(const void* p, size_t n) {
        const auto t0 = swdetail::clk::now();
        const char* c = static_cast<const char*>(p);
        while (n) {
            const ssize_t w = ::write(fd_, c, n);
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) { const std::string why = strerror(errno); discard(); throw Error(E_IO, "cannot write " + path_ + ": " + why); }
            c += w; n -= (size_t)w; pos_ += (uint64_t)w;
        }
        sigwrite_stats().write_ms += swdetail::ms_since(t0);
        sigwrite_stats().out_bytes += (uint64_t)(c - static_cast<const char*>(p));
    }
    uint64_t pos() const { return pos_; }
    bool is_open() const { return fd_ >= 0; }
    void commit() {
        if (fd_ < 0) throw Error(E_IO, "the output " + path_ + " is not open");
        const int rc = ::close(fd_);
        fd_ = -1;
        if (rc != 0 || ::rename(tmp_.c_str(), path_.c_str()) != 0) {
            const std::string why = strerror(errno);
            ::unlink(tmp_.c_str());
            throw Error(E_IO, "cannot write " + path_ + ": " + why);
        }
    }
    void discard() {
        if (fd_ >= 0) { ::close(fd_); fd_ = -1; ::unlink(tmp_.c_str()); }
    }

  private:
    std::string path_, tmp_;
    int fd_ = -1;
    uint64_t pos_ = 0;
};

// the records of an uncompressed zip as Python's zipfile writes them (zip64 where a count or an offset does not fit)
class SwZip {
  public:
    explicit SwZip(SwFile& f) : f_(f) {}
    // method 0 (stored) or 8 (deflated: `data` is the raw deflate stream, crc / size those of the plain bytes)
    void add(const std::string& name, const uint8_t* data, uint64_t comp_size, uint64_t size, uint32_t crc, uint16_t method) {
        Entry e{name, f_.pos(), comp_size, size, crc, method};
        const bool big = comp_size >= 0xffffffffull || size >= 0xffffffffull;
        std::string h;
        le32(h, 0x04034b50u); le16(h, big ? 45 : 20); le16(h, 0); le16(h, method); le16(h, 0); le16(h, DOS_DATE);
        le32(h, crc); le32(h, big ? 0xffffffffu : (uint32_t)comp_size); le32(h, big ? 0xffffffffu : (uint32_t)size);
        le16(h, (uint16_t)name.size()); le16(h, big ? 20 : 0);
        h += name;
        if (big) { le16(h, 1); le16(h, 16); le64(h, size); le64(h, comp_size); }
        f_.write(h.data(), h.size());
        f_.write(data, comp_size);
        entries_.push_back(std::move(e));
    }
    void finish() {
        const uint64_t cd_off = f_.pos();
        std::string cd;
        for (const Entry& e : entries_) {
            std::string x;                                          // zip64 extra: only the fields that overflowed, in this order
            if (e.size >= 0xffffffffull) le64(x, e.size);
            if (e.comp_size >= 0xffffffffull) le64(x, e.comp_size);
            if (e.offset >= 0xffffffffull) le64(x, e.offset);
            const uint16_t ver = x.empty() ? 20 : 45;
            le32(cd, 0x02014b50u); le16(cd, (uint16_t)(3 << 8 | ver)); le16(cd, ver); le16(cd, 0); le16(cd, e.method); le16(cd, 0); le16(cd, DOS_DATE);
            le32(cd, e.crc);
            le32(cd, e.comp_size >= 0xffffffffull ? 0xffffffffu : (uint32_t)e.comp_size);
            le32(cd, e.size >= 0xffffffffull ? 0xffffffffu : (uint32_t)e.size);
            le16(cd, (uint16_t)e.name.size()); le16(cd, x.empty() ? 0 : (uint16_t)(x.size() + 4)); le16(cd, 0); le16(cd, 0); le16(cd, 0);
            le32(cd, 0444u << 16);
            le32(cd, e.offset >= 0xffffffffull ? 0xffffffffu : (uint32_t)e.offset);
            cd += e.name;
            if (!x.empty()) { le16(cd, 1); le16(cd, (uint16_t)x.size()); cd += x; }
            if (cd.size() > ((size_t)8 << 20)) { f_.write(cd.data(), cd.size()); cd.clear(); }
        }
        f_.write(cd.data(), cd.size());
        const uint64_t cd_size = f_.pos() - cd_off, n = entries_.size();
        std::string e;
        if (n >= 0xffffull || cd_off >= 0xffffffffull || cd_size >= 0xffffffffull) {
            const uint64_t rec_off = f_.pos();
            le32(e, 0x06064b50u); le64(e, 44); le16(e, 45); le16(e, 45); le32(e, 0); le32(e, 0); le64(e, n); le64(e, n); le64(e, cd_size); le64(e, cd_off);
            le32(e, 0x07064b50u); le32(e, 0); le64(e, rec_off); le32(e, 1);
        }
        le32(e, 0x06054b50u); le16(e, 0); le16(e, 0);
        le16(e, n >= 0xffffull ? 0xffffu : (uint16_t)n); le16(e, n >= 0xffffull ? 0xffffu : (uint16_t)n);
        le32(e, cd_size >= 0xffffffffull ? 0xffffffffu : (uint32_t)cd_size); le32(e, cd_off >= 0xffffffffull ? 0xffffffffu : (uint32_t)cd_off);
        le16(e, 0);
        f_.write(e.data(), e.size());
    }

  private:
    static constexpr uint16_t DOS_DATE = 0x0021;                    // 1980-01-01, time 00:00:00: a set always writes the same bytes
    struct Entry { std::string name; uint64_t offset, comp_size, size; uint32_t crc; uint16_t method; };
    static void le16(std::string& s, uint16_t v) { s += (char)(v & 0xff); s += (char)(v >> 8); }
    static void le32(std::string& s, uint32_t v) { le16(s, (uint16_t)(v & 0xffff)); le16(s, (uint16_t)(v >> 16)); }
    static void le64(std::string& s, uint64_t v) { le32(s, (uint32_t)v); le32(s, (uint32_t)(v >> 32)); }
    SwFile& f_;
    std::vector<Entry> entries_;
};

inline std::string sw_hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; ++i) { s[2 * i] = d[p[i] >> 4]; s[2 * i + 1] = d[p[i] & 15]; }
    return s;
}

// the batches of a source: runs of rows whose text is about SW_BATCH_BYTES at most
inline std::vector<uint64_t> sw_batches(const SwSource& src) {
    uint64_t budget = SW_BATCH_BYTES;
    if (const char* e = getenv("SMG_SIGWRITE_BATCH_BYTES")) { const uint64_t v = strtoull(e, nullptr, 10); if (v) budget = v; }   // (tests: many small batches)
    std::vector<uint64_t> cut{0};
    uint64_t est = 0;
    for (uint64_t r = 0; r < src.n; ++r) {
        const uint64_t row = (src.h_offsets[r + 1] - src.h_offsets[r]) * (SW_MAX_DIGITS + 1) + 512 + src.name(r).size() * 6 + src.filename(r).size() * 6;
        if (est && est + row > budget) { cut.push_back(r); est = 0; }
        est += row;
    }
    cut.push_back(src.n);
    return cut;
}

// ---- the array form (.sig, .sig.gz, to_json) -------------------------------------------------------------------------------------
// The rows of a source as further elements of one JSON array, batch by batch, through `sink`; gz: the gzip member the text goes
// into (null: plain text).  The array's closing bracket is sw_array_close's.
template <class Sink>
inline void sw_array_add(const SwSource& src, SwGzStream* gz, bool& any_rows, Sink sink, hipStream_t st) {
    const std::vector<uint64_t> cut = sw_batches(src);
    for (size_t b = 0; b + 1 < cut.size(); ++b) {
        if (cut[b] == cut[b + 1]) continue;
        SwBatch batch;
        sw_build_batch(src, cut[b], cut[b + 1], false, !any_rows, false, SW_MD5_HOST_BOUND, batch, st);
        any_rows = true;
        std::vector<uint8_t> bytes;
        if (!gz) {
            const auto t0 = swdetail::clk::now();
            bytes.resize(batch.text_bytes);
            HostXfer::get().device_to_host(bytes.data(), batch.text.p, batch.text_bytes, st);
            sigwrite_stats().d2h_ms += swdetail::ms_since(t0);
        } else gz->add(batch.text.as<uint8_t>(), batch.text_bytes, false, bytes, st);
        sink(bytes.data(), bytes.size());
    }
}
// the array's last bytes: "]" alone, or "[]" when nothing was added
template <class Sink>
inline void sw_array_close(SwGzStream* gz, bool any_rows, Sink sink, hipStream_t st) {
    const std::string end = any_rows ? "]" : "[]";
    if (!gz) { sink(end.data(), end.size()); return; }
    AsyncBuf d_end(64, st);
    hip_check(hipMemcpyAsync(d_end.p, end.data(), end.size(), hipMemcpyHostToDevice, st), "H2D");
    std::vector<uint8_t> bytes;
    gz->add(d_end.as<uint8_t>(), end.size(), true, bytes, st);
    sink(bytes.data(), bytes.size());
}

// ---- the writer: open -> add -> add -> close -------------------------------------------------------------------------------------
class SigWriter {
  public:
    enum Kind { SIG, SIG_GZ, ZIP };
    SigWriter(const std::string& path, int compression) : path_(path), compression_(compression < 0 ? 0 : compression), file_(path), zip_(file_) {
        auto ends = [&](const char* suf) { const size_t n = strlen(suf); return path.size() >= n && path.compare(path.size() - n, n, suf) == 0; };
        kind_ = ends(".zip") ? ZIP : ends(".gz") ? SIG_GZ : SIG;     // save_load.py:543-549: anything else is a signature file
        gz_.compression = compression_;
    }

    void add(const SwSource& src, hipStream_t st) {
        if (closed_ || !file_.is_open()) throw err_internal("this output is not open");
        if (src.n && src.ksize == 0) throw err_internal("the set's sketches do not share one set of parameters: it cannot be written");
        try {
            if (kind_ == ZIP) add_zip(src, st); else add_array(src, st);
        } catch (...) { file_.discard(); throw; }
    }

    void close(hipStream_t st) {
        if (closed_) return;
        closed_ = true;
        if (!file_.is_open()) throw err_internal("this output is not open");
        try {
            if (kind_ == ZIP) {
                const std::string csv = manifest_to_csv(manifest_);
                std::string comp(compressBound((uLong)csv.size()) + 64, '\0');
                z_stream zs;
                memset(&zs, 0, sizeof zs);
                if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -MAX_WBITS, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw err_internal("zlib");
                zs.next_in = (Bytef*)csv.data(); zs.avail_in = (uInt)csv.size();
                zs.next_out = (Bytef*)&comp[0]; zs.avail_out = (uInt)comp.size();
                const int rc = deflate(&zs, Z_FINISH);
                const uint64_t nc = zs.total_out;
                deflateEnd(&zs);
                if (rc != Z_STREAM_END) throw err_internal("zlib could not deflate the manifest");
                zip_.add("SOURMASH-MANIFEST.csv", (const uint8_t*)comp.data(), nc, csv.size(), (uint32_t)crc32(0, (const Bytef*)csv.data(), (uInt)csv.size()), 8);
                zip_.finish();
            } else {
                sw_array_close(kind_ == SIG ? nullptr : &gz_, any_rows_, [&](const void* p, size_t n) { file_.write(p, n); }, st);
            }
            file_.commit();
        } catch (...) { file_.discard(); throw; }
    }

  private:
    // .sig / .sig.gz: the rows as elements of one array; its closing bracket is written by close()
    void add_array(const SwSource& src, hipStream_t st) {
        sw_array_add(src, kind_ == SIG ? nullptr : &gz_, any_rows_, [&](const void* p, size_t n) { file_.write(p, n); }, st);
    }

    void add_zip(const SwSource& src, hipStream_t st) {
        using namespace swdetail;
        const std::vector<uint64_t> cut = sw_batches(src);
        const std::string params = std::to_string(src.json_ksize()) + "/" + std::to_string(src.hash_function) + "/" + std::to_string(src.seed) + "/" +
                                   std::to_string(src.max_hash) + "/" + std::to_string(src.num);
        for (size_t b = 0; b + 1 < cut.size(); ++b) {
            const uint64_t r0 = cut[b], n = cut[b + 1] - cut[b];
            if (n == 0) continue;
            SwBatch batch;
            sw_build_batch(src, r0, r0 + n, true, true, true, SW_MD5_HOST_BOUND, batch, st);
            SwPacked packed;
            sw_deflate_docs(batch.text.as<uint8_t>(), batch.doc_off, batch.doc_len, compression_, SW_PACK_CHUNK, packed, st);
            auto t0 = clk::now();
            const std::vector<uint32_t> member_crc = crc_docs(packed.out.as<uint8_t>(), packed.off, packed.len, st);   // the zip entry's: over the member bytes
            sigwrite_stats().crc_ms += ms_since(t0);
            t0 = clk::now();
            std::vector<uint8_t> bytes(packed.out_bytes);
            HostXfer::get().device_to_host(bytes.data(), packed.out.p, packed.out_bytes, st);
            sigwrite_stats().d2h_ms += ms_since(t0);
            for (uint64_t i = 0; i < n; ++i) {
                const std::string md5 = sw_hex(&batch.md5[16 * i], 16);
                const std::string name = src.name(r0 + i), filename = src.filename(r0 + i);
                // same md5, same name, file name and parameters: the same document, written once; otherwise the next free suffix
                const std::string ident = name + '\0' + filename + '\0' + params;
                std::unordered_map<std::string, std::string>& seen = members_[md5];      // document -> member, for this md5
                std::string& member = seen[ident];
                if (member.empty()) {
                    member = "signatures/" + md5 + ".sig.gz";
                    if (seen.size() > 1) member += "_" + std::to_string(seen.size() - 2);
                    zip_.add(member, bytes.data() + packed.off[i], packed.len[i], packed.len[i], member_crc[i], 0);
                }
                ManifestRow m;
                m.internal_location = member; m.md5 = md5; m.name = name; m.filename = filename;
                m.moltype = molecule_name(src.hash_function); m.ksize = src.ksize; m.num = src.num;
                m.scaled = src.max_hash ? scaled_for_max_hash(src.max_hash) : 0;
                m.n_hashes = src.h_offsets[r0 + i + 1] - src.h_offsets[r0 + i];
                manifest_.push_back(std::move(m));
            }
        }
    }

    std::string path_;
    int compression_;
    Kind kind_ = SIG;
    SwFile file_;
    SwZip zip_;
    SwGzStream gz_;
    bool any_rows_ = false, closed_ = false;
    std::vector<ManifestRow> manifest_;
    std::unordered_map<std::string, std::unordered_map<std::string, std::string>> members_;
};

}  // namespace smg
