// Host emulation of sigwrite.hip: the functions of sourmash_amd/csrc/sigwrite_core.hpp walked with lanes as loop indices.
//
//   sw_emul_decimal   a number's digit count and digits
//   sw_emul_md5       sw_md5_kernel: waves of 64 lanes, a row per lane, the 64 rings interleaved word by word as in LDS
//   sw_emul_table / sw_emul_header   the code words and the block header the host builds
//   sw_emul_deflate   sw_pack_kernel + sw_frame_kernel for one document: the raw deflate stream (block header, the chunks' codes
//                     ORed into zeroed words -- whole words inside a chunk, OR at both ends --, end-of-block)
// Built as a shared library for tests/test_sigwrite_core_cpu.py, and with -DSW_EMUL_MAIN as a stand-alone program that reads
// cases from a file and prints results as hex lines (run under AddressSanitizer / UndefinedBehaviorSanitizer).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../sourmash_amd/csrc/sigwrite_core.hpp"

using namespace smg;

extern "C" {

uint32_t sw_emul_decimal(uint64_t v, uint8_t* out) {
    const uint32_t nd = sw_digit_count(v);
    sw_put_decimal(v, nd, [&](uint32_t j, uint8_t b) { out[j] = b; });
    return nd;
}

void sw_emul_md5(uint32_t ksize, const uint64_t* hashes, const uint64_t* offsets, uint32_t n_rows, uint8_t* out) {
    std::vector<uint32_t> lds(32 * 64);
    for (uint32_t wave = 0; wave * 64 < n_rows; ++wave)
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t r = wave * 64 + lane;
            if (r >= n_rows) continue;
            const SwRing ring{lds.data() + lane, 64};
            sw_md5_row(ring, ksize, hashes + offsets[r], offsets[r + 1] - offsets[r], out + 16 * (size_t)r);
        }
}

void sw_emul_table(uint32_t* table) { sw_build_table(table); }

uint32_t sw_emul_header(uint8_t* bytes, uint32_t cap) {
    std::vector<uint8_t> h;
    const uint32_t nbits = sw_build_block_header(h);
    if (h.size() > cap) return 0;
    memcpy(bytes, h.data(), h.size());
    return nbits;
}

// -> bytes of the stream written at out (out_words 32-bit words, zeroed here), 0 if it does not fit
uint64_t sw_emul_deflate(const uint8_t* text, uint64_t len, uint32_t chunk, uint32_t n_lanes, uint32_t* out, uint64_t out_words) {
    if (chunk == 0 || chunk > SW_MAX_CHUNK || n_lanes == 0) return 0;
    uint32_t table[SW_SYMBOLS];
    sw_build_table(table);
    std::vector<uint8_t> hdr;
    const uint32_t hdr_bits = sw_build_block_header(hdr);
    // the chunks and their first bits (the host's part: a sum per chunk, a running sum per member)
    std::vector<SwChunk> chunks;
    uint64_t bit = hdr_bits;
    for (uint64_t off = 0; off < len || chunks.empty(); off += chunk) {
        SwChunk c;
        c.in_off = off; c.in_len = (uint32_t)(len - off < chunk ? len - off : chunk);
        c.flags = off + chunk >= len ? SW_CHUNK_LAST : 0u;
        c.out_bit = bit;
        for (uint32_t l = 0; l < n_lanes; ++l)
            bit += sw_lane_bits(text + off, sw_lane_lo(c.in_len, l, n_lanes), sw_lane_hi(c.in_len, l, n_lanes), table, (c.flags & SW_CHUNK_LAST) && l == n_lanes - 1);
        chunks.push_back(c);
    }
    const uint64_t total_bytes = (bit + 7) / 8;
    if ((total_bytes + 3) / 4 > out_words) return 0;
    memset(out, 0, (size_t)((total_bytes + 3) / 4) * 4);
    // the pack kernel: a block per chunk
    std::vector<uint32_t> words(SW_CHUNK_WORDS), lane_bits(n_lanes);
    for (const SwChunk& c : chunks) {
        const uint8_t* t = text + c.in_off;
        uint32_t sum = 0;
        for (uint32_t l = 0; l < n_lanes; ++l) {
            lane_bits[l] = sw_lane_bits(t, sw_lane_lo(c.in_len, l, n_lanes), sw_lane_hi(c.in_len, l, n_lanes), table, (c.flags & SW_CHUNK_LAST) && l == n_lanes - 1);
            sum += lane_bits[l];
        }
        const uint32_t nw = sw_chunk_words(c.out_bit, sum);
        if (nw > SW_CHUNK_WORDS) return 0;
        std::fill(words.begin(), words.end(), 0u);
        uint32_t at = (uint32_t)(c.out_bit & 31u);
        for (uint32_t l = 0; l < n_lanes; ++l) {
            sw_lane_pack(t, sw_lane_lo(c.in_len, l, n_lanes), sw_lane_hi(c.in_len, l, n_lanes), table, (c.flags & SW_CHUNK_LAST) && l == n_lanes - 1, at,
                         [&](uint32_t w, uint32_t v) { words.at(w) |= v; });
            at += lane_bits[l];
        }
        const uint64_t w0 = c.out_bit >> 5;
        for (uint32_t w = 0; w < nw; ++w) {
            if (w0 + w >= out_words) return 0;
            if (w == 0 || w == nw - 1) out[w0 + w] |= words[w];
            else out[w0 + w] = words[w];
        }
    }
    // the frame kernel: the block header, whole bytes stored, its last partial byte ORed in
    uint8_t* ob = reinterpret_cast<uint8_t*>(out);
    for (uint32_t i = 0; i < hdr.size(); ++i) {
        if (i * 8 + 8 <= hdr_bits) ob[i] = hdr[i];
        else ob[i] |= hdr[i];
    }
    return total_bytes;
}

}  // extern "C"

#ifdef SW_EMUL_MAIN
static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}

// case file, a case per line:  "dec V" | "md5 KSIZE H0 H1 ..." | "deflate CHUNK LANES HEXBYTES" (HEXBYTES may be "-": no bytes)
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::string line;
    int ch;
    std::vector<std::string> lines;
    while ((ch = fgetc(f)) != EOF) {
        if (ch == '\n') { lines.push_back(line); line.clear(); } else line += (char)ch;
    }
    if (!line.empty()) lines.push_back(line);
    fclose(f);
    for (const std::string& l : lines) {
        std::vector<std::string> tok;
        size_t at = 0;
        while (at < l.size()) {
            const size_t sp = l.find(' ', at);
            tok.push_back(l.substr(at, sp == std::string::npos ? std::string::npos : sp - at));
            if (sp == std::string::npos) break;
            at = sp + 1;
        }
        if (tok.empty()) continue;
        if (tok[0] == "dec" && tok.size() == 2) {
            uint8_t d[SW_MAX_DIGITS];
            const uint32_t nd = sw_emul_decimal(strtoull(tok[1].c_str(), nullptr, 10), d);
            printf("%s\n", std::string((const char*)d, nd).c_str());
        } else if (tok[0] == "md5" && tok.size() >= 2) {
            std::vector<uint64_t> h;
            for (size_t i = 2; i < tok.size(); ++i) h.push_back(strtoull(tok[i].c_str(), nullptr, 10));
            const uint64_t off[2] = {0, h.size()};
            uint8_t out[16];
            sw_emul_md5((uint32_t)strtoul(tok[1].c_str(), nullptr, 10), h.data(), off, 1, out);
            printf("%s\n", hex(out, 16).c_str());
        } else if (tok[0] == "deflate" && tok.size() == 4) {
            std::vector<uint8_t> text;
            text.reserve(16);                                        // (data() of an empty vector may be null)
            if (tok[3] != "-")
                for (size_t i = 0; i + 1 < tok[3].size(); i += 2) text.push_back((uint8_t)strtoul(tok[3].substr(i, 2).c_str(), nullptr, 16));
            const uint64_t words = (text.size() * 15 + 2048) / 32 + 8;
            std::vector<uint32_t> out(words);
            const uint64_t n = sw_emul_deflate(text.data(), text.size(), (uint32_t)strtoul(tok[1].c_str(), nullptr, 10),
                                               (uint32_t)strtoul(tok[2].c_str(), nullptr, 10), out.data(), words);
            printf("%s\n", n ? hex(reinterpret_cast<const uint8_t*>(out.data()), n).c_str() : "FAILED");
        } else {
            fprintf(stderr, "bad case: %s\n", l.c_str());
            return 2;
        }
    }
    return 0;
}
#endif
