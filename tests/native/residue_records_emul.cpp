// Host build of the rules of per-record residue sketching (sourmash_amd/csrc/records_core.hpp: records with explicit ends;
// translate_records_core.hpp: every record's six-frame translation in a block of its own) -- a test-only artefact.
// tests/test_residue_records_cpu.py compares them with numpy and with the oracle's codon table.
#include <cstring>
#include <vector>
#include "../../sourmash_amd/csrc/records_core.hpp"
#include "../../sourmash_amd/csrc/translate_records_core.hpp"

// out[i] = record of the window of k bytes starting at pos[i], or -1 when the rule drops it; ends may be null
extern "C" void emul_rec_assign_ends(const uint64_t* starts, const uint64_t* ends, uint64_t n_records, const uint64_t* pos, uint64_t n, uint32_t k,
                                     int64_t* out) {
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t r = 0;
        out[i] = smg::rec_assign_ends(starts, ends, n_records, pos[i], k, &r) ? (int64_t)r : -1;
    }
}

extern "C" int emul_rec_ends_valid(const uint64_t* starts, const uint64_t* ends, uint64_t r) { return smg::rec_ends_valid(starts, ends, r) ? 1 : 0; }

// block_starts[0 .. n_records]: the exclusive prefix sum of the records' block sizes -> the size of the residue buffer
extern "C" uint64_t emul_block_starts(const uint64_t* starts, const uint64_t* ends, uint64_t n_records, uint64_t* block_starts) {
    uint64_t at = 0;
    for (uint64_t r = 0; r < n_records; ++r) {
        block_starts[r] = at;
        at += smg::translated_block_bytes(smg::rec_len(starts, ends, r));
    }
    block_starts[n_records] = at;
    return at;
}

extern "C" uint64_t emul_translated_records_bound(uint64_t len, uint64_t n_records) { return smg::translated_records_bound(len, n_records); }

// the residue buffer as the kernel writes it, word by word (out: room for whole 8-byte words), and the block of every byte
extern "C" void emul_translate_records(const uint8_t* seq, const uint64_t* starts, const uint64_t* ends, const uint64_t* block_starts,
                                       uint64_t n_records, uint32_t hf, uint8_t* out, uint64_t* block_of) {
    uint8_t code_f[256], code_r[256], codon[216];
    for (int t = 0; t < 256; ++t) {
        const uint8_t c = smg::ascii_upper((uint8_t)t);
        code_f[t] = (uint8_t)smg::nt_code(c);
        code_r[t] = (uint8_t)smg::nt_code(smg::dna_complement_or_nul(c));
    }
    const char* letters = "ACGTN?";
    for (int t = 0; t < 216; ++t)
        codon[t] = smg::residue_encode(smg::translate_codon((uint8_t)letters[t / 36], (uint8_t)letters[(t / 6) % 6], (uint8_t)letters[t % 6]), hf);
    const smg::TranslateTables T{code_f, code_r, codon};
    const uint64_t total = block_starts[n_records];
    for (uint64_t G = 0; G < (total + 7) / 8; ++G) {
        const uint64_t w = smg::translate_records_word(seq, starts, ends, block_starts, n_records, T, G);
        std::memcpy(out + 8 * G, &w, 8);
    }
    for (uint64_t o = 0; o < total; ++o) block_of[o] = smg::translate_block_of(block_starts, n_records, o);
}
