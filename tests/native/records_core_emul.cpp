// Host build of the two rules of per-record sketching (sourmash_amd/csrc/records_core.hpp: the record a k-mer belongs to, and
// whether record number and hash share one sort key) -- a test-only artefact.  tests/test_records_cpu.py compares them with
// Python's arithmetic.
#include <stdint.h>
#include "../../sourmash_amd/csrc/records_core.hpp"

// out[i] = record of the k-mer starting at pos[i], or -1 when the rule drops it
extern "C" void emul_rec_assign(const uint64_t* starts, uint64_t n_records, const uint64_t* pos, uint64_t n, uint32_t k, int64_t* out) {
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t r = 0;
        out[i] = smg::rec_assign(starts, n_records, pos[i], k, &r) ? (int64_t)r : -1;
    }
}

extern "C" int emul_rec_packed(uint64_t n_records, uint64_t max_hash) { return smg::rec_packed(n_records, max_hash) ? 1 : 0; }
extern "C" int emul_rec_hash_bits(uint64_t max_hash) { return smg::rec_hash_bits(max_hash); }
