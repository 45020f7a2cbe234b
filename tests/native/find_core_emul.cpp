// Host build of the membership rule of k-mer finding (sourmash_amd/csrc/find_core.hpp: the bucket directory over a query's sorted
// hashes and the lookup in it) -- a test-only artefact.  tests/test_find_core_cpu.py compares it with numpy.isin.
#include <stdint.h>
#include "../../sourmash_amd/csrc/find_core.hpp"

extern "C" uint32_t emul_find_dir_shift(uint64_t n, uint64_t max_hash) { return smg::find_dir_shift(n, max_hash); }
extern "C" uint64_t emul_find_dir_buckets(uint64_t max_hash, uint32_t shift) { return smg::find_dir_buckets(max_hash, shift); }
extern "C" uint64_t emul_find_max_buckets() { return smg::FIND_MAX_BUCKETS; }

// dir[0 .. nb] as the device builds it: one entry per bucket boundary
extern "C" void emul_find_dir(const uint64_t* q, uint64_t n, uint32_t shift, uint64_t nb, uint32_t* dir) {
    for (uint64_t b = 0; b <= nb; ++b) dir[b] = smg::find_dir_entry(q, n, shift, b);
}

// out[i] = probes[i] is a member; returns the number of probes whose lookup would have read outside dir[0 .. nb] (always 0:
// find_member is called only when the bucket is inside, which the count proves for the caller)
extern "C" uint64_t emul_find_member(const uint64_t* q, const uint32_t* dir, uint32_t shift, uint64_t nb, uint64_t max_hash,
                                     const uint64_t* probes, uint64_t n_probes, uint8_t* out) {
    uint64_t outside = 0;
    for (uint64_t i = 0; i < n_probes; ++i) {
        const uint64_t h = probes[i];
        if (h - 1 < max_hash && (h >> shift) + 1 > nb) ++outside;      // a looked-up hash reads dir[b] and dir[b + 1]
        out[i] = smg::find_member(q, dir, shift, max_hash, h) ? 1 : 0;
    }
    return outside;
}
