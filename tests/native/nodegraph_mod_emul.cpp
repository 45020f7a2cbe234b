// Host build of the Nodegraph kernels' reduction h mod d (sourmash_amd/csrc/nodegraph_core.hpp: mulhi quotient estimate by a
// precomputed reciprocal, two corrections) and base codes (test-only artefact).  tests/test_nodegraph_cpu.py compares them with
// Python's arithmetic.
#include <stdint.h>
#include "../../sourmash_amd/csrc/nodegraph_core.hpp"

extern "C" void emul_ng_mod(const uint64_t* h, uint64_t n, uint64_t d, uint64_t* out) {
    const uint64_t m = smg::ng_magic(d);
    for (uint64_t i = 0; i < n; ++i) out[i] = smg::ng_mod(h[i], d, m);
}

// code of every byte value, or 255 for a byte the bulk paths do not take
extern "C" void emul_ng_codes(uint8_t* out) {
    for (uint32_t c = 0; c < 256; ++c) {
        bool ok;
        const uint32_t code = smg::ng_code(c, &ok);
        out[c] = ok ? (uint8_t)code : 255;
    }
}
