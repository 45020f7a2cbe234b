// Host emulation of the appending sketch kernel with the per-byte work done at staging (test-only artefact).
// Compiles sourmash_amd/csrc/kmer_core.hpp for the CPU and walks a buffer tile by tile exactly as sketch_dna_kernel<K, 16, false>
// does: the alignment prefix (`skip` bytes in front of the caller's buffer, blanked), 16-byte chunks staged by the kernel's own
// stage_tile into an upper-cased and a complemented copy of the tile, zero fill past the end, the tile's dirty flag, and lanes
// that read their windows from the two copies (read_window) into process_lane_staged.  tests/test_strand_lds_cpu.py compares
// the result with the oracle.
#include <cstring>
#include <utility>
#include <vector>
#include "../../sourmash_amd/csrc/kmer_core.hpp"

constexpr int BLOCK = 256, P = 16;

template <int K>
static uint64_t run(const uint8_t* seq, uint64_t len, uint32_t skip, uint64_t seed, uint64_t thr, uint64_t* out, uint64_t cap,
                    uint64_t* dirty_tiles) {
    using T = smg::TileGeom<K, P, BLOCK>;
    // what the launcher does: back to the 16-byte boundary, the prefix counted in
    std::vector<uint8_t> buf(skip + len + 1, (uint8_t)'A');       // the prefix holds valid-looking bytes: blanking must kill them
    if (len) std::memcpy(buf.data() + skip, seq, len);
    const uint8_t* base_ptr = buf.data();
    const uint64_t total = len + skip;
    const uint64_t n_tiles = (total + T::TILE - 1) / T::TILE;
    std::vector<uint32_t> s_in(T::IN_CHUNKS * 4), s_comp(T::IN_CHUNKS * 4);
    uint64_t n = 0;
    *dirty_tiles = 0;
    for (uint64_t tile = 0; tile < n_tiles; ++tile) {
        const uint64_t base = tile * (uint64_t)T::TILE;
        unsigned s_dirty = 0;
        smg::stage_tile<T::IN_CHUNKS, true, BLOCK>(base_ptr, base, total, skip, s_in.data(), s_comp.data(), &s_dirty);
        *dirty_tiles += s_dirty;
        for (int tid = 0; tid < BLOCK; ++tid) {
            uint32_t U[T::LANE_RD], C[T::LANE_RD];
            smg::read_window<T::LANE_RD, P>(s_in.data(), tid, U);
            smg::read_window<T::LANE_RD, P>(s_comp.data(), tid, C);
            smg::process_lane_staged<K, P>(U, C, s_dirty != 0, seed, thr, [&](int, uint64_t h) { if (n < cap) out[n] = h; ++n; });
        }
    }
    return n;
}

typedef uint64_t (*run_fn)(const uint8_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint64_t*, uint64_t, uint64_t*);
template <int... KS>
static run_fn pick(uint32_t k, std::integer_sequence<int, KS...>) {
    static const run_fn table[] = {&run<KS + 1>...};
    return k >= 1 && k <= sizeof...(KS) ? table[k - 1] : nullptr;
}

// every ksize of the register-window kernel (k = 1 .. 88); ~0 for any other
extern "C" uint64_t emul_strand_sketch(const uint8_t* seq, uint64_t len, uint32_t k, uint32_t skip, uint64_t seed, uint64_t thr,
                                       uint64_t* out, uint64_t cap, uint64_t* dirty_tiles) {
    const run_fn f = skip < 16 ? pick(k, std::make_integer_sequence<int, 88>()) : nullptr;
    return f ? f(seq, len, skip, seed, thr, out, cap, dirty_tiles) : ~0ull;
}
