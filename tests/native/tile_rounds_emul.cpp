// Host emulation of the appending sketch kernel's walk over tiles of several window rounds (test-only artefact).
// Compiles sourmash_amd/csrc/kmer_core.hpp for the CPU and walks a buffer the way sketch_dna_kernel<K, 16, false> does when its
// tile is `rounds` consecutive windows of 256 x 16 positions: the LDS copies sized for R_MAX rounds, the chunks of the tile
// actually walked staged by the kernel's own stage_tile (alignment prefix blanked, zero fill past the end, one dirty flag per
// tile), then for every round r the lanes read their windows at lane index tid + r * 256 (read_window) into
// process_lane_staged.  tests/test_tile_rounds_cpu.py compares the result with the oracle, and the launcher's rule for `rounds`
// (sk_tile_rounds) with the values it must give.
#include <cstring>
#include <vector>
#include "../../sourmash_amd/csrc/kmer_core.hpp"

constexpr int BLOCK = 256, P = 16, R_MAX = 3;

template <int K>
static uint64_t run(const uint8_t* seq, uint64_t len, uint32_t skip, uint32_t rounds, uint64_t seed, uint64_t thr, uint64_t* out,
                    uint64_t cap, uint64_t* dirty_tiles) {
    using T = smg::TileGeom<K, P, BLOCK, R_MAX>;
    // what the launcher does: back to the 16-byte boundary, the prefix counted in, tiles of the length this launch walks
    std::vector<uint8_t> buf(skip + len + 1, (uint8_t)'A');       // the prefix holds valid-looking bytes: blanking must kill them
    if (len) std::memcpy(buf.data() + skip, seq, len);
    const uint64_t total = len + skip, tile_len = (uint64_t)rounds * T::WINDOW;
    const uint64_t n_tiles = (total + tile_len - 1) / tile_len;
    // the copies are poisoned with valid bases in front of every tile: a round must never read what its tile did not stage
    std::vector<uint32_t> s_in(T::IN_CHUNKS * 4), s_comp(T::IN_CHUNKS * 4);
    uint64_t n = 0;
    *dirty_tiles = 0;
    for (uint64_t tile = 0; tile < n_tiles; ++tile) {
        const uint64_t base = tile * tile_len;
        std::fill(s_in.begin(), s_in.end(), 0x41414141u);
        std::fill(s_comp.begin(), s_comp.end(), 0x54545454u);
        unsigned s_dirty = 0;
        smg::stage_tile<T::IN_CHUNKS, true, BLOCK>(buf.data(), base, total, skip, s_in.data(), s_comp.data(), &s_dirty,
                                                   T::chunks((int)rounds));
        *dirty_tiles += s_dirty;
        for (uint32_t r = 0; r < rounds; ++r) {
            for (int tid = 0; tid < BLOCK; ++tid) {
                uint32_t U[T::LANE_RD], C[T::LANE_RD];
                smg::read_window<T::LANE_RD, P>(s_in.data(), tid + (int)r * BLOCK, U);
                smg::read_window<T::LANE_RD, P>(s_comp.data(), tid + (int)r * BLOCK, C);
                smg::process_lane_staged<K, P>(U, C, s_dirty != 0, seed, thr, [&](int, uint64_t h) { if (n < cap) out[n] = h; ++n; });
            }
        }
    }
    return n;
}

// k = 12, 21, 31, 51, 88 and rounds = 1 .. 3; ~0 for anything else
extern "C" uint64_t emul_tile_rounds_sketch(const uint8_t* seq, uint64_t len, uint32_t k, uint32_t skip, uint32_t rounds, uint64_t seed,
                                            uint64_t thr, uint64_t* out, uint64_t cap, uint64_t* dirty_tiles) {
    if (skip >= 16 || rounds < 1 || rounds > (uint32_t)R_MAX) return ~0ull;
    switch (k) {
    case 12: return run<12>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 21: return run<21>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 31: return run<31>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 51: return run<51>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 88: return run<88>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    default: return ~0ull;
    }
}

// the launcher's rule (sketch_kernel.hpp, SketchLaunch::launch): rounds of a launch with threshold thr whose kernel holds r_max
// rounds in LDS and `cap` sink entries; a round is 256 x 16 positions
extern "C" uint32_t emul_tile_rounds_rule(uint64_t thr, uint32_t r_max, uint32_t cap) {
    return smg::sk_tile_rounds(thr, r_max, (uint32_t)BLOCK * P, cap);
}
