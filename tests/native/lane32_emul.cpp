// Host emulation of the appending sketch kernel's walk with 32 start positions per lane (test-only artefact).
// Compiles sourmash_amd/csrc/kmer_core.hpp for the CPU and walks a buffer the way sketch_dna_kernel<K, 16, false> does where
// sk_lane_positions(K, false) is 32: a window is 256 lanes x 32 positions, a tile `rounds` (1 .. 2) of them staged by the
// kernel's own stage_tile into copies sized for two rounds, every lane reads its window of P + K - 1 bytes with read_window at
// lane index tid + r * 256 and hashes it with process_lane_staged<K, 32, EARLY, PLAIN, LATE = true> -- the last key dword masked
// behind the strand select, as the kernel asks for it.  tests/test_lane32_cpu.py compares the result with the oracle.
// The second entry checks the hash the lanes call, alone: mmh3_open_words<K> and mmh3_h1_words<K> on zero-padded key dwords
// against mmh3_h1_bytes for every K = 1 .. 88, every tail shape.
#include <cstring>
#include <utility>
#include <vector>
#include "../../sourmash_amd/csrc/kmer_core.hpp"

constexpr int BLOCK = 256, P = 32, R_MAX = 2;

template <int K>
static uint64_t run(const uint8_t* seq, uint64_t len, uint32_t skip, uint32_t rounds, uint64_t seed, uint64_t thr, uint64_t* out,
                    uint64_t cap, uint64_t* dirty_tiles) {
    using T = smg::TileGeom<K, P, BLOCK, R_MAX>;
    static_assert(T::WINDOW == 8192 && T::LANE_RD % 4 == 0 && smg::LaneGeom<K, P>::NBYTES <= 192, "the geometry the kernel walks");
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
                smg::process_lane_staged<K, P, true, false, true>(U, C, s_dirty != 0, seed, thr,
                                                                  [&](int, uint64_t h) { if (n < cap) out[n] = h; ++n; });
            }
        }
    }
    return n;
}

// k = 19, 21, 31, 32, 33, 47, 48, 51, 64, 88 and rounds = 1, 2; ~0 for anything else
extern "C" uint64_t emul_lane32_sketch(const uint8_t* seq, uint64_t len, uint32_t k, uint32_t skip, uint32_t rounds, uint64_t seed,
                                       uint64_t thr, uint64_t* out, uint64_t cap, uint64_t* dirty_tiles) {
    if (skip >= 16 || rounds < 1 || rounds > (uint32_t)R_MAX) return ~0ull;
    switch (k) {
    case 19: return run<19>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 21: return run<21>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 31: return run<31>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 32: return run<32>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 33: return run<33>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 47: return run<47>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 48: return run<48>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 51: return run<51>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 64: return run<64>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    case 88: return run<88>(seq, len, skip, rounds, seed, thr, out, cap, dirty_tiles);
    default: return ~0ull;
    }
}

// ---- murmur3.hpp: the words form of the hash against the bytes form ---------------------------------------------------------------
static uint64_t next_random(uint64_t& s) {               // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

template <int K>
static uint64_t words_mismatches(uint64_t keys, uint64_t& rng) {
    constexpr int NW = (K + 3) / 4;
    uint64_t bad = 0;
    for (uint64_t i = 0; i < keys; ++i) {
        uint8_t key[4 * NW];
        for (int b = 0; b < 4 * NW; ++b) key[b] = b < K ? (uint8_t)next_random(rng) : 0;       // zero padded
        if (i == 0) std::memset(key, 0, K);
        if (i == 1) std::memset(key, 0xff, K);
        uint32_t w[NW];
        for (int d = 0; d < NW; ++d)
            w[d] = (uint32_t)key[4 * d] | ((uint32_t)key[4 * d + 1] << 8) | ((uint32_t)key[4 * d + 2] << 16) | ((uint32_t)key[4 * d + 3] << 24);
        const uint64_t seed = i % 3 == 0 ? 42 : i % 3 == 1 ? 0 : next_random(rng);
        const uint64_t want = smg::mmh3_h1_bytes(key, K, seed);
        bad += smg::mmh3_h1_words<K>(w, seed) != want;
        bad += smg::mmh3_h1_words<K, true>(w, seed) != want;                                   // the plain multiplies
        const smg::Mmh3Open o = smg::mmh3_open_words<K>(w, seed);
        bad += smg::mmh3_close(o) != want;
    }
    return bad;
}
template <int... KS>
static uint64_t all_words_mismatches(uint64_t keys, uint64_t& rng, std::integer_sequence<int, KS...>) {
    return (words_mismatches<KS + 1>(keys, rng) + ...);
}

// mismatches (0 is a pass) of mmh3_open_words<K> / mmh3_h1_words<K> against mmh3_h1_bytes on `keys` keys for every K = 1 .. 88
extern "C" uint64_t emul_lane32_murmur(uint64_t keys) {
    uint64_t rng = 0x1234;
    return all_words_mismatches(keys, rng, std::make_integer_sequence<int, 88>{});
}
