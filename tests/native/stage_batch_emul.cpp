// Host emulation of the appending sketch kernel's batched tile staging (test-only artefact; a stand-alone program).
// Compiles sourmash_amd/csrc/kmer_core.hpp for the CPU and walks a buffer the way sketch_dna_kernel<K, 16, false> does with the
// lane geometry the kernel's rules give that ksize.  Every tile is staged twice into poisoned copies: by the loop of stage_tile
// (one chunk after the other, zero fill, prefix blanking), and the way the kernel does it -- where stage_batch_ok says the tile
// has all the chunks the copies were sized for and lies wholly inside the buffer, lane by lane through stage_lane_batched (all
// loads of a lane first, then the per-byte work and the stores in load order), on the loop otherwise.  s_in, s_comp and the
// flag must agree word for word, the words no chunk of the tile covers included.  The lanes then read their windows
// (read_window at lane index tid + r * 256) into process_lane_staged, and the kept hashes go to a file that
// tests/test_stage_batch_cpu.py compares with the oracle.
//
//   stage_batch_emul K ROUNDS SKIP THR IN OUT   ->   "tiles T batched B dirty D", hashes (u64) in OUT; exit 1 on a mismatch
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../sourmash_amd/csrc/kmer_core.hpp"

constexpr int BLOCK = 256;

template <int K, int P, int R_MAX>
static int run(const std::vector<uint8_t>& seq, uint32_t skip, uint32_t rounds, uint64_t thr, std::vector<uint64_t>& out) {
    using T = smg::TileGeom<K, P, BLOCK, R_MAX>;
    constexpr bool PLAIN = K == 50 || K == 51, LATE = true;      // what sketch_kernel.hpp asks of process_lane_staged at these k
    if (rounds > (uint32_t)R_MAX) { fprintf(stderr, "rounds above %d\n", R_MAX); return 2; }
    // what the launcher does: back to the 16-byte boundary, the prefix counted in, tiles of the length this launch walks.  The
    // buffer ends with its last byte (a vector of exactly that size), so that a read past `total` is one past the allocation.
    const uint64_t len = seq.size(), total = len + skip, tile_len = (uint64_t)rounds * T::WINDOW;
    std::vector<uint8_t> buf(total);
    std::memset(buf.data(), 'A', skip);                          // the prefix holds valid-looking bytes: blanking must kill them
    if (len) std::memcpy(buf.data() + skip, seq.data(), len);
    const uint64_t n_tiles = (total + tile_len - 1) / tile_len;
    const int n_chunks = T::chunks((int)rounds);
    std::vector<uint32_t> a_in(T::IN_CHUNKS * 4), a_comp(T::IN_CHUNKS * 4), b_in(T::IN_CHUNKS * 4), b_comp(T::IN_CHUNKS * 4);
    uint64_t batched = 0, dirty_tiles = 0;
    for (uint64_t tile = 0; tile < n_tiles; ++tile) {
        const uint64_t base = tile * tile_len;
        // poisoned with valid bases: a round must never read what its tile did not stage, and neither form may write behind it
        std::fill(a_in.begin(), a_in.end(), 0x41414141u);
        std::fill(a_comp.begin(), a_comp.end(), 0x54545454u);
        b_in = a_in;
        b_comp = a_comp;
        unsigned a_dirty = 0, b_dirty = 0;                        // lane 0 clears the flag in front of every tile
        smg::stage_tile<T::IN_CHUNKS, true, BLOCK>(buf.data(), base, total, skip, a_in.data(), a_comp.data(), &a_dirty, n_chunks);
        if (smg::stage_batch_ok(base, total, skip, n_chunks, T::IN_CHUNKS)) {
            ++batched;
            for (int lane = 0; lane < BLOCK; ++lane)
                smg::stage_lane_batched<T::IN_CHUNKS, BLOCK>(buf.data(), base, lane, b_in.data(), b_comp.data(), &b_dirty);
        } else {
            smg::stage_tile<T::IN_CHUNKS, true, BLOCK>(buf.data(), base, total, skip, b_in.data(), b_comp.data(), &b_dirty, n_chunks);
        }
        if (a_in != b_in || a_comp != b_comp || a_dirty != b_dirty) {
            fprintf(stderr, "tile %" PRIu64 ": the two stagings differ (s_in %d, s_comp %d, flag %u / %u)\n", tile, (int)(a_in != b_in),
                    (int)(a_comp != b_comp), a_dirty, b_dirty);
            return 1;
        }
        const bool dirty = b_dirty != 0;
        dirty_tiles += dirty;
        for (uint32_t r = 0; r < rounds; ++r) {
            for (int tid = 0; tid < BLOCK; ++tid) {
                uint32_t U[T::LANE_RD], C[T::LANE_RD];
                smg::read_window<T::LANE_RD, P>(b_in.data(), tid + (int)r * BLOCK, U);
                smg::read_window<T::LANE_RD, P>(b_comp.data(), tid + (int)r * BLOCK, C);
                smg::process_lane_staged<K, P, true, PLAIN, LATE>(U, C, dirty, 42, thr, [&](int, uint64_t h) { out.push_back(h); });
            }
        }
    }
    printf("tiles %" PRIu64 " batched %" PRIu64 " dirty %" PRIu64 "\n", n_tiles, batched, dirty_tiles);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: %s K ROUNDS SKIP THR IN OUT\n", argv[0]); return 2; }
    const int k = atoi(argv[1]);
    const uint32_t rounds = (uint32_t)atoi(argv[2]), skip = (uint32_t)atoi(argv[3]);
    const uint64_t thr = strtoull(argv[4], nullptr, 10);
    if (skip >= 16 || rounds < 1) return 2;
    std::vector<uint8_t> seq;
    if (FILE* f = fopen(argv[5], "rb")) {
        uint8_t tmp[65536];
        for (size_t n; (n = fread(tmp, 1, sizeof tmp, f)) > 0;) seq.insert(seq.end(), tmp, tmp + n);
        fclose(f);
    } else {
        return 2;
    }
    std::vector<uint64_t> out;
    int rc;
    // lane positions and rounds as sk_lane_positions / sk_rounds_max of sketch_kernel.hpp give them: 32 x 2, at k = 37 16 x 3
    switch (k) {
    case 19: rc = run<19, 32, 2>(seq, skip, rounds, thr, out); break;
    case 31: rc = run<31, 32, 2>(seq, skip, rounds, thr, out); break;
    case 37: rc = run<37, 16, 3>(seq, skip, rounds, thr, out); break;
    case 51: rc = run<51, 32, 2>(seq, skip, rounds, thr, out); break;
    case 88: rc = run<88, 32, 2>(seq, skip, rounds, thr, out); break;
    default: fprintf(stderr, "ksize not instantiated\n"); return 2;
    }
    if (rc) return rc;
    FILE* f = fopen(argv[6], "wb");
    if (!f) return 2;
    if (!out.empty() && fwrite(out.data(), 8, out.size(), f) != out.size()) { fclose(f); return 2; }
    fclose(f);
    return 0;
}
