// Host emulation of the appending sketch kernel's tile hand-out (test-only artefact; a program of its own, so that it also runs
// under the sanitizers).  Compiles sourmash_amd/csrc/kmer_core.hpp for the CPU and walks tiles the way the workgroups of
// sketch_dna_kernel<K, 16, false> do when a launch has a ticket counter: a workgroup's first tile is its own index, every later
// one comes from the kernel's own rule (tile_first, tile_from_ticket, tile_end) with a ticket taken in front of the hashing of the
// current tile.  G "workgroups" each keep what a workgroup keeps between its tiles -- the two LDS copies, the dirty flag, the next
// tile -- and a scheduler decides which of them runs its next tile: the order in which tickets are granted.
//
//   tile_handout_emul index
//       the index rule alone, for G in {1, 3, 8} and n_tiles in {0, 1, G - 1, G, G + 1, 5 G + 3}, three orders: every tile once,
//       none behind the end, the counter's final value.  Exit status 0 and "index ok" on success.
//   tile_handout_emul walk K ROUNDS G ORDER SKIP THR IN OUT
//       walk the bytes of file IN (k = 12, 31 or 88; tiles of ROUNDS rounds; ORDER 0: workgroup 0 takes every ticket, 1: strict
//       round-robin, 2: seeded shuffle, 3: no counter, the static stride) and write the kept hashes as u64 to file OUT in the
//       order they were kept.  tests/test_tile_handout_cpu.py compares them with the oracle.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../sourmash_amd/csrc/kmer_core.hpp"

constexpr int BLOCK = 256, P = 16, R_MAX = 3;
enum Order { ONE_TAKES_ALL = 0, ROUND_ROBIN = 1, SHUFFLE = 2, STATIC_STRIDE = 3 };

// which workgroup runs its next tile: `live` holds the workgroups that still have one
struct Scheduler {
    int order;
    uint64_t state = 0x9e3779b97f4a7c15ull;
    size_t pos = 0;                                                              // round-robin: the place in `live` that is next
    size_t pick(const std::vector<uint32_t>& live) {
        if (order == ONE_TAKES_ALL || order == STATIC_STRIDE) return 0;          // the lowest live workgroup until it is done
        if (order == ROUND_ROBIN) return pos % live.size();
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (size_t)((state >> 33) % live.size());
    }
    void ran(size_t at, bool done) { pos = done ? at : at + 1; }                 // a workgroup that left: the one behind it is next
};

// The walk of G workgroups over n_tiles tiles: visit(workgroup, tile) for every tile a workgroup runs.  -> tickets taken.
template <class Visit>
static uint64_t walk_tiles(uint32_t G, uint64_t n_tiles, int order, Visit&& visit) {
    uint64_t counter = 0;
    const bool handout = order != STATIC_STRIDE;
    std::vector<uint64_t> tile(G);
    std::vector<uint32_t> live;
    for (uint32_t w = 0; w < G; ++w) {
        tile[w] = smg::tile_first(w);
        if (!smg::tile_end(tile[w], n_tiles)) live.push_back(w);
    }
    Scheduler sched{order};
    while (!live.empty()) {
        size_t at = sched.pick(live);
        const uint32_t w = live[at];
        // one turn of the kernel's loop: the ticket for the next tile in front of the hashing, the tile, then the move
        const uint64_t next = handout ? smg::tile_from_ticket(G, counter++) : tile[w] + G;
        visit(w, tile[w]);
        tile[w] = next;
        const bool done = smg::tile_end(tile[w], n_tiles);
        if (done) live.erase(live.begin() + (long)at);
        sched.ran(at, done);
    }
    return counter;
}

static int fail(const char* what, uint32_t G, uint64_t n_tiles, int order) {
    fprintf(stderr, "index rule: %s (G = %u, n_tiles = %llu, order %d)\n", what, G, (unsigned long long)n_tiles, order);
    return 1;
}

static int check_index_rule() {
    const uint32_t Gs[] = {1, 3, 8};
    int cases = 0;
    for (uint32_t G : Gs) {
        const uint64_t ns[] = {0, 1, (uint64_t)G - 1, G, (uint64_t)G + 1, 5ull * G + 3};
        for (uint64_t n_tiles : ns) {
            for (int order = ONE_TAKES_ALL; order <= STATIC_STRIDE; ++order) {
                std::vector<uint32_t> seen(n_tiles, 0);
                std::vector<uint64_t> per_wg(G, 0);
                bool past_end = false;
                const uint64_t tickets = walk_tiles(G, n_tiles, order, [&](uint32_t w, uint64_t t) {
                    if (t >= n_tiles) past_end = true;
                    else ++seen[t];
                    ++per_wg[w];
                });
                if (past_end) return fail("a tile index behind the end was walked", G, n_tiles, order);
                for (uint64_t t = 0; t < n_tiles; ++t)
                    if (seen[t] != 1) return fail(seen[t] ? "a tile was walked twice" : "a tile was not walked", G, n_tiles, order);
                if (order == STATIC_STRIDE) {
                    if (tickets != 0) return fail("the static stride took a ticket", G, n_tiles, order);
                } else if (n_tiles > G) {
                    // n_tiles - G tiles are reached by ticket, and each of the G workgroups takes one ticket that fails
                    if (tickets != n_tiles - G + G) return fail("the counter does not end at n_tiles - G + G", G, n_tiles, order);
                } else {
                    // every workgroup that has a tile takes its one failing ticket; the launcher passes no counter here
                    if (tickets != n_tiles) return fail("the counter does not end at the number of workgroups with a tile", G, n_tiles, order);
                }
                if (order == ONE_TAKES_ALL && n_tiles > G && per_wg[0] != n_tiles - G + 1)
                    return fail("workgroup 0 did not take every ticket", G, n_tiles, order);
                if (order == ROUND_ROBIN && n_tiles > G)
                    for (uint32_t w = 0; w < G; ++w)
                        if (per_wg[w] < n_tiles / G || per_wg[w] > n_tiles / G + 1) return fail("round-robin is not even", G, n_tiles, order);
                ++cases;
            }
        }
    }
    printf("index ok: %d cases\n", cases);
    return 0;
}

// What a workgroup keeps from tile to tile: never cleared here between tiles except where the kernel clears it.
template <int K>
struct Workgroup {
    using T = smg::TileGeom<K, P, BLOCK, R_MAX>;
    std::vector<uint32_t> s_in = std::vector<uint32_t>(T::IN_CHUNKS * 4, 0x41414141u), s_comp = std::vector<uint32_t>(T::IN_CHUNKS * 4, 0x54545454u);
    unsigned s_dirty = 1;                                      // a stale flag: the kernel zeroes it in front of every tile
};

template <int K>
static int walk(const std::vector<uint8_t>& in, uint32_t rounds, uint32_t G, int order, uint32_t skip, uint64_t thr, std::vector<uint64_t>& out) {
    using T = smg::TileGeom<K, P, BLOCK, R_MAX>;
    // what the launcher does: back to the 16-byte boundary, the prefix counted in, tiles of the length this launch walks
    std::vector<uint8_t> buf(skip + in.size() + 1, (uint8_t)'A');
    if (!in.empty()) std::memcpy(buf.data() + skip, in.data(), in.size());
    const uint64_t total = in.size() + skip, tile_len = (uint64_t)rounds * T::WINDOW;
    const uint64_t n_tiles = (total + tile_len - 1) / tile_len;
    std::vector<Workgroup<K>> wgs(G);
    walk_tiles(G, n_tiles, order, [&](uint32_t w, uint64_t tile) {
        Workgroup<K>& wg = wgs[w];
        const uint64_t base = tile * tile_len;
        wg.s_dirty = 0;
        smg::stage_tile<T::IN_CHUNKS, true, BLOCK>(buf.data(), base, total, skip, wg.s_in.data(), wg.s_comp.data(), &wg.s_dirty,
                                                   T::chunks((int)rounds));
        for (uint32_t r = 0; r < rounds; ++r) {
            for (int tid = 0; tid < BLOCK; ++tid) {
                uint32_t U[T::LANE_RD], C[T::LANE_RD];
                smg::read_window<T::LANE_RD, P>(wg.s_in.data(), tid + (int)r * BLOCK, U);
                smg::read_window<T::LANE_RD, P>(wg.s_comp.data(), tid + (int)r * BLOCK, C);
                smg::process_lane_staged<K, P>(U, C, wg.s_dirty != 0, 42, thr, [&](int, uint64_t h) { out.push_back(h); });
            }
        }
    });
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "index") return check_index_rule();
    if (argc != 10 || std::string(argv[1]) != "walk") {
        fprintf(stderr, "usage: %s index | walk K ROUNDS G ORDER SKIP THR IN OUT\n", argv[0]);
        return 2;
    }
    const int k = atoi(argv[2]), order = atoi(argv[5]);
    const uint32_t rounds = (uint32_t)atoi(argv[3]), G = (uint32_t)atoi(argv[4]), skip = (uint32_t)atoi(argv[6]);
    const uint64_t thr = strtoull(argv[7], nullptr, 10);
    if (rounds < 1 || rounds > (uint32_t)R_MAX || G < 1 || order < ONE_TAKES_ALL || order > STATIC_STRIDE || skip >= 16) return 2;
    std::vector<uint8_t> in;
    FILE* f = fopen(argv[8], "rb");
    if (!f) return 2;
    uint8_t chunk[65536];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) in.insert(in.end(), chunk, chunk + n);
    fclose(f);
    std::vector<uint64_t> out;
    int rc;
    switch (k) {
    case 12: rc = walk<12>(in, rounds, G, order, skip, thr, out); break;
    case 31: rc = walk<31>(in, rounds, G, order, skip, thr, out); break;
    case 88: rc = walk<88>(in, rounds, G, order, skip, thr, out); break;
    default: return 2;
    }
    f = fopen(argv[9], "wb");
    if (!f) return 2;
    if (!out.empty() && fwrite(out.data(), 8, out.size(), f) != out.size()) rc = 2;
    fclose(f);
    return rc;
}
