// sketch_kernel.hpp -- the register-window DNA sketch kernel (template) and its launcher, shared by the translation units
// that instantiate it: sketch.hip (k = 1 .. 64), sketch_long.hip (k = 65 .. SK_FAST_MAX_K, two parts) and sketch_dense.hip (the
// per-position form of all of them, six parts), so that the fully unrolled instantiations compile side by side.  See sketch.hip
// for the design notes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "kmer_core.hpp"
#include "tile_launch.hpp"
#include "arena.hpp"

namespace smg {

constexpr int SK_BLOCK = 256;      // 4 waves, one per SIMD
// The longest k-mer the unrolled kernel is instantiated for.  Its window lives in registers: from k = 89 on an instantiation needs
// more than 256 of them and runs one wave per SIMD (k = 88: 131 Gbase/s, k = 96: 93), where the run-time-k kernel of
// sketch_words.hip -- 67 registers at any k -- is already faster (k = 96: 106, k = 128: 85 against 68; profiles/r05_long_k.json).
constexpr int SK_FAST_MAX_K = 88;
constexpr int SK_OUT_CAP = 2048;   // LDS staging entries for kept hashes (16 KiB)

// The instantiations that keep the plain 64-bit constant multiply in their hash (murmur3.hpp, mul_c64<C, PLAIN>): with the limb
// form's one more live register each of these would run one wave per SIMD fewer (profiles/mul_c64_kernel_resources.txt).
constexpr bool sk_plain_mul(int k, bool dense) {
    if (dense) return k == 1 || k == 5 || k == 8 || k == 25 || k == 28 || k == 81 || k == 82 || k == 84;
    return k == 50 || k == 51;
}
// The appending form stages the tile upper-cased and complemented and has the lanes read both from LDS (kmer_core.hpp,
// process_lane_staged).  An instantiation that would run fewer waves per SIMD that way stays on process_lane: k <= 11, where the
// second copy's 4 KiB of LDS take the seventh workgroup of a CU, and k = 18, 20 and 30, which need a few registers more and
// cross a step of the register file (profiles/strand_lds_kernel_resources.txt).
constexpr bool sk_staged(int k) { return k > 11 && k != 18 && k != 20 && k != 30; }
// The staged appending form walks tiles of several window rounds: R_MAX consecutive windows of SK_BLOCK x 16 positions (x 32
// where sk_lane_positions says so, below, with rounds and sink of its own) are
// staged together, behind one pair of barriers, one wait for the global loads and one halo, and a rolled loop takes the lanes
// through them (`rounds`, a launch argument: 1 where the sink could overfill between two flush checks, kmer_core.hpp
// sk_tile_rounds).  SK_R_MAX sizes the LDS copies: 2 with the 2,048-entry sink and 3 with a 1,024-entry one are about 33 KB at
// k = 31, so that the four workgroups per CU the registers allow still fit in 160 KB.  An instantiation that runs more than four
// workgroups per CU by its registers would lose one to the longer tile's LDS and stays at one round
// (profiles/tile_rounds_kernel_resources.txt).
#ifndef SMG_SK_R_MAX
#define SMG_SK_R_MAX 3
#endif
constexpr int SK_R_MAX = SMG_SK_R_MAX;
static_assert(SK_R_MAX >= 1 && SK_R_MAX <= 3, "four rounds do not fit four workgroups per CU");
// The last key dword of a K % 4 != 0 masked once behind the strand select instead of once per strand (kmer_core.hpp, PosOps):
// the staged appending form, but for k = 13, which would run five workgroups per CU instead of six with it (80 -> 82 registers).
constexpr bool sk_late_mask(int k) { return sk_staged(k) && k != 13; }
constexpr bool sk_one_round(int k) { return k <= 17; }      // k = 12, 13: six workgroups per CU, 14 .. 17: five
// Start positions a lane takes per round.  The kernel's template argument P stays 16 -- it is the kernel's name, which the
// benchmark, the counter summaries and tools/valu_mix.py look it up by -- and the kernel derives its lane geometry from this rule.
// 32 in the staged appending form of several rounds (k >= 19): a lane's window is P + K - 1 bytes, and the unaligned forward
// dwords (P + 28 offsets at k = 31), the reverse dwords (P + 24) and the compare words are shared between the positions of a
// lane, so the halo's share of the byte plumbing halves when P doubles, and a lane reads 8 x 16 bytes of LDS per 32 positions
// where two rounds of 16 read 12.  An instantiation that would run fewer waves per SIMD, gain scratch or spill with the longer
// window's registers stays at 16 (sk_lane16_only; profiles/lane32_kernel_resources.txt), as do the per-position form, the
// unstaged k and k <= 17.  SMG_SK_LANE_POSITIONS: a variant build with one value for every k of the rule, for A/B runs.
constexpr bool sk_lane16_only(int k) { return (k >= 35 && k <= 40) || (k >= 53 && k <= 56); }   // past 128 / 168 registers at 32
#ifndef SMG_SK_LANE_POSITIONS
#define SMG_SK_LANE_POSITIONS 32
#endif
constexpr int sk_lane_positions(int k, bool dense) {
    return !dense && sk_staged(k) && !sk_one_round(k) && !sk_lane16_only(k) ? SMG_SK_LANE_POSITIONS : 16;
}
// Rounds and sink by the window: with 32 positions per lane a window is 8,192 positions, and two rounds (2 x 16.4 KB of copies at
// k = 31) with a 512-entry sink are 36.9 KB, one round with the 2,048-entry sink 32.8 KB: four workgroups per CU fit either way,
// three rounds do not.  SMG_SK_LANE32_R_MAX: the other of the two, for A/B runs (profiles/lane32_bench.txt).
#ifndef SMG_SK_LANE32_R_MAX
#define SMG_SK_LANE32_R_MAX 2
#endif
static_assert(SMG_SK_LANE32_R_MAX >= 1 && SMG_SK_LANE32_R_MAX <= 2, "three rounds of 8,192 positions do not fit four workgroups per CU");
constexpr int sk_rounds_max(int k, bool dense) {
    if (dense || !sk_staged(k) || sk_one_round(k)) return 1;
    return sk_lane_positions(k, dense) == 32 ? SMG_SK_LANE32_R_MAX : SK_R_MAX;
}
// Sink entries by the tile's length in positions (r_max rounds of SK_BLOCK x lane_positions): the longer the tile's copies, the
// smaller the sink beside them.  A tile of 16,384 positions is expected to keep about 16 hashes at scaled = 1,000, well under
// the quarter of 512 entries that sk_tile_rounds asks for and the half at which the sink is flushed.
constexpr int sk_out_cap(int r_max, int lane_positions = 16) {
    const int tile = r_max * SK_BLOCK * lane_positions;
    return tile >= 16384 ? SK_OUT_CAP / 4 : tile >= 12288 ? SK_OUT_CAP / 2 : SK_OUT_CAP;
}
// The appending form hands its tiles out by tickets where a launch has more tiles than workgroups (tile_counter below): a
// workgroup's share is then what it gets through, not a fixed 1 / grid of the tiles, and the launch ends within one tile's time
// of its last workgroup, whatever the grid.  An instantiation that would run fewer waves per SIMD with the ticket's LDS word
// stays on the static stride; none does (profiles/tile_handout_kernel_resources.txt).  SMG_SK_STATIC_WALK: a variant build
// without tickets, for A/B runs.
#ifdef SMG_SK_STATIC_WALK
constexpr bool sk_handout(int) { return false; }
#else
constexpr bool sk_handout(int) { return true; }
#endif
// The staged appending form of several rounds stages a tile that lies wholly inside the buffer in one batch (kmer_core.hpp,
// stage_tile<.., BATCH>): a lane issues the loads of all its chunks -- five at k = 31, 1,026 chunks for 256 lanes, the two
// stray ones of the halo among them -- in front of the first use, where the rolled loop pays a round trip to memory per trip.
// The loads live in the turnover between two tiles, where the window's registers are dead.  A launch that walks tiles of one
// round (small `scaled`, num sketches) stays on the loop: whole trips of the batch would serve no chunk there.  An instantiation
// that would run fewer waves per SIMD, gain scratch or spill with the batch stays on the loop; none does
// (profiles/stage_batch_kernel_resources.txt) -- but that holds by an empty asm in stage_tile that keeps the staging addresses
// out of the hash loop's registers, which no test guards: re-run tools/kernel_resources.py after a compiler change.
// SMG_SK_STAGE_LOOP: a variant build with the loop everywhere, for A/B runs.
#ifdef SMG_SK_STAGE_LOOP
constexpr bool sk_stage_batched(int) { return false; }
#else
constexpr bool sk_stage_batched(int k) { return sk_staged(k) && !sk_one_round(k); }
#endif
// Workgroups per CU a launch may ask for (tile_launch.hpp, sk_grid); 0: as many workgroups as are resident at once
// (sk_resident_grid), which is what a launch with tickets takes -- at k = 31 a step of the benchmark took 27.04 ms with the 1,024
// resident workgroups, 27.01 with 2,048 and 27.03 with 8,192, a tie, and the smallest grid has the fewest start-ups and partial
// flushes (profiles/tile_handout_bench.txt).  On the static stride the long tiles want a large grid, for with three times fewer of
// them the end of the launch weighs more: 29.2 ms with 2,048 workgroups, 28.2 with 4,096, 27.7 with 8,192
// (profiles/tile_rounds_bench.txt), 27.5 with 16,384 and 27.3 with 32,768.  SMG_SK_GRID_PER_CU: a variant build that measures
// another cap, for every instantiation.
#ifdef SMG_SK_GRID_PER_CU
constexpr unsigned sk_grid_per_cu(int, bool) { return SMG_SK_GRID_PER_CU; }
#else
constexpr unsigned sk_grid_per_cu(int r_max, bool handout) { return handout ? 0 : r_max > 1 ? 32 : 8; }
#endif

// DENSE == false: append kept hashes (unordered) to out, count in *out_count.
// DENSE == true : out[i] = hash of the k-mer starting at i (out pre-zeroed by the
//                 caller; bad k-mers and hash 0 stay 0) -- kmerminhash_seq_to_hashes.
template <int K, int P, bool DENSE>
__global__ __launch_bounds__(SK_BLOCK) void sketch_dna_kernel(
    const uint8_t* __restrict__ seq, uint64_t len, uint64_t seed, uint64_t thr,
    uint64_t* __restrict__ out, unsigned long long* __restrict__ out_count, uint64_t out_cap,
    uint64_t n_tiles, uint32_t skip, uint32_t rounds, unsigned long long* __restrict__ tile_counter) {
    // seq is 16-byte aligned; its first `skip` (< 16) bytes precede the caller's buffer and are
    // treated as invalid.  len includes them.  DENSE positions are reported relative to seq + skip.
    // A tile is `rounds` (1 .. R_MAX) windows of SK_BLOCK x LP positions (LP = sk_lane_positions(K, DENSE), not P); n_tiles counts tiles of that length.
    // tile_counter (appending form only): null, and the workgroups walk the tiles by stride; or a zeroed counter of this launch
    // alone, and every tile behind a workgroup's first is handed out by a ticket from it (kmer_core.hpp, tile_first).
    static_assert(P == 16, "the kernel's name; the lane's positions are LP");
    constexpr int LP = sk_lane_positions(K, DENSE);          // start positions per lane and round
    constexpr int R_MAX = sk_rounds_max(K, DENSE), OUT_CAP = sk_out_cap(R_MAX, LP);
    using T = TileGeom<K, LP, SK_BLOCK, R_MAX>;
    constexpr int WINDOW = T::WINDOW, LANE_RD = T::LANE_RD, IN_CHUNKS = T::IN_CHUNKS;
    constexpr bool STAGED = !DENSE && sk_staged(K);          // per-byte work at staging, U and C from LDS
    static_assert(R_MAX == 1 || STAGED, "only the staged form walks several rounds");
    const uint32_t n_rounds = R_MAX > 1 ? rounds : 1u;

    __shared__ __attribute__((aligned(16))) uint32_t s_in[IN_CHUNKS * 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_comp[STAGED ? IN_CHUNKS * 4 : 4];   // complement of s_in, byte for byte
    __shared__ unsigned int s_dirty;                          // some staged byte of the tile is not ACGT
    __shared__ uint64_t s_out[OUT_CAP];
    __shared__ unsigned int s_cnt;
    __shared__ unsigned long long s_base;
    __shared__ unsigned long long s_next;                     // the tile behind this one, where tickets hand them out
    const bool handout = !DENSE && sk_handout(K) && tile_counter != nullptr;
    const LdsSink<OUT_CAP, SK_BLOCK> sink{{s_out}, &s_cnt, &s_base, {out}, out_count, out_cap};

    const int tid = threadIdx.x;
    if (tid == 0) s_cnt = 0;

    uint64_t tile = tile_first(blockIdx.x);
    while (!tile_end(tile, n_tiles)) {
        const uint64_t base = tile * ((uint64_t)n_rounds * WINDOW);
        if constexpr (STAGED) {
            if (tid == 0) s_dirty = 0;   // its readers of the previous tile are behind that tile's flush barrier
        }
        __syncthreads();   // previous tile's readers are done with s_in; s_cnt reset visible
        if constexpr (STAGED) {
            constexpr bool BATCH = sk_stage_batched(K);
            if constexpr (R_MAX > 1) stage_tile<IN_CHUNKS, true, SK_BLOCK, BATCH>(seq, base, len, skip, s_in, s_comp, &s_dirty, T::chunks((int)n_rounds));
            else stage_tile<IN_CHUNKS, true, SK_BLOCK, BATCH>(seq, base, len, skip, s_in, s_comp, &s_dirty);
        } else {
            // stage_tile<IN_CHUNKS, false> (kmer_core.hpp), kept inline: through the function, in either shape of its loader, the
            // dense k = 1 goes from 64 to 66 VGPRs, the dense k = 25 from 128 to 130, the appending k = 18 from 96 to 98 -- a wave
            // per SIMD each.
            for (int c = tid; c < IN_CHUNKS; c += SK_BLOCK) {
                const uint64_t off = base + (uint64_t)c * 16;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (off + 16 <= len) {
                    v = *reinterpret_cast<const uint4*>(seq + off);
                } else if (off < len) {
                    uint32_t w[4] = {0, 0, 0, 0};
                    for (uint64_t b = off; b < len; ++b) w[(b - off) >> 2] |= (uint32_t)seq[b] << (8 * ((b - off) & 3));
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                if (off == 0 && skip) {                      // blank the alignment prefix
                    uint32_t w[4] = {v.x, v.y, v.z, v.w};
                    for (uint32_t b = 0; b < skip; ++b) w[b >> 2] &= ~(0xffu << (8 * (b & 3)));
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                *reinterpret_cast<uint4*>(&s_in[c * 4]) = v;
            }
        }
        __syncthreads();
        if constexpr (!DENSE && sk_handout(K)) {
            // The ticket for the next tile, taken early: its round trip lies behind this tile's hashing.  No workgroup waits for
            // another.  s_next is read behind the sink barrier below; its next writer is then behind the next tile's two barriers.
            if (handout && tid == 0) s_next = tile_from_ticket(gridDim.x, atomicAdd(tile_counter, 1ull));
        }
        uint32_t raw[LANE_RD];
        if constexpr (R_MAX == 1) read_window<LANE_RD, LP>(s_in, tid, raw);
        auto emit = [&](int o, uint64_t h) {
            if constexpr (DENSE) {
                const uint64_t pos = base + (uint64_t)tid * LP + (uint64_t)o - skip;   // valid k-mers never start in the prefix
                if (pos < out_cap) out[pos] = h;
            } else {
                sink.append(h);
            }
        };
        if constexpr (STAGED) {
            static_assert(!STAGED || LP == 16 || LP == 32, "the staged form reads whole 16-byte groups");
            uint32_t comp[LANE_RD];
            if constexpr (R_MAX == 1) {
                read_window<LANE_RD, LP>(s_comp, tid, comp);
                const bool dirty = __builtin_amdgcn_readfirstlane(s_dirty) != 0;
                process_lane_staged<K, LP, true, sk_plain_mul(K, false), sk_late_mask(K)>(raw, comp, dirty, seed, thr, emit);
            } else {
                // the rounds of the tile, rolled: the position code stays one copy, its registers and its size what they were
                const bool dirty = __builtin_amdgcn_readfirstlane(s_dirty) != 0;   // one flag for the whole tile
#pragma unroll 1
                for (uint32_t r = 0; r < n_rounds; ++r) {
                    read_window<LANE_RD, LP>(s_in, tid + (int)r * SK_BLOCK, raw);
                    read_window<LANE_RD, LP>(s_comp, tid + (int)r * SK_BLOCK, comp);
                    process_lane_staged<K, LP, true, sk_plain_mul(K, false), sk_late_mask(K)>(raw, comp, dirty, seed, thr, emit);
                }
            }
        } else {
            process_lane<K, LP, !DENSE, sk_plain_mul(K, DENSE)>(raw, seed, thr, emit);
        }
        if constexpr (DENSE) { tile += gridDim.x; continue; }
        __syncthreads();
        if (handout) {                                        // read by every lane in front of the next tile's first barrier; kept scalar
            const unsigned long long next = s_next;
            tile = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(next >> 32)) << 32) |
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)next);
        } else {
            tile += gridDim.x;
        }
        sink.flush(OUT_CAP / 2);
    }
    if constexpr (DENSE) return;
    __syncthreads();
    sink.flush(1);
}

typedef hipError_t (*sketch_launch_fn)(const uint8_t*, uint64_t, uint64_t, uint64_t, uint64_t*, unsigned long long*, uint64_t, uint32_t, hipStream_t);
// Workgroups that are resident at once: the runtime's occupancy figure for the instantiation times the device's CUs, asked once.
template <int K, bool DENSE>
unsigned sk_resident_grid() {
    static const unsigned resident = [] {
        int per_cu = 0, dev = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)sketch_dna_kernel<K, 16, DENSE>, SK_BLOCK, 0) != hipSuccess ||
            hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            per_cu < 1 || cus < 1) {
            (void)hipGetLastError();
            return 2048u;
        }
        return (unsigned)per_cu * (unsigned)cus;
    }();
    return resident;
}
// The launchers of sketch_dna_kernel<K, 16, DENSE>, one per ksize (tile_launch.hpp: launcher<SketchLaunch<DENSE>>(k)).  DENSE ==
// false, the appending form: parts 0 .. 3 (k = 1 .. 64) in sketch.hip, 4 and 5 in sketch_long.hip.  DENSE == true, the
// per-position form (kmerminhash_seq_to_hashes: one hash per k-mer start, 0 for bad k-mers): six parts in sketch_dense.hip.
// grid: 0, the launcher's own number of workgroups, or exactly that many (the appending form; a test's way to many tiles per
// workgroup on a small input).
template <bool DENSE>
struct SketchLaunch {
    using fn = sketch_launch_fn;
    static constexpr int KMAX = SK_FAST_MAX_K;
    template <int K>
    static hipError_t launch(const uint8_t* d_seq, uint64_t len, uint64_t seed, uint64_t thr, uint64_t* d_out,
                             unsigned long long* d_count, uint64_t cap, uint32_t grid, hipStream_t stream) {
        // the rounds first: the tile count and the grid are those of the tile length this launch walks
        constexpr uint32_t LP = (uint32_t)sk_lane_positions(K, DENSE), WINDOW = (uint32_t)SK_BLOCK * LP;
        constexpr uint32_t R_MAX = (uint32_t)sk_rounds_max(K, DENSE);
        const uint32_t rounds = sk_tile_rounds(thr, R_MAX, WINDOW, (uint32_t)sk_out_cap((int)R_MAX, (int)LP));
        const TileSpan t = align_to_tiles(d_seq, len, (uint64_t)rounds * WINDOW);
        if (t.n_tiles == 0) return hipSuccess;
        constexpr unsigned per_cu = sk_grid_per_cu((int)R_MAX, !DENSE && sk_handout(K));
        unsigned g;
        if (grid && !DENSE) {
            g = grid;
        } else if constexpr (per_cu == 0) {                  // exactly the workgroups that are resident at once
            const unsigned resident = sk_resident_grid<K, DENSE>();
            g = (unsigned)(t.n_tiles < resident ? t.n_tiles : resident);
        } else {
            g = sk_grid(t.n_tiles, per_cu);
        }
        // Tickets only where some workgroup has a second tile.  The counter is this launch's own: 8 bytes of the arena, taken,
        // zeroed and released in the order of `stream`, so that neither the launch in front of this one on the stream nor one
        // in flight on another stream (whose block this is not, or whose release the arena has this stream wait for) sees it.
        ArenaBuf counter;
        if constexpr (!DENSE && sk_handout(K)) {
            if (t.n_tiles > g) {
                hipError_t e = counter.get(8, stream);
                if (e == hipSuccess) e = hipMemsetAsync(counter.p, 0, 8, stream);
                if (e != hipSuccess) return e;
            }
        }
        hipLaunchKernelGGL((sketch_dna_kernel<K, 16, DENSE>), dim3(g), dim3(SK_BLOCK), 0, stream,
                           t.seq, t.len, seed, thr, d_out, d_count, cap, t.n_tiles, t.skip, rounds, counter.as<unsigned long long>());
        return hipGetLastError();
    }
};

}  // namespace smg
