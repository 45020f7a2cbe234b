// nodegraph.hip -- Nodegraph (khmer's Bloom filter, sketch/nodegraph.rs) bits set and tested on the GPU.
//
// A graph is n tables of prime sizes; a hash h sets bit h mod size_t of every table t.  k-mers are hashed with khmer's two-bit
// code (A 0, T 1, C 2, G 3): h = min(forward word, reverse-complement word), k <= 32.  The device mirror of a graph is one
// u32 word array (all tables, fixedbitset layout: bit b = bit b & 31 of word b >> 5) plus a table of {size, reciprocal,
// first word} (NgTable) and a u64 counter of table-0 bits turned on (capi_nodegraph.cpp keeps it resident and adds the counter to the
// host's `occupied` when it reads the tables back).
//
//   h mod size: ng_mod (nodegraph_core.hpp), a mulhi quotient estimate by the precomputed floor((2^64 - 1) / size) and at
//               most two corrections -- no 64-bit divide in the loop, exact for every h and size < 2^63.
//   LDS form (all words <= 64 KiB, e.g. the SBT graphs: 4 x 100,000 bits = 50 KB): each workgroup sets bits in its own copy
//               with LDS atomic OR and folds the copy into the device words at the end (an atomicOr only for words holding
//               a bit the device does not show yet).  The grid keeps at least 8 tiles per workgroup, so that the fold stays
//               small next to the hashing (the HLL kernel's rule).
//   global form: atomicOr on the device words behind a read filter (bits only turn on: a bit already seen set needs no
//               atomic).  On large sparse tables nearly every k-mer misses the filter: one random 4-byte atomic per table and
//               k-mer, which bounds this form (cdna_hip_programming.md, Guideline 12).
//   occupied:   the table-0 bits that went from 0 to 1, taken from the old words the atomics return (global form: per bit;
//               LDS form: per folded word), summed per wave, one atomicAdd per wave.  The count does not depend on the
//               order of the updates, so bulk results equal the host's one-by-one result exactly.
//
// The k-mer walk is a run-time-k loop of shifts and masks (no per-K instantiation: the table updates, not the walk, bound it).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_api.hpp"
#include "nodegraph_kernel.hpp"
#include "tile_launch.hpp"

namespace smg {

static bool ng_lds(const NgDev& g) { return g.n_words <= NG_LDS_MAX_WORDS; }

hipError_t nodegraph_dna_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, const NgDev& g, hipStream_t stream) {
    if (k == 0 || k > NG_MAX_K) return hipErrorInvalidValue;
    if (len < k || g.n_tables == 0) return hipSuccess;
    const TileSpan t = align_to_tiles(d_seq, len, NG_TILE);
    const bool lds = ng_lds(g);
    const unsigned grid = lds_grid(t.n_tiles, lds);
    if (lds) {
        const size_t shm = (size_t)g.n_words * 4;
        const hipError_t allowed = allow_dynamic_lds<&ng_dna_kernel<true>>(shm, (size_t)NG_LDS_MAX_WORDS * 4);
        if (allowed != hipSuccess) return allowed;
        hipLaunchKernelGGL(ng_dna_kernel<true>, dim3(grid), dim3(NG_BLOCK), shm, stream, t.seq, t.len, k, g.tabs, g.n_tables,
                           g.words, (uint32_t)g.n_words, g.t0_words, g.occ, t.n_tiles, t.skip);
    } else {
        hipLaunchKernelGGL(ng_dna_kernel<false>, dim3(grid), dim3(NG_BLOCK), 0, stream, t.seq, t.len, k, g.tabs, g.n_tables,
                           g.words, 0u, g.t0_words, g.occ, t.n_tiles, t.skip);
    }
    return hipGetLastError();
}

hipError_t nodegraph_hashes_launch(const uint64_t* d_hashes, uint64_t n, const NgDev& g, hipStream_t stream) {
    if (n == 0 || g.n_tables == 0) return hipSuccess;
    const uint64_t nb = (n + NG_BLOCK - 1) / NG_BLOCK;
    const bool lds = ng_lds(g);
    // LDS form: at least 8 blocks' worth of hashes per workgroup, as for the k-mer kernel's tiles
    const unsigned grid = lds_grid(nb, lds);
    if (lds) {
        const size_t shm = (size_t)g.n_words * 4;
        const hipError_t allowed = allow_dynamic_lds<&ng_hashes_kernel<true>>(shm, (size_t)NG_LDS_MAX_WORDS * 4);
        if (allowed != hipSuccess) return allowed;
        hipLaunchKernelGGL(ng_hashes_kernel<true>, dim3(grid), dim3(NG_BLOCK), shm, stream, d_hashes, n, g.tabs, g.n_tables,
                           g.words, (uint32_t)g.n_words, g.t0_words, g.occ);
    } else {
        hipLaunchKernelGGL(ng_hashes_kernel<false>, dim3(grid), dim3(NG_BLOCK), 0, stream, d_hashes, n, g.tabs, g.n_tables,
                           g.words, 0u, g.t0_words, g.occ);
    }
    return hipGetLastError();
}

hipError_t nodegraph_matches_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n_rows, const NgDev& g,
                                    uint64_t* d_out, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    const uint64_t nb = (n_rows + (NG_BLOCK / 64) - 1) / (NG_BLOCK / 64);
    const unsigned grid = (unsigned)(nb < 4096 ? nb : 4096);
    hipLaunchKernelGGL(ng_matches_kernel, dim3(grid), dim3(NG_BLOCK), 0, stream, d_hashes, d_offsets, n_rows, g.tabs, g.n_tables,
                       (const uint32_t*)g.words, d_out);
    return hipGetLastError();
}

}  // namespace smg
