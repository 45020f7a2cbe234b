// tile_launch.hpp -- the host side of the DNA k-mer kernels' tile walk: the aligned span a launch covers, its grid, the dynamic
// LDS permission, and the per-k launch table with the parts it is compiled in.  Used by every launcher of a kernel that stages
// 16-byte chunks of a tile (sketch_kernel.hpp, records_kernel.hpp, hll_kernel.hpp, sketch_multi.hip, sketch_words.hip,
// nodegraph.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>

namespace smg {

// The caller's buffer moved down to a 16-byte boundary: the kernels load whole aligned chunks.  The first `skip` (< 16) bytes of
// seq precede the caller's buffer and are blanked where the tile is staged; len includes them.
struct TileSpan {
    const uint8_t* seq;
    uint64_t len;
    uint32_t skip;
    uint64_t n_tiles;
};
inline TileSpan align_to_tiles(const uint8_t* d_seq, uint64_t len, uint64_t tile_positions) {
    const uint32_t skip = (uint32_t)((uintptr_t)d_seq & 15);
    return {d_seq - skip, len + skip, skip, (len + skip + tile_positions - 1) / tile_positions};
}

// workgroups for a launch: one per tile up to per_cu (8) for each of the 256 CUs, the rest by grid stride.  n_tiles counts tiles of
// the length the launch walks (a tile of the staged sketch kernel is several window rounds; its launcher starts the resident
// workgroups and hands the tiles out by tickets, or asks for more workgroups per CU on the static stride, sketch_kernel.hpp).
inline unsigned sk_grid(uint64_t n_tiles, unsigned per_cu = 8) {
    const uint64_t max_blocks = 256ull * per_cu;
    return (unsigned)(n_tiles < max_blocks ? n_tiles : max_blocks);
}
// for a kernel that keeps a table per workgroup in LDS and folds it into the device's at the end (HyperLogLog registers, Nodegraph
// words): still up to 2048, but in the LDS form at least 8 tiles per workgroup, so that the fold (about one tile's work for
// 64 KiB) stays small next to the hashing
inline unsigned lds_grid(uint64_t n_tiles, bool lds) {
    uint64_t g = sk_grid(n_tiles);
    if (lds && g > 256 && g > n_tiles / 8) g = n_tiles / 8 > 256 ? n_tiles / 8 : 256;
    return (unsigned)g;
}

// A kernel gets 48 KiB of dynamic LDS unasked.  A launch with more (`bytes`) has to be allowed, once per kernel: `most` is the
// largest size the kernel is ever launched with.
template <auto Kernel>
hipError_t allow_dynamic_lds(size_t bytes, size_t most) {
    if (bytes <= 48 * 1024) return hipSuccess;
    static const hipError_t allowed = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
    return allowed;
}

// ---- one launcher per ksize ---------------------------------------------------------------------------------------------------
// A kernel family F that is unrolled per ksize is a struct with the launcher's type `fn` and `template <int K> static launch`.
// launcher<F>(k) is F::launch<k>.  The instantiations of a family are compiled in parts of K_PART ksizes each -- part i holds
// k = 16 i + 1 .. min(16 i + 16, KMAX) -- so that they build side by side: a translation unit compiled with -DKMER_PART=i
// defines part i with SMG_KMER_PART (the Makefile lists the families and their parts).
constexpr int K_PART = 16;

// table[k - K0 - 1] of F::launch<K0 + 1> .. F::launch<K0 + N>
template <class F, int K0, int... KS>
typename F::fn k_launcher_from(uint32_t k, std::integer_sequence<int, KS...>) {
    static const typename F::fn table[] = {&F::template launch<K0 + KS + 1>...};
    return table[k - K0 - 1];
}
template <class F, int PART>
typename F::fn part_launcher(uint32_t k);        // defined where the part is compiled
template <class F>
typename F::fn launcher(uint32_t k) {
    static_assert(F::KMAX > 5 * K_PART && F::KMAX <= 6 * K_PART, "six parts");
    switch ((k - 1u) / (uint32_t)K_PART) {
    case 0: return part_launcher<F, 0>(k);
    case 1: return part_launcher<F, 1>(k);
    case 2: return part_launcher<F, 2>(k);
    case 3: return part_launcher<F, 3>(k);
    case 4: return part_launcher<F, 4>(k);
    default: return part_launcher<F, 5>(k);
    }
}
#define SMG_KMER_PART(F, PART)                                                                                                   \
    template <>                                                                                                                  \
    typename F::fn part_launcher<F, PART>(uint32_t k) {                                                                          \
        constexpr int K0 = K_PART * (PART), N = F::KMAX - K0 < K_PART ? F::KMAX - K0 : K_PART;                                   \
        return k_launcher_from<F, K0>(k, std::make_integer_sequence<int, N>());                                                  \
    }

}  // namespace smg
