// hll_dense.hip -- the HyperLogLog register kernel (hll_kernel.hpp) for every k = 1 .. SK_FAST_MAX_K = 88, compiled six times
// (-DHLL_PART=0..5, up to 16 ksizes each: the Makefile) so that the fully unrolled instantiations build side by side.
#include "hll_kernel.hpp"

#ifndef HLL_PART
#error "compile with -DHLL_PART=0..5"
#endif

namespace smg {

#define HLL_CAT2(a, b) a##b
#define HLL_CAT(a, b) HLL_CAT2(a, b)
// ksizes 1 + 16 * part .. min(16 + 16 * part, SK_FAST_MAX_K)
hll_launch_fn HLL_CAT(hll_launcher_, HLL_PART)(uint32_t k) {
    return hll_launcher_from<16 * HLL_PART>(k, std::make_integer_sequence<int, sk_part_size(16 * HLL_PART)>());
}

}  // namespace smg
