// sketch_records_k.hip -- the (hash, position) kernel (records_kernel.hpp) for every k = 1 .. SK_FAST_MAX_K = 88, compiled six
// times (-DREC_PART=0..5, up to 16 ksizes each: the Makefile) so that the fully unrolled instantiations build side by side.
#include "records_kernel.hpp"

#ifndef REC_PART
#error "compile with -DREC_PART=0..5"
#endif

namespace smg {

#define REC_CAT2(a, b) a##b
#define REC_CAT(a, b) REC_CAT2(a, b)
// ksizes 1 + 16 * part .. min(16 + 16 * part, SK_FAST_MAX_K)
records_launch_fn REC_CAT(records_launcher_, REC_PART)(uint32_t k) {
    return records_launcher_from<16 * REC_PART>(k, std::make_integer_sequence<int, sk_part_size(16 * REC_PART)>());
}

}  // namespace smg
