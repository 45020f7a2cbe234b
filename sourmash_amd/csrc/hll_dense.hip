// hll_dense.hip -- the HyperLogLog register kernel (hll_kernel.hpp) for every k = 1 .. SK_FAST_MAX_K = 88: one part of its
// launch table per -DKMER_PART=0..5.
#include "hll_kernel.hpp"
namespace smg { SMG_KMER_PART(HllLaunch, KMER_PART) }
