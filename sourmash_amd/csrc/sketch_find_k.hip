// sketch_find_k.hip -- the k-mer finding kernel (find_kernel.hpp) for every k = 1 .. SK_FAST_MAX_K = 88: one part of its launch
// table per -DKMER_PART=0..5.
#include "find_kernel.hpp"
namespace smg { SMG_KMER_PART(FindLaunch, KMER_PART) }
