// sketch_records_k.hip -- the (hash, position) kernel (records_kernel.hpp) for every k = 1 .. SK_FAST_MAX_K = 88: one part of
// its launch table per -DKMER_PART=0..5.
#include "records_kernel.hpp"
namespace smg { SMG_KMER_PART(RecordsLaunch, KMER_PART) }
