// sketch_long.hip -- the appending form of the register-window sketch kernel for k = 65 .. SK_FAST_MAX_K = 88: parts 4 and 5 of
// its launch table, compiled with -DKMER_PART=0..1 (sketch_kernel.hpp says where the line to sketch_words.hip is drawn, and why).
#include "sketch_kernel.hpp"
namespace smg { SMG_KMER_PART(SketchLaunch<false>, 4 + KMER_PART) }
