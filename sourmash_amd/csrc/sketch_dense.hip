// sketch_dense.hip -- the register-window kernel in its per-position form (one hash per k-mer start: kmerminhash_seq_to_hashes,
// src/core/src/ffi/minhash.rs:63-99 over src/core/src/signature.rs:246-306) for every k = 1 .. SK_FAST_MAX_K = 88: one part of
// its launch table per -DKMER_PART=0..5.
#include "sketch_kernel.hpp"
namespace smg { SMG_KMER_PART(SketchLaunch<true>, KMER_PART) }
