// record_queue.hpp -- the deferred-record queue behind add_sequence of MinHash, HyperLogLog and Nodegraph (host only; no HIP).
//
// The reference's loop is one add_sequence per record (src/sourmash/command_sketch.py:746-768, signature.rs:38-58).  A kernel
// launch per 150-base read would cost ~40 us of copy + launch + synchronise each, so add_sequence only validates the record and
// appends it to the container's `pending` string; the string goes through the family's k-mer kernel in one launch when it is
// large enough or when anything looks at the container ("settle").  `pending` stays a std::string member of the host containers
// (minhash_host.hpp, hll_host.hpp, nodegraph_host.hpp): their copy, assign and clear() carry it.
//
// The three families share the three pieces below -- where the valid prefix of a record ends, how a record is appended, what
// becomes of the queue's storage after a settle -- and differ in this, on purpose:
//
//   family       | consumed when the device work throws                              | lock for settle            | lock for append
//   -------------+-------------------------------------------------------------------+----------------------------+-------------------
//   MinHash      | yes: adding hashes is not idempotent for abundance counts         | ONE process-wide recursive | none
//                |                                                                   | mutex (capi.cpp)           |
//   HyperLogLog  | no: the queue stays and is hashed again later (max is idempotent) | the handle's settle_mu     | the handle's settle_mu
//   Nodegraph    | no: the queue stays and is counted again later (bits only turn on)| the handle's settle_mu     | the handle's settle_mu
//
// The ksize checks and early returns around these pieces are the families' own (capi.cpp: add_sequence_dna, capi_hll.cpp:
// hll_add_sequence_impl, capi_nodegraph.cpp: ng_add_sequence_impl).
#pragma once
#if defined(__SSE2__)
#include <emmintrin.h>
#endif
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>

#pragma GCC visibility push(hidden)   // nothing here belongs in the export table of a library that includes it
namespace smg {

constexpr size_t PENDING_FLUSH_BYTES = (size_t)32 << 20;            // a queue this large is settled from inside the add_sequence loop
constexpr size_t PENDING_KEEP_BYTES = (size_t)1 << 20;              // storage a settled queue may keep for the next records

// first byte outside ACGTacgt (what kills a k-mer, encodings.rs:370-377 after signature.rs:214's upper-casing), or SIZE_MAX.
// Only decides whether add_sequence(force = false) must raise and where the valid prefix ends; the k-mers themselves
// are validated again, hashed and filtered by the kernel.
inline size_t first_invalid_byte(const uint8_t* seq, size_t len) {
    static const struct Table {
        uint8_t bad[256];
        Table() { memset(bad, 1, sizeof(bad)); for (const char* c = "ACGTacgt"; *c; ++c) bad[(uint8_t)*c] = 0; }
    } t;
    size_t i = 0;
#if defined(__SSE2__)
    // sixteen bytes at a time (SSE2, part of every x86-64): fold the case bit away, then a byte is fine iff it equals one
    // of A C G T (a byte >= 0x80 keeps its top bit and equals none of them)
    const __m128i fold = _mm_set1_epi8((char)0xdf), cA = _mm_set1_epi8('A'), cC = _mm_set1_epi8('C'), cG = _mm_set1_epi8('G'),
                  cT = _mm_set1_epi8('T');
    for (; i + 16 <= len; i += 16) {
        const __m128i x = _mm_and_si128(_mm_loadu_si128(reinterpret_cast<const __m128i*>(seq + i)), fold);
        const __m128i ok = _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(x, cA), _mm_cmpeq_epi8(x, cC)),
                                        _mm_or_si128(_mm_cmpeq_epi8(x, cG), _mm_cmpeq_epi8(x, cT)));
        const unsigned m = (unsigned)_mm_movemask_epi8(ok);
        if (m != 0xffffu) return i + (size_t)__builtin_ctz(~m & 0xffffu);
    }
#endif
    for (; i < len; ++i)
        if (t.bad[seq[i]]) return i;
    return SIZE_MAX;
}

// What add_sequence queues of a record and whether it raises afterwards (signature.rs:38-58 + :246-306).  force == false: the
// walk is streaming in the reference, so every k-mer before the first one that covers an invalid byte is added before InvalidDNA
// is raised: the valid prefix seq[0, use_len) is queued, then the error names the k-mer at bad_kmer.  force == true: the whole
// record is queued and the kernel skips the bad k-mers.  The caller has ensured len >= k > 0.
// `scanned`: the caller has run first_invalid_byte over seq[0, len) already and passes its result in `first_bad`.
struct ValidPrefix {
    size_t use_len;
    bool raise;
    size_t bad_kmer;
};
inline ValidPrefix valid_prefix(const uint8_t* seq, size_t len, size_t k, bool force, bool scanned = false, size_t first_bad = SIZE_MAX) {
    ValidPrefix v{len, false, 0};
    if (!force) {
        const size_t p = scanned ? first_bad : first_invalid_byte(seq, len);
        if (p != SIZE_MAX) {
            v.bad_kmer = p + 1 >= k ? p + 1 - k : 0;                // first k-mer whose window covers byte p
            if (v.bad_kmer < len - k + 1) {
                v.raise = true;
                v.use_len = v.bad_kmer + k - 1;                     // k-mers 0 .. bad_kmer-1 only
            }
        }
    }
    return v;
}

// seq[0, use_len) and a '\n' (records never share a k-mer) onto the queue, if it holds a k-mer at all.  -> the queue is due for a
// settle from inside the add_sequence loop
inline bool queue_record(std::string& pending, const uint8_t* seq, size_t use_len, size_t k) {
    if (use_len < k) return false;
    pending.append((const char*)seq, use_len);
    pending.push_back('\n');
    return pending.size() >= PENDING_FLUSH_BYTES;
}

// The queue after a settle.  A flush from inside the add_sequence loop (`streaming`) keeps the queue's storage (a fresh 32 MiB
// string per flush costs 8,192 page faults, which was a fifth of the per-record time of a loop over 150-bp reads); a flush
// because somebody looks at the container gives storage beyond 1 MiB back, or every sketch of a many-ksize signature would hold
// a copy of its longest record for life.
inline void release_queue(std::string& pending, bool streaming) {
    if (streaming || pending.capacity() <= PENDING_KEEP_BYTES) pending.clear();
    else std::string().swap(pending);
}

}  // namespace smg
#pragma GCC visibility pop
