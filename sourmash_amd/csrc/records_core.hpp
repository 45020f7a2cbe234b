// records_core.hpp -- the rules of per-record sketching (sketch_records.hip) that the host and the device share: which
// record a k-mer belongs to -- for records that touch and for records with explicit ends -- and whether (record, hash) fits one
// 64-bit sort key.  Plain C++ on the host (tests/native/records_core_emul.cpp and residue_records_emul.cpp compile it with g++).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef SMG_HD
#if defined(__HIPCC__)
#define SMG_HD __host__ __device__ __forceinline__
#else
#define SMG_HD inline
#endif
#endif

namespace smg {

// Records are described by starts[0 .. n_records], ascending: record r is the bytes [starts[r], starts[r + 1]).
// The k-mer of k bytes that starts at pos belongs to r = upper_bound(starts, pos) - 1 -- the last record that starts at or
// before pos, so an empty record never owns a k-mer -- and is kept only if it lies inside that record: no k-mer spans two
// records, whatever byte (if any) separates them, and nothing in front of starts[0] or behind starts[n_records] counts.
SMG_HD bool rec_assign(const uint64_t* starts, uint64_t n_records, uint64_t pos, uint32_t k, uint64_t* rec) {
    if (n_records == 0 || pos < starts[0]) return false;
    uint64_t lo = 0, hi = n_records + 1;                 // first index with starts[index] > pos
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (starts[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    const uint64_t r = lo - 1;                           // lo >= 1: starts[0] <= pos
    if (r >= n_records) return false;                    // at or behind starts[n_records]
    if (pos + k > starts[r + 1]) return false;
    *rec = r;
    return true;
}

// Records with explicit ends: record r is the bytes [starts[r], ends[r]) with starts[r] <= ends[r] <= starts[r + 1]; a null `ends`
// means ends[r] = starts[r + 1] (records touch).  The bytes of [ends[r], starts[r + 1]) belong to no record -- the byte a file
// parser leaves between two records, which is no base but would be a residue.  The window of k bytes that starts at pos belongs
// to r = upper_bound(starts, pos) - 1, as above, and is kept only if it ends at or before ends[r].
SMG_HD uint64_t rec_end(const uint64_t* starts, const uint64_t* ends, uint64_t r) { return ends ? ends[r] : starts[r + 1]; }
SMG_HD uint64_t rec_len(const uint64_t* starts, const uint64_t* ends, uint64_t r) { return rec_end(starts, ends, r) - starts[r]; }
SMG_HD bool rec_ends_valid(const uint64_t* starts, const uint64_t* ends, uint64_t r) {
    return ends[r] >= starts[r] && ends[r] <= starts[r + 1];
}
SMG_HD bool rec_assign_ends(const uint64_t* starts, const uint64_t* ends, uint64_t n_records, uint64_t pos, uint32_t k, uint64_t* rec) {
    if (n_records == 0 || pos < starts[0]) return false;
    uint64_t lo = 0, hi = n_records + 1;                 // first index with starts[index] > pos
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (starts[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    const uint64_t r = lo - 1;                           // lo >= 1: starts[0] <= pos
    if (r >= n_records) return false;                    // at or behind starts[n_records]
    if (pos + k > rec_end(starts, ends, r)) return false;
    *rec = r;
    return true;
}

// significant bits of v (0 for 0)
SMG_HD int rec_bits(uint64_t v) {
    int b = 0;
    while (b < 64 && (v >> b)) ++b;
    return b;
}
// bits a kept hash needs: 1 <= h <= max_hash, max_hash == 0 keeps every hash
SMG_HD int rec_hash_bits(uint64_t max_hash) { return max_hash ? rec_bits(max_hash) : 64; }

// Packed form: the record number rides in the key bits above the hash (the packing of tag_gather, device_sort.hip) and one
// 64-bit sort + run-length encode orders every record's hashes.  It needs bits(n_records - 1) + hash bits <= 64; otherwise
// the wide form sorts (hash, record) pairs in two stable passes.  Key 0 is free in either form (a kept hash is >= 1): it marks
// the pairs the assign rule drops.
SMG_HD bool rec_packed(uint64_t n_records, uint64_t max_hash) {
    return rec_bits(n_records ? n_records - 1 : 0) + rec_hash_bits(max_hash) <= 64;
}

}  // namespace smg
