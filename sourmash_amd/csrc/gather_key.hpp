// gather_key.hpp -- part of gather_api.hpp in plain C++ (tests/native/slice_walk_emul.cpp checks it with g++): a round's pick as one
// u64 whose maximum is the reference's choice -- largest remaining overlap, ties to the dataset inserted first -- and the stop rule.
#pragma once
#include <stdint.h>
#include "qindex_core.hpp"          // SMG_HD

namespace smg {

// counts and indices are below 2^32; 0 is "nothing"
SMG_HD unsigned long long gather_key(unsigned long long count, unsigned long long global_index) {
    return (count << 32) | (0xffffffffull & ~global_index);
}
SMG_HD uint64_t gather_key_index(unsigned long long key) { return 0xffffffffull & ~key; }

// search.py:15-37 + index/__init__.py:825-861: the rounds stop when nothing overlaps, the query is exhausted, the threshold is
// unattainable (more hashes than the query has left) or the best overlap is below it
SMG_HD bool gather_stops(unsigned long long key, unsigned long long qlen, unsigned long long thr) {
    return key == 0 || qlen == 0 || qlen < thr || (key >> 32) < thr;
}

}  // namespace smg
