// Host-side Nodegraph behind the opaque `SourmashNodegraph*` handle.
//
// The khmer-compatible Bloom filter of src/core/src/sketch/nodegraph.rs: n tables of prime sizes, each a bitset; a hash h
// sets bit h mod size in every table.  `occupied` counts the bits of table 0 that went from 0 to 1.  The file format is
// khmer's ("OXLI", version 4, type 2).
//
// Bitsets use fixedbitset's layout: bit b is bit (b & 31) of u32 word (b >> 5).  All tables share one word array (`words`,
// table t from word offs[t]) so that the device mirror is one block.  A table of `size` bits holds (size / 8 + 4) / 4 words:
// the file stores size / 8 + 1 bytes of each table, and this is the number of words those bytes need (never fewer than
// ceil(size / 32)).
//
// Nothing here touches the device: capi_nodegraph.cpp keeps the device mirror and runs the kernels of nodegraph.hip.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>
#include "nodegraph_core.hpp"
#include "smg_errors.hpp"

namespace smg {

// deterministic Miller-Rabin: the first twelve primes as bases decide every n < 3.3e24, so every u64
inline uint64_t ng_mulmod(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((unsigned __int128)a * b % m); }
inline uint64_t ng_powmod(uint64_t a, uint64_t e, uint64_t m) {
    uint64_t r = 1 % m;
    a %= m;
    for (; e; e >>= 1, a = ng_mulmod(a, a, m))
        if (e & 1) r = ng_mulmod(r, a, m);
    return r;
}
inline bool ng_is_prime(uint64_t n) {
    static const uint64_t bases[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
    if (n < 2) return false;
    for (uint64_t p : bases) {
        if (n % p == 0) return n == p;
    }
    uint64_t d = n - 1;
    int s = 0;
    while ((d & 1) == 0) { d >>= 1; ++s; }
    for (uint64_t a : bases) {
        uint64_t x = ng_powmod(a, d, n);
        if (x == 1 || x == n - 1) continue;
        bool composite = true;
        for (int r = 1; r < s; ++r) {
            x = ng_mulmod(x, x, n);
            if (x == n - 1) { composite = false; break; }
        }
        if (composite) return false;
    }
    return true;
}

// Nodegraph::with_tables: from max(starting_size - 1, 2), made odd, down in steps of 2, keeping primes, until n_tables
// are kept or 1 has been tested.  starting_size == 0 underflows in the reference; here it is an error.
inline std::vector<uint64_t> ng_table_sizes(uint64_t starting_size, uint64_t n_tables) {
    if (starting_size == 0) throw Error(E_MSG, "Nodegraph starting_size must be at least 1");
    std::vector<uint64_t> sizes;
    uint64_t i = std::max<uint64_t>(starting_size - 1, 2);
    if (i % 2 == 0) i -= 1;
    while (sizes.size() != n_tables) {
        if (ng_is_prime(i)) sizes.push_back(i);
        if (i == 1) break;
        i -= 2;
    }
    return sizes;
}

// khmer's two-bit hash of a k-mer of any length (nodegraph.rs `_hash`): forward word over the codes left to right, reverse
// word over the complement codes right to left, both shifted left by 2 per base in 64 bits; the smaller one.  Strict: only
// upper-case A/C/G/T (the reference aborts on anything else; here it is InvalidDNA and nothing is counted).
inline uint64_t ng_twobit_hash(const uint8_t* s, size_t n) {
    if (n == 0) throw Error(E_INVALID_DNA, "invalid DNA character in input k-mer: (empty k-mer)");
    uint64_t fw = 0, rv = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t c = s[i];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T') throw err_invalid_dna(std::string((const char*)s, n));
        bool ok;
        fw = (fw << 2) | ng_code(c, &ok);
        rv = (rv << 2) | (ng_code(s[n - 1 - i], &ok) ^ 1u);
    }
    return fw < rv ? fw : rv;
}

struct Nodegraph {
    std::vector<uint64_t> sizes;        // bits per table
    std::vector<uint64_t> offs;         // first word of each table in `words`
    std::vector<uint32_t> words;
    size_t ksize = 0;
    uint64_t occupied = 0;
    // content generation: bumped by every host change of the tables or `occupied` (capi_nodegraph.cpp uploads the device mirror only
    // when it holds an older generation)
    uint64_t gen = 0;
    // DNA records handed to add_sequence and not counted yet, each followed by a '\n' (no k-mer spans it): capi_nodegraph.cpp runs them
    // through the k-mer kernel in one launch when the queue is large or when anything reads the tables
    std::string pending;
    std::recursive_mutex settle_mu;

    Nodegraph() = default;              // nodegraph_new: ksize 0, no tables
    Nodegraph(const Nodegraph&) = delete;
    Nodegraph& operator=(const Nodegraph&) = delete;

    static uint64_t n_words(uint64_t size) { return (size / 8 + 4) / 4; }

    // lay out tables of the given sizes, all bits clear
    void layout(const std::vector<uint64_t>& sz) {
        uint64_t total = 0;
        std::vector<uint64_t> o;
        for (uint64_t s : sz) {
            o.push_back(total);
            const uint64_t w = n_words(s);
            if (w > (((uint64_t)1 << 62) - total) / 4) throw Error(E_MSG, "Nodegraph table too large to allocate");
            total += w;
        }
        try {
            std::vector<uint32_t>((size_t)total, 0u).swap(words);
        } catch (const std::bad_alloc&) {
            throw Error(E_MSG, "Nodegraph table too large to allocate (" + std::to_string(total * 4) + " bytes)");
        } catch (const std::length_error&) {
            throw Error(E_MSG, "Nodegraph table too large to allocate (" + std::to_string(total * 4) + " bytes)");
        }
        sizes = sz;
        offs = o;
        ++gen;
    }
    void with_tables(size_t k, uint64_t starting_size, uint64_t n_tables) {
        const std::vector<uint64_t> sz = ng_table_sizes(starting_size, n_tables);
        layout(sz);
        ksize = k;
        occupied = 0;
    }

    size_t n_tables() const { return sizes.size(); }
    uint32_t* table(size_t t) { return words.data() + offs[t]; }
    const uint32_t* table(size_t t) const { return words.data() + offs[t]; }
    void check_size(size_t t) const {
        if (sizes[t] == 0) throw Error(E_MSG, "Nodegraph table " + std::to_string(t) + " has size 0");
    }

    bool count(uint64_t h) {
        bool is_new = false;
        for (size_t t = 0; t < sizes.size(); ++t) {
            check_size(t);
            const uint64_t b = h % sizes[t];
            uint32_t& w = table(t)[b >> 5];
            const uint32_t bit = 1u << (b & 31);
            if (!(w & bit)) {
                w |= bit;
                if (t == 0) ++occupied;
                is_new = true;
            }
        }
        ++gen;
        return is_new;
    }
    size_t get(uint64_t h) const {
        for (size_t t = 0; t < sizes.size(); ++t) {
            check_size(t);
            const uint64_t b = h % sizes[t];
            if (!((table(t)[b >> 5] >> (b & 31)) & 1u)) return 0;
        }
        return 1;
    }

    double expected_collisions() const {
#pragma clang fp contract(off)
        if (sizes.empty()) throw Error(E_MSG, "Nodegraph without tables has no expected collision rate");
        const uint64_t min_size = *std::min_element(sizes.begin(), sizes.end());
        const double fp_one = (double)occupied / (double)min_size;
        return pow(fp_one, (double)sizes.size());
    }

    // set bits of table t within its length
    uint64_t popcount(size_t t) const {
        const uint32_t* w = table(t);
        const uint64_t full = sizes[t] >> 5;
        uint64_t n = 0;
        for (uint64_t i = 0; i < full; ++i) n += (uint64_t)__builtin_popcount(w[i]);
        if (sizes[t] & 31) n += (uint64_t)__builtin_popcount(w[full] & ((1u << (sizes[t] & 31)) - 1u));
        return n;
    }
    // bits set in both tables within both lengths (fixedbitset intersection().count()), and in either (union().count())
    static void pair_counts(const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb, uint64_t* inter, uint64_t* uni) {
        auto word = [](const uint32_t* w, uint64_t n, uint64_t i) -> uint32_t {
            if (i >= (n + 31) / 32) return 0;
            const uint32_t v = w[i];
            if ((i + 1) * 32 <= n) return v;
            return v & ((1u << (n & 31)) - 1u);
        };
        const uint64_t nw = (std::max(na, nb) + 31) / 32;
        uint64_t in = 0, un = 0;
        for (uint64_t i = 0; i < nw; ++i) {
            const uint32_t x = word(a, na, i), y = word(b, nb, i);
            in += (uint64_t)__builtin_popcount(x & y);
            un += (uint64_t)__builtin_popcount(x | y);
        }
        *inter = in;
        *uni = un;
    }
    double similarity(const Nodegraph& o) const {
        uint64_t in = 0, un = 0;
        for (size_t t = 0; t < std::min(n_tables(), o.n_tables()); ++t) {
            uint64_t i1, u1;
            pair_counts(table(t), sizes[t], o.table(t), o.sizes[t], &i1, &u1);
            in += i1;
            un += u1;
        }
        return (double)in / (double)un;
    }
    double containment(const Nodegraph& o) const {
        uint64_t in = 0, own = 0;
        for (size_t t = 0; t < std::min(n_tables(), o.n_tables()); ++t) {
            uint64_t i1, u1;
            pair_counts(table(t), sizes[t], o.table(t), o.sizes[t], &i1, &u1);
            in += i1;
        }
        for (size_t t = 0; t < n_tables(); ++t) own += popcount(t);
        return (double)in / (double)own;
    }

    // Update<Nodegraph> for Nodegraph: union of the zipped tables (a table grows to the other's length when that is
    // longer, as fixedbitset's union_with does), then occupied = popcount(table 0) (0 when nothing was zipped)
    void update(const Nodegraph& o) {
        const size_t nz = std::min(n_tables(), o.n_tables());
        bool grow = false;
        for (size_t t = 0; t < nz; ++t) grow |= o.sizes[t] > sizes[t];
        if (grow) {
            std::vector<uint64_t> sz = sizes;
            for (size_t t = 0; t < nz; ++t) sz[t] = std::max(sz[t], o.sizes[t]);
            std::vector<uint32_t> old;
            old.swap(words);
            const std::vector<uint64_t> old_offs = offs, old_sizes = sizes;
            layout(sz);
            for (size_t t = 0; t < sz.size(); ++t)
                memcpy(table(t), old.data() + old_offs[t], (size_t)n_words(old_sizes[t]) * 4);
        }
        for (size_t t = 0; t < nz; ++t) {
            uint32_t* a = table(t);
            const uint32_t* b = o.table(t);
            const uint64_t nw = n_words(o.sizes[t]);
            for (uint64_t i = 0; i < nw; ++i) a[i] |= b[i];
        }
        occupied = nz ? popcount(0) : 0;
        ++gen;
    }

    // khmer's file layout
    std::string serialize() const {
        std::string s("OXLI");
        auto put = [&s](uint64_t v, int n) { for (int i = 0; i < n; ++i) s.push_back((char)(uint8_t)(v >> (8 * i))); };
        put(4, 1);
        put(2, 1);
        put((uint32_t)ksize, 4);
        put((uint8_t)sizes.size(), 1);
        put(occupied, 8);
        size_t total = s.size();
        for (uint64_t sz : sizes) total += 8 + (size_t)(sz / 8 + 1);
        s.reserve(total);
        for (size_t t = 0; t < sizes.size(); ++t) {
            put(sizes[t], 8);
            s.append((const char*)table(t), (size_t)(sizes[t] / 8 + 1));   // little-endian host: the words' bytes in order
        }
        return s;
    }
    // `data` is the plain (inflated) stream
    void parse(const uint8_t* data, size_t len) {
        size_t pos = 0;
        auto need = [&](size_t n) {
            if (len - pos < n) throw Error(E_IO, "failed to fill whole buffer");
        };
        auto get = [&](int n) {
            need((size_t)n);
            uint64_t v = 0;
            for (int i = 0; i < n; ++i) v |= (uint64_t)data[pos + i] << (8 * i);
            pos += (size_t)n;
            return v;
        };
        need(4);
        if (memcmp(data, "OXLI", 4) != 0) throw Error(E_IO, "not a nodegraph file (bad signature)");
        pos = 4;
        const uint64_t version = get(1);
        if (version != 4) throw Error(E_IO, "unsupported nodegraph file version " + std::to_string(version));
        const uint64_t ht_type = get(1);
        if (ht_type != 2) throw Error(E_IO, "not a nodegraph file (table type " + std::to_string(ht_type) + ")");
        const size_t k = (size_t)get(4);
        const uint64_t nt = get(1);
        const uint64_t occ = get(8);
        std::vector<uint64_t> sz;
        std::vector<size_t> at;
        for (uint64_t t = 0; t < nt; ++t) {
            const uint64_t s = get(8);
            if (s / 8 + 1 > len - pos) throw Error(E_IO, "failed to fill whole buffer");
            sz.push_back(s);
            at.push_back(pos);
            pos += (size_t)(s / 8 + 1);
        }
        layout(sz);
        for (size_t t = 0; t < sz.size(); ++t) memcpy(table(t), data + at[t], (size_t)(sz[t] / 8 + 1));
        ksize = k;
        occupied = occ;
    }
};

}  // namespace smg
