// Host checks of the sketch kernel's early reject on ONE product and of the seed folded into MurmurHash3's first block
// (test-only artefact; compiles sourmash_amd/csrc/kmer_core.hpp and murmur3.hpp for the CPU).
// tests/test_early_reject_sum_cpu.py drives it.
#include <cstring>
#include <utility>
#include "../../sourmash_amd/csrc/kmer_core.hpp"

static uint64_t splitmix(uint64_t& x) {
    x += 0x9e3779b97f4a7c15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

// n pseudo-random open pairs (every 7th: the two fmix64 inputs sum to 0; every 7th + 3: a + b == 0 itself, the product that
// wraps): counts[d + 1] += 1 for d = t - s in {-1, 0, +1} (mod 2^32), t the true top dword and s the estimate of
// mmh3_close_hi_sum.  Returns the number of pairs with any other d.
extern "C" uint64_t emul_sum_form_violations(uint64_t n, uint64_t seed, uint64_t* counts) {
    uint64_t bad = 0, x = seed;
    counts[0] = counts[1] = counts[2] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t h1 = splitmix(x), h2 = splitmix(x);
        if (i % 7 == 0) h2 = (uint64_t)0 - h1;
        smg::Mmh3Open o{smg::fmix64_head(h1), smg::fmix64_head(h2)};
        if (i % 7 == 3) o.b = (uint64_t)0 - o.a;
        const uint32_t t = (uint32_t)(smg::mmh3_close(o) >> 32), s = smg::mmh3_close_hi_sum(o);
        const uint32_t d = t - s;
        if (d == 0xffffffffu) ++counts[0];
        else if (d == 0u) ++counts[1];
        else if (d == 1u) ++counts[2];
        else ++bad;
    }
    return bad;
}

// An open pair whose closed hash is exactly h: b is pseudo-random, a = fmix64_tail^-1(h - fmix64_tail(b)).
static smg::Mmh3Open open_for(uint64_t h, uint64_t& x) {
    const uint64_t c = 0xc4ceb9fe1a85ec53ULL;
    uint64_t inv = c;                                    // Newton: correct bits double each step (c is odd: 3 bits to start with)
    for (int i = 0; i < 6; ++i) inv *= 2 - c * inv;
    const uint64_t b = splitmix(x);
    const uint64_t y = h - smg::fmix64_tail(b);
    const uint64_t p = y ^ (y >> 33);                    // the xor-shift by 33 is its own inverse
    return smg::Mmh3Open{p * inv, b};
}

// For `reps` open pairs closing to h: 0 if every one closes to h and early_may_keep agrees with the keep rule wherever the rule
// keeps (h <= thr implies may_keep), else the number that do not.  *passed = how many the filter let through.
extern "C" uint64_t emul_filter_violations(uint64_t h, uint64_t thr, uint64_t reps, uint64_t seed, uint64_t* passed) {
    uint64_t bad = 0, x = seed;
    *passed = 0;
    const uint32_t lim = smg::early_limit(thr);
    for (uint64_t i = 0; i < reps; ++i) {
        const smg::Mmh3Open o = open_for(h, x);
        if (smg::mmh3_close(o) != h) { ++bad; continue; }
        const bool may = smg::early_may_keep(o, lim);
        if (may) ++*passed;
        if (h <= thr && !may) ++bad;
    }
    return bad;
}

// process_lane<31, 16> over a buffer as the kernel walks it (kmer_core_emul.cpp), early reject on or off
template <bool EARLY>
static uint64_t run31(const uint8_t* seq, uint64_t len, uint64_t seed, uint64_t thr, uint64_t* out, uint64_t cap) {
    using G = smg::LaneGeom<31, 16>;
    uint64_t n = 0;
    for (uint64_t start = 0; start < len; start += 16) {
        uint32_t raw[G::NW];
        uint8_t bytes[G::NW * 4];
        for (int b = 0; b < G::NW * 4; ++b) bytes[b] = (start + b < len) ? seq[start + b] : 0;
        for (int b = G::NBYTES; b < G::NW * 4; ++b) bytes[b] = (start + b < len) ? seq[start + b] : (uint8_t)'N';
        std::memcpy(raw, bytes, sizeof(raw));
        smg::process_lane<31, 16, EARLY>(raw, seed, thr, [&](int, uint64_t h) { if (n < cap) out[n] = h; ++n; });
    }
    return n;
}
extern "C" uint64_t emul_lane31(const uint8_t* seq, uint64_t len, uint64_t seed, uint64_t thr, uint64_t* out, uint64_t cap, int early) {
    return early ? run31<true>(seq, len, seed, thr, out, cap) : run31<false>(seq, len, seed, thr, out, cap);
}

// mmh3_h1_words<K> (first block with the seed folded in) and mmh3_h1_bytes on the same k bytes
template <int K>
static uint64_t words(const uint8_t* key, uint64_t seed) {
    uint32_t w[(K + 3) / 4] = {};
    std::memcpy(w, key, K);
    return smg::mmh3_h1_words<K>(w, seed);
}
extern "C" int emul_h1_pair(const uint8_t* key, uint32_t k, uint64_t seed, uint64_t* by_words, uint64_t* by_bytes) {
    *by_bytes = smg::mmh3_h1_bytes(key, k, seed);
    switch (k) {
    case 15: *by_words = words<15>(key, seed); return 0;
    case 16: *by_words = words<16>(key, seed); return 0;
    case 31: *by_words = words<31>(key, seed); return 0;
    case 32: *by_words = words<32>(key, seed); return 0;
    case 47: *by_words = words<47>(key, seed); return 0;
    }
    return 1;
}
