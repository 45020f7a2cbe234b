// Host checks of the limb-wise 64-bit constant multiply of MurmurHash3 (sourmash_amd/csrc/murmur3.hpp, mul_c64): the same limbs
// the kernels run, compiled for the CPU (test-only artefact).  tests/test_mul_c64_cpu.py drives it.
#include <cstring>
#include "../../sourmash_amd/csrc/murmur3.hpp"

// The constants of murmur3.hpp: the four multipliers of the hash and the two addends of its block step (never multiplied by in
// the hash, here as two more bit patterns with an all-zero top limb).
static constexpr uint64_t CONSTS[6] = {smg::MMH3_C1, smg::MMH3_C2, smg::FMIX_C1, smg::FMIX_C2, 0x52dce729ULL, 0x38495ab5ULL};

template <int I>
static uint64_t limb(uint64_t x) { return smg::mul_c64<CONSTS[I]>(x); }
template <int I>
static uint64_t plain(uint64_t x) { return smg::mul_c64<CONSTS[I], true>(x); }

extern "C" int emul_n_consts() { return 6; }
extern "C" uint64_t emul_const(int i) { return CONSTS[i]; }

// limb form and plain form of x * CONSTS[i]
extern "C" int emul_mul_c64(int i, uint64_t x, uint64_t* by_limbs, uint64_t* by_plain) {
    switch (i) {
    case 0: *by_limbs = limb<0>(x); *by_plain = plain<0>(x); return 0;
    case 1: *by_limbs = limb<1>(x); *by_plain = plain<1>(x); return 0;
    case 2: *by_limbs = limb<2>(x); *by_plain = plain<2>(x); return 0;
    case 3: *by_limbs = limb<3>(x); *by_plain = plain<3>(x); return 0;
    case 4: *by_limbs = limb<4>(x); *by_plain = plain<4>(x); return 0;
    case 5: *by_limbs = limb<5>(x); *by_plain = plain<5>(x); return 0;
    }
    return 1;
}

static uint64_t splitmix(uint64_t& x) {
    x += 0x9e3779b97f4a7c15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

// n pseudo-random x (every 5th with its low limb all ones, every 5th + 2 with its high limb all ones): the number of
// (x, constant) pairs whose limb form differs from x * c, c as a run-time value
extern "C" uint64_t emul_sweep_violations(uint64_t n, uint64_t seed) {
    uint64_t bad = 0, s = seed;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t x = splitmix(s);
        if (i % 5 == 0) x |= 0xffffffffULL;
        if (i % 5 == 2) x |= 0xffffffff00000000ULL;
        uint64_t a, b;
        for (int c = 0; c < 6; ++c) {
            emul_mul_c64(c, x, &a, &b);
            volatile uint64_t k = CONSTS[c];
            const uint64_t want = x * k;
            bad += (a != want) + (b != want);
        }
    }
    return bad;
}

// fmix64 and its two halves against the textbook form
extern "C" uint64_t emul_fmix_violations(uint64_t n, uint64_t seed) {
    uint64_t bad = 0, s = seed;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t x = i < 4 ? (i == 0 ? 0 : i == 1 ? 1 : i == 2 ? ~0ULL : 1ULL << 63) : splitmix(s);
        volatile uint64_t c1 = 0xff51afd7ed558ccdULL, c2 = 0xc4ceb9fe1a85ec53ULL;
        uint64_t k = x;
        k ^= k >> 33; k *= c1; k ^= k >> 33; k *= c2; k ^= k >> 33;
        bad += smg::fmix64(x) != k;
        bad += smg::fmix64<true>(x) != k;
        bad += smg::fmix64_tail(smg::fmix64_head(x)) != k;
        bad += (uint32_t)(smg::fmix64_tail(x) >> 32) != smg::fmix64_tail_hi(x);
    }
    return bad;
}

// mmh3_h1_words<K>, limb form and plain form, and mmh3_h1_bytes on the same k bytes
template <int K>
static void words(const uint8_t* key, uint64_t seed, uint64_t* out) {
    uint32_t w[(K + 3) / 4] = {};
    std::memcpy(w, key, K);
    out[0] = smg::mmh3_h1_words<K>(w, seed);
    out[1] = smg::mmh3_h1_words<K, true>(w, seed);
}
extern "C" int emul_h1_forms(const uint8_t* key, uint32_t k, uint64_t seed, uint64_t* out3) {
    out3[2] = smg::mmh3_h1_bytes(key, k, seed);
    switch (k) {
#define CASE(K) case K: words<K>(key, seed, out3); return 0;
    CASE(1) CASE(7) CASE(8) CASE(9) CASE(15) CASE(16) CASE(17) CASE(21) CASE(24) CASE(25) CASE(31) CASE(32) CASE(33) CASE(47) CASE(48)
    CASE(51) CASE(63) CASE(64) CASE(65) CASE(88) CASE(89) CASE(128)
#undef CASE
    }
    return 1;
}
