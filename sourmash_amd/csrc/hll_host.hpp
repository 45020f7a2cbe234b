// Host-side HyperLogLog behind the opaque `SourmashHyperLogLog*` handle.
//
// The distinct-k-mer counter of src/core/src/sketch/hyperloglog/{mod.rs,estimators.rs}: 2^p one-byte registers, each the
// largest "rank" (leading zeros of the hash's upper 64 - p bits, plus one) seen among the hashes whose low p bits select it,
// and Ertl's maximum-likelihood estimators (cardinality, and the joint estimate of |A - B|, |B - A|, |A n B|).
//
// Written from the algorithm.  The estimators perform the same floating-point operations in the same order as the
// reference, with the same libm calls, so they return the same f64 bits; every f64 -> size_t conversion saturates (negative
// or NaN -> 0, too large -> SIZE_MAX), which is what Rust's `as usize` does and what a plain C++ cast leaves undefined.
//
// Nothing here touches the device: k-mers are hashed into the registers by hll.hip (capi_hll.cpp queues the records first).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>
#include "smg_errors.hpp"

namespace smg {

// Rust's `f as usize`
inline size_t sat_usize(double x) {
    if (!(x > 0.0)) return 0;                                   // negative, zero, NaN
    if (x >= 18446744073709551616.0) return SIZE_MAX;          // 2^64 and above, +inf
    return (size_t)x;
}

// Rust's `f as i32` (only used where the reference converts a usize with `as i32`: truncation to the low 32 bits)
inline int32_t trunc_i32(uint64_t v) { return (int32_t)(uint32_t)v; }

// 2^n for the small integer n the estimators use: exact, as f64::powi(2.0, n) is for every such n
inline double pow2i(int32_t n) { return ldexp(1.0, n); }

// estimators.rs `mle`: counts[0 .. q+2), counts[i] = registers holding i.  `m` = 2^p.
inline double hll_mle(const std::vector<uint64_t>& counts, size_t p, size_t q, double relerr) {
#pragma clang fp contract(off)
    const uint64_t m = (uint64_t)1 << p;
    if (counts[0] == m) return 0.0;
    if (counts[q + 1] == m) return INFINITY;
    size_t k_min = 0;
    while (k_min < counts.size() && counts[k_min] == 0) ++k_min;
    size_t k_max = counts.size() - 1;
    while (k_max > 0 && counts[k_max] == 0) --k_max;
    const size_t k_min_prime = std::max<size_t>(1, k_min);
    const size_t k_max_prime = std::min(q, k_max);

    double z = 0.0;
    for (int32_t i = trunc_i32(k_max_prime); i >= trunc_i32(k_min_prime); --i) z = 0.5 * z + (double)counts[(size_t)i];
    z *= pow2i(-trunc_i32(k_min_prime));

    uint64_t c_prime = counts[q + 1];
    if (q >= 1) c_prime += counts[k_max_prime];

    double g_prev = 0.0;
    const double a = z + (double)counts[0];
    const double b = z + (double)counts[q + 1] * pow2i(-trunc_i32(q));
    const double m_prime = (double)(m - counts[0]);

    double x = b <= 1.5 * a ? m_prime / (0.5 * b + a)            // weak lower bound
                            : m_prime / (b * log(1.0 + b / a));  // strong lower bound
    double delta_x = x;
    const double del = relerr / sqrt((double)m);
    while (delta_x > x * del) {
        // secant iteration
        const size_t kappa = sat_usize(2.0 + floor(log2(x)));
        double x_prime = x * pow2i(-trunc_i32(std::max(k_max_prime, kappa)) - 1);
        const double x_pp = x_prime * x_prime;
        double h = x_prime - (x_pp / 3.0) + (x_pp * x_pp) * (1.0 / 45.0 - x_pp / 472.5);   // Taylor approximation
        for (int32_t k = trunc_i32(kappa) - 1; k >= trunc_i32(k_max_prime); --k) {
            const double h_prime = 1.0 - h;
            h = (x_prime + h * h_prime) / (x_prime + h_prime);
            x_prime += x_prime;
        }
        double g = (double)c_prime * h;
        for (int32_t k = trunc_i32(k_max_prime) - 1; k >= trunc_i32(k_min_prime); --k) {
            const double h_prime = 1.0 - h;
            h = (x_prime + h * h_prime) / (x_prime + h_prime);
            g += (double)counts[(size_t)k] * h;
            x_prime += x_prime;
        }
        g += x * a;
        delta_x = ((g > g_prev) | (m_prime >= g)) ? delta_x * (m_prime - g) / (g - g_prev) : 0.0;
        x += delta_x;
        g_prev = g;
    }
    return (double)m * x;
}

struct JointMle { size_t only_a, only_b, common; };

// estimators.rs `joint_mle`: the registers are zipped (the shorter length wins), p and q are the first sketch's
inline JointMle hll_joint_mle(const uint8_t* k1, size_t n1, const uint8_t* k2, size_t n2, size_t p, size_t q) {
#pragma clang fp contract(off)
    const size_t n = std::min(n1, n2);
    std::vector<uint64_t> c1(q + 2), c2(q + 2), cu(q + 2), cg1(q + 2), cg2(q + 2), ceq(q + 2);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t a = k1[i], b = k2[i];
        if (a < b) { c1[a]++; cg2[b]++; }
        else if (a > b) { cg1[a]++; c2[b]++; }
        else ceq[a]++;
        cu[std::max(a, b)]++;
    }
    for (size_t i = 0; i < q + 2; ++i) { c1[i] += cg1[i] + ceq[i]; c2[i] += cg2[i] + ceq[i]; }
    const double c_ax = hll_mle(c1, p, q, 0.01);
    const double c_bx = hll_mle(c2, p, q, 0.01);
    const double c_abx = hll_mle(cu, p, q, 0.01);
    std::vector<uint64_t> axb(q + 2), bxa(q + 2);
    axb[q] = n1;
    bxa[q] = n2;
    for (size_t i = 0; i < q; ++i) {
        axb[i] = cg1[i] + ceq[i] + cg2[i + 1];
        axb[q] -= axb[i];
        bxa[i] = cg2[i] + ceq[i] + cg1[i + 1];
        bxa[q] -= bxa[i];
    }
    const double c_axb_half = hll_mle(axb, p, q - 1, 0.01);
    const double c_bxa_half = hll_mle(bxa, p, q - 1, 0.01);
    const double cx1 = 1.5 * c_bx + 1.5 * c_ax - c_bxa_half - c_axb_half;
    const double cx2 = 2.0 * (c_bxa_half + c_axb_half) - 3.0 * c_abx;
    return JointMle{sat_usize(c_abx - c_bx), sat_usize(c_abx - c_ax), sat_usize(0.5 * (cx1 + cx2))};
}

struct HyperLogLog {
    std::vector<uint8_t> registers;
    size_t p = 0, q = 0, ksize = 0;
    // DNA records handed to add_sequence and not hashed yet, each followed by a '\n' (no k-mer spans it): capi_hll.cpp runs them
    // through the HLL kernel in one launch when the queue is large or when anything reads the registers
    std::string pending;
    std::recursive_mutex settle_mu;     // settling a handle's queue is serialised (two readers on two threads)

    HyperLogLog() = default;            // the reference's Default: p = 0, no registers
    HyperLogLog(const HyperLogLog& o) : registers(o.registers), p(o.p), q(o.q), ksize(o.ksize), pending(o.pending) {}

    static HyperLogLog make(size_t p, size_t ksize) {
        if (p < 4 || p > 18) throw Error(E_HLL_PRECISION_BOUNDS, "HLL precision must be between 4 and 18");
        HyperLogLog h;
        h.p = p;
        h.q = 64 - p;
        h.ksize = ksize;
        h.registers.assign((size_t)1 << p, 0);
        return h;
    }
    // p = ceil(log2((1.04 / e)^2)), then the bounds check of make()
    static size_t precision_for(double error_rate) {
        const double r = 1.04 / error_rate;
        return sat_usize(ceil(log2(r * r)));
    }

    void add_hash(uint64_t h) {
        if (registers.empty()) throw err_internal("HyperLogLog without registers (made by hll_new)");
        const uint64_t value = h >> p;
        const size_t idx = (size_t)(h & (((uint64_t)1 << p) - 1));
        const uint32_t rank = (value ? (uint32_t)__builtin_clzll(value) : 64u) + 1u - (uint32_t)p;
        if (registers[idx] < rank) registers[idx] = (uint8_t)rank;
    }

    void check_compatible(const HyperLogLog& o) const {
        if (ksize != o.ksize) throw err_mismatch_ksizes();
        if (registers.size() != o.registers.size())
            throw Error(E_MISMATCH_NUM, "num mismatch: " + std::to_string((uint32_t)registers.size()) + " != " +
                                            std::to_string((uint32_t)o.registers.size()));
    }
    void merge(const HyperLogLog& o) {
        check_compatible(o);
        for (size_t i = 0; i < registers.size(); ++i) registers[i] = std::max(registers[i], o.registers[i]);
    }
    void merge_registers(const uint8_t* r, size_t n) {
        for (size_t i = 0; i < n && i < registers.size(); ++i) registers[i] = std::max(registers[i], r[i]);
    }

    size_t cardinality() const {
        if (registers.empty()) throw err_internal("HyperLogLog without registers (made by hll_new)");
        std::vector<uint64_t> counts(q + 2);
        for (uint8_t r : registers) {
            if ((size_t)r >= counts.size()) throw err_internal("HyperLogLog register out of range");
            counts[r]++;
        }
        const double relerr = p < 8 ? 0.01 : p < 16 ? 0.05 : 0.1;
        return sat_usize(hll_mle(counts, p, q, relerr));
    }
    JointMle joint(const HyperLogLog& o) const {
        if (registers.empty() || q < 1) throw err_internal("HyperLogLog without registers (made by hll_new)");
        for (const auto* v : {&registers, &o.registers})
            for (uint8_t r : *v)
                if ((size_t)r > q + 1) throw err_internal("HyperLogLog register out of range");
        return hll_joint_mle(registers.data(), registers.size(), o.registers.data(), o.registers.size(), p, q);
    }
    double similarity(const HyperLogLog& o) const {
        const JointMle j = joint(o);
        return (double)j.common / (double)(j.only_a + j.only_b + j.common);
    }
    double containment(const HyperLogLog& o) const {
        const JointMle j = joint(o);
        return (double)j.common / (double)(j.only_a + j.common);
    }
    size_t intersection(const HyperLogLog& o) const { return joint(o).common; }

    // "HLL", version 1, p, q, ksize (one byte each, truncated), the registers
    std::string serialize() const {
        std::string s("HLL");
        s.push_back(1);
        s.push_back((char)(uint8_t)p);
        s.push_back((char)(uint8_t)q);
        s.push_back((char)(uint8_t)ksize);
        s.append((const char*)registers.data(), registers.size());
        return s;
    }
    // `data` is the plain (inflated) stream
    static HyperLogLog parse(const uint8_t* data, size_t len) {
        if (len < 7 || memcmp(data, "HLL", 3) != 0) throw Error(E_IO, "not a HyperLogLog file (bad magic)");
        if (data[3] != 1) throw Error(E_IO, "unsupported HyperLogLog version " + std::to_string(data[3]));
        HyperLogLog h;
        h.p = data[4];
        h.q = data[5];
        h.ksize = data[6];
        if (h.p > 63) throw Error(E_IO, "HyperLogLog precision out of range");
        const size_t n = (size_t)1 << h.p;
        if (len - 7 < n) throw Error(E_IO, "failed to fill whole buffer");
        h.registers.assign(data + 7, data + 7 + n);
        return h;
    }
};

}  // namespace smg
