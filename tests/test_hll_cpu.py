"""HyperLogLog on the host (no GPU): precision from error rates, add_hash ranks, merge and its errors, the file and buffer
formats, and the estimators against an independent Python statement of Ertl's MLE (sketch/hyperloglog/estimators.rs) --
equal f64 bits and equal integers."""
import ctypes as C
import gzip
import math
import random
import struct

import pytest

import sourmash_amd as sm
from sourmash_amd._lowlevel import lib
from sourmash_amd.hll import HLL


# ---- the estimators, restated -----------------------------------------------------------------------------------------
def _usize(x):
    "Rust's `f64 as usize`"
    if not x > 0:
        return 0
    if x >= 2.0 ** 64:
        return 2 ** 64 - 1
    return int(x)


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def mle(counts, p, q, relerr):
    m = 1 << p
    if counts[0] == m:
        return 0.0
    if counts[q + 1] == m:
        return math.inf
    k_min = next(i for i, v in enumerate(counts) if v != 0)
    k_max = next(i for i in range(len(counts) - 1, -1, -1) if counts[i] != 0)
    kmin_p = max(1, k_min)
    kmax_p = min(q, k_max)
    z = 0.0
    for i in range(kmax_p, kmin_p - 1, -1):
        z = 0.5 * z + float(counts[i])
    z *= math.ldexp(1.0, -kmin_p)
    c_prime = counts[q + 1] + (counts[kmax_p] if q >= 1 else 0)
    g_prev = 0.0
    a = z + float(counts[0])
    b = z + float(counts[q + 1]) * math.ldexp(1.0, -q)
    m_prime = float(m - counts[0])
    x = m_prime / (0.5 * b + a) if b <= 1.5 * a else m_prime / (b * math.log(1.0 + b / a))
    delta_x = x
    dl = relerr / math.sqrt(float(m))
    while delta_x > x * dl:
        kappa = _usize(2.0 + math.floor(math.log2(x)))
        x_prime = x * math.ldexp(1.0, -_i32(max(kmax_p, kappa)) - 1)
        x_pp = x_prime * x_prime
        h = x_prime - (x_pp / 3.0) + (x_pp * x_pp) * (1.0 / 45.0 - x_pp / 472.5)
        for _ in range(_i32(kappa) - 1, kmax_p - 1, -1):
            hp = 1.0 - h
            h = (x_prime + h * hp) / (x_prime + hp)
            x_prime += x_prime
        g = float(c_prime) * h
        for k in range(kmax_p - 1, kmin_p - 1, -1):
            hp = 1.0 - h
            h = (x_prime + h * hp) / (x_prime + hp)
            g += float(counts[k]) * h
            x_prime += x_prime
        g += x * a
        delta_x = delta_x * (m_prime - g) / (g - g_prev) if (g > g_prev or m_prime >= g) else 0.0
        x += delta_x
        g_prev = g
    return float(m) * x


def cardinality(regs, p):
    q = 64 - p
    counts = [0] * (q + 2)
    for r in regs:
        counts[r] += 1
    return _usize(mle(counts, p, q, 0.01 if p < 8 else 0.05 if p < 16 else 0.1))


def joint_mle(k1, k2, p):
    q = 64 - p
    z = lambda: [0] * (q + 2)  # noqa: E731
    c1, c2, cu, cg1, cg2, ceq = z(), z(), z(), z(), z(), z()
    for a, b in zip(k1, k2):
        if a < b:
            c1[a] += 1
            cg2[b] += 1
        elif a > b:
            cg1[a] += 1
            c2[b] += 1
        else:
            ceq[a] += 1
        cu[max(a, b)] += 1
    for i in range(q + 2):
        c1[i] += cg1[i] + ceq[i]
        c2[i] += cg2[i] + ceq[i]
    c_ax, c_bx, c_abx = mle(c1, p, q, 0.01), mle(c2, p, q, 0.01), mle(cu, p, q, 0.01)
    axb, bxa = z(), z()
    axb[q], bxa[q] = len(k1), len(k2)
    for i in range(q):
        axb[i] = cg1[i] + ceq[i] + cg2[i + 1]
        axb[q] -= axb[i]
        bxa[i] = cg2[i] + ceq[i] + cg1[i + 1]
        bxa[q] -= bxa[i]
    c_axb_half = mle(axb, p, q - 1, 0.01)
    c_bxa_half = mle(bxa, p, q - 1, 0.01)
    cx1 = 1.5 * c_bx + 1.5 * c_ax - c_bxa_half - c_axb_half
    cx2 = 2.0 * (c_bxa_half + c_axb_half) - 3.0 * c_abx
    return _usize(c_abx - c_bx), _usize(c_abx - c_ax), _usize(0.5 * (cx1 + cx2))


def _bits(x):
    return struct.pack("<d", x)


def make(regs, p, ksize=21):
    "an HLL holding exactly these registers (through the file format)"
    return HLL.from_buffer(b"HLL" + bytes([1, p, 64 - p, ksize]) + bytes(regs))


def add_hash_py(regs, p, h):
    v = h >> p
    rank = (64 - v.bit_length()) + 1 - p
    i = h & ((1 << p) - 1)
    regs[i] = max(regs[i], rank)


# ---- construction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e,p", [(0.01, 14), (0.05, 9), (0.1, 7), (0.02, 12), (0.26, 4), (0.0025, 18)])
def test_precision_from_error_rate(e, p):
    h = HLL(e, 21)
    assert h.precision == p
    assert len(h.registers()) == 1 << p
    assert h.ksize == 21


@pytest.mark.parametrize("e", [0.5, 0.4, 0.002, 0.0001])
def test_precision_bounds(e):
    with pytest.raises(ValueError) as ei:
        HLL(e, 21)
    assert "precision" in str(ei.value)
    lib.sourmash_err_clear()
    assert not lib.hll_with_error_rate(e, 21)
    assert lib.sourmash_err_get_last_code() == 1301


def test_default_handle():
    p = lib.hll_new()
    assert p
    assert lib.hll_ksize(p) == 0
    lib.hll_free(p)


# ---- add_hash ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 10, 14, 18])
def test_add_hash_ranks(p):
    q = 64 - p
    h = HLL.from_buffer(b"HLL" + bytes([1, p, q, 21]) + bytes(1 << p))
    h.add(0)                                        # idx 0, rank q + 1
    regs = h.registers()
    assert regs[0] == q + 1
    top = (1 << 64) - 1
    h.add(top)                                      # idx 2^p - 1, rank 1
    assert h.registers()[(1 << p) - 1] == 1
    h.add(1 << p)                                   # value 1: rank q; idx 0 stays q + 1
    assert h.registers()[0] == q + 1
    h.add((1 << p) | 5)                             # idx 5, value 1 -> rank q
    assert h.registers()[5] == q
    h.add((1 << 63) | 7)                            # idx 7, top bit set -> rank 1
    assert h.registers()[7] == 1
    rng = random.Random(p)
    want = list(h.registers())
    for _ in range(3000):
        x = rng.getrandbits(64) >> rng.randrange(64)
        h.add(x)
        add_hash_py(want, p, x)
    assert list(h.registers()) == want


# ---- merge ------------------------------------------------------------------------------------------------------------
def test_merge():
    rng = random.Random(7)
    a = [rng.randrange(0, 52) for _ in range(1 << 12)]
    b = [rng.randrange(0, 52) for _ in range(1 << 12)]
    ha, hb = make(a, 12), make(b, 12)
    ha.update(hb)
    assert list(ha.registers()) == [max(x, y) for x, y in zip(a, b)]
    assert list(hb.registers()) == b
    with pytest.raises(Exception):
        ha.update(make(b, 12, ksize=31))
    lib.sourmash_err_clear()
    lib.hll_merge(ha._objptr, make(b, 12, ksize=31)._objptr)
    assert lib.sourmash_err_get_last_code() == 101
    lib.sourmash_err_clear()
    lib.hll_merge(ha._objptr, make([0] * 1024, 10)._objptr)
    assert lib.sourmash_err_get_last_code() == 107
    with pytest.raises(TypeError):
        ha.update(5)
    with pytest.raises(TypeError):
        ha.similarity(5)
    with pytest.raises(ValueError):
        ha.matches(5)
    with pytest.raises(NotImplementedError):
        ha.get(5)


# ---- formats ----------------------------------------------------------------------------------------------------------
def test_save_load_round_trip(tmp_path):
    h = HLL(0.01, 1)
    for i in range(1, 5000):
        h.add(i)
    f = tmp_path / "a.hll"
    h.save(str(f))
    raw = f.read_bytes()
    assert raw[:7] == b"HLL" + bytes([1, 14, 50, 1])
    assert raw[7:] == h.registers()
    h2 = HLL.load(str(f))
    assert h2.registers() == h.registers() and h2.ksize == 1 and h2.precision == 14
    g = tmp_path / "a.hll.gz"
    g.write_bytes(gzip.compress(raw))
    assert HLL.load(str(g)).registers() == h.registers()
    buf = h.to_bytes()
    assert buf[:2] == b"\x1f\x8b"
    assert gzip.decompress(buf) == raw
    assert HLL.from_buffer(buf).registers() == h.registers()
    assert HLL.from_buffer(raw).registers() == h.registers()
    # ksize is stored in one byte (truncated)
    assert HLL.from_buffer(HLL(0.1, 300).to_bytes()).ksize == 300 % 256


def test_bad_files(tmp_path):
    for bad in (b"HLX\x01\x04\x3c\x15" + bytes(16), b"HLL\x02\x04\x3c\x15" + bytes(16), b"HLL\x01\x04\x3c\x15" + bytes(3), b"HL"):
        with pytest.raises(sm.exceptions.SourmashError):
            HLL.from_buffer(bad)
    with pytest.raises(sm.exceptions.SourmashError):
        HLL.load(str(tmp_path / "missing.hll"))


# ---- estimators, bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", list(range(4, 19)))
def test_cardinality_random_registers(p):
    rng = random.Random(1000 + p)
    q = 64 - p
    for trial in range(3):
        fill = [0.0, 0.3, 0.9][trial]
        regs = [0 if rng.random() > fill else min(q + 1, 1 + int(rng.expovariate(math.log(2)))) for _ in range(1 << p)]
        assert make(regs, p).cardinality() == cardinality(regs, p)


@pytest.mark.parametrize("p", [4, 7, 8, 12, 15, 16, 18])
def test_joint_mle_random_registers(p):
    rng = random.Random(2000 + p)
    q = 64 - p
    geo = lambda: min(q + 1, 1 + int(rng.expovariate(math.log(2))))  # noqa: E731
    a = [geo() if rng.random() < 0.8 else 0 for _ in range(1 << p)]
    b = [max(x, geo()) if rng.random() < 0.5 else geo() for x in a]
    ha, hb = make(a, p), make(b, p)
    oa, ob, c = joint_mle(a, b, p)
    assert ha.intersection(hb) == c
    assert _bits(ha.similarity(hb)) == _bits(c / (oa + ob + c)) if (oa + ob + c) else math.isnan(ha.similarity(hb))
    assert _bits(ha.containment(hb)) == _bits(c / (oa + c)) if (oa + c) else math.isnan(ha.containment(hb))
    oa2, ob2, c2 = joint_mle(b, a, p)
    assert hb.intersection(ha) == c2


@pytest.mark.parametrize("p", [4, 9, 14, 16, 18])
def test_edge_registers(p):
    q = 64 - p
    zero = make([0] * (1 << p), p)
    assert zero.cardinality() == 0 == cardinality([0] * (1 << p), p)
    full = make([q + 1] * (1 << p), p)
    assert full.cardinality() == 2 ** 64 - 1
    assert math.isnan(zero.similarity(zero)) and math.isnan(zero.containment(zero))
    assert zero.intersection(zero) == joint_mle([0] * (1 << p), [0] * (1 << p), p)[2]
    assert full.intersection(full) == joint_mle([q + 1] * (1 << p), [q + 1] * (1 << p), p)[2]
    assert full.intersection(zero) == joint_mle([q + 1] * (1 << p), [0] * (1 << p), p)[2]


def test_reference_1_to_5000():
    h = HLL(0.01, 1)
    regs = [0] * (1 << 14)
    for i in range(1, 5000):
        h.add(i)
        add_hash_py(regs, 14, i)
    assert list(h.registers()) == regs
    assert h.cardinality() == cardinality(regs, 14)
    assert len(h) == h.cardinality()


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


@pytest.mark.parametrize("p", [16, 17, 18])
def test_mle_corner_cases(p):
    "sketch/hyperloglog/mod.rs test_mle_corner_cases (the reference hashes with Rust's DefaultHasher; any 64-bit mix will do)"
    h1, h2 = make([0] * (1 << p), p), make([0] * (1 << p), p)
    r1, r2 = [0] * (1 << p), [0] * (1 << p)
    for i in range(1, 5000):
        h1.add(_splitmix(i))
        add_hash_py(r1, p, _splitmix(i))
    for i in range(5000, 10000):
        h2.add(_splitmix(i))
        add_hash_py(r2, p, _splitmix(i))
    c = h1.cardinality()
    assert c == cardinality(r1, p) and 4500 < c < 5500
    u = make(list(h1.registers()), p)
    u.update(h2)
    cu = u.cardinality()
    assert cu == cardinality([max(a, b) for a, b in zip(r1, r2)], p) and 9500 < cu < 10500
    inter = h1.intersection(h2)
    assert inter == joint_mle(r1, r2, p)[2] and inter < 500


def test_ctypes_buffer_free():
    h = HLL(0.1, 21)
    size = C.c_size_t(0)
    raw = lib.hll_to_buffer(h._objptr, C.byref(size))
    assert size.value > 0
    lib.nodegraph_buffer_free(C.cast(raw, C.c_void_p), size.value)
