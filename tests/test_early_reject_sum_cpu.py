"""CPU checks of the two exact shortcuts of the sketch kernel's hot path (sourmash_amd/csrc/murmur3.hpp, kmer_core.hpp
compiled for the host): the early reject that looks at the top dword of ONE product, (a + b) * c, instead of two, and the
seed folded into the constant of MurmurHash3's first block.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "early_reject_sum_emul.cpp")
SO = os.path.join(HERE, "native", "libearly_reject_sum_emul.so")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", h) for h in ("kmer_core.hpp", "murmur3.hpp")]
U64 = 2**64


@pytest.fixture(scope="module")
def lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    lib = C.CDLL(SO)
    lib.emul_sum_form_violations.restype = C.c_uint64
    lib.emul_sum_form_violations.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    lib.emul_filter_violations.restype = C.c_uint64
    lib.emul_filter_violations.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.emul_lane31.restype = C.c_uint64
    lib.emul_lane31.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int]
    lib.emul_h1_pair.restype = C.c_int
    lib.emul_h1_pair.argtypes = [C.c_char_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def _lane31(lib, seq, thr, early, seed=42):
    a = np.frombuffer(seq, dtype=np.uint8)
    out = np.zeros(len(a), dtype=np.uint64)
    n = lib.emul_lane31(a.ctypes.data, len(a), seed, thr, out.ctypes.data, len(out), int(early))
    assert n <= len(out)
    return out[:n]                                           # in the order the lanes emit them


def test_top_dword_of_the_summed_product(lib):
    "t - s is -1, 0 or +1 (mod 2^32) for 2 * 10^6 pairs, the wrapping sums among them; each of the three values occurs"
    counts = (C.c_uint64 * 3)()
    assert lib.emul_sum_form_violations(2_000_000, 42, counts) == 0
    assert sum(counts) == 2_000_000
    assert all(c > 0 for c in counts), list(counts)


def test_filter_on_constructed_hashes(lib):
    """Open pairs built to close to a chosen hash h (top dwords 0, 1, 0xfffffffe, 0xffffffff and the values next to the dword
    boundaries): with thr on, one below and one above h, and 2^64 - 1, the filter never rejects a pair the keep rule keeps."""
    passed = C.c_uint64()
    tops = (0, 1, 0xfffffffe, 0xffffffff, 0x00418937)       # (the last: the top dword of max_hash at scaled = 1000)
    lows = (0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff)
    for top in tops:
        for low in lows:
            h = (top << 32) | low
            if h == 0:
                continue
            for thr in {h, h - 1, (h + 1) % U64, U64 - 1, (top << 32) | 0xffffffff, top << 32} - {0}:
                assert lib.emul_filter_violations(h, thr, 200, h ^ thr, C.byref(passed)) == 0, (hex(h), hex(thr))
                if h <= thr:
                    assert passed.value == 200
    # and it still rejects: a hash two dwords above the threshold's never passes
    assert lib.emul_filter_violations(5 << 32, (2 << 32) | 7, 200, 1, C.byref(passed)) == 0 and passed.value == 0
    # ... while one dword above may (the window is {t - 1, t, t + 1}); three dwords above the scaled = 1000 threshold never
    thr = oracle.max_hash_for_scaled(1000)
    assert lib.emul_filter_violations(thr + (3 << 32), thr, 200, 2, C.byref(passed)) == 0 and passed.value == 0


def test_process_lane_early_on_equals_off(lib):
    "process_lane<31, 16> emits exactly the same hashes, in the same order, with the early reject on and off"
    rng = np.random.default_rng(11)
    s = bytearray(rng.choice(np.frombuffer(b"ACGTacgt", dtype=np.uint8), 6000))
    for i in range(1, len(s), 89):
        s[i] = ord("N")
    s = bytes(s)
    allh = np.sort(np.array([h for h in oracle.seq_to_hashes(s, 31, seed=42, force=True) if h], dtype=np.uint64))
    assert len(allh) > 3000
    thrs = {U64 - 1, U64 - 2}
    for h in map(int, (allh[0], allh[1], allh[len(allh) // 2], allh[-2], allh[-1])):
        thrs.update([h, h - 1, h + 1])                       # on, one below, one above a real hash value
        for top in (0, 1, 0xfffffffe, 0xffffffff):           # thresholds whose top dword sits at either end
            thrs.update([(top << 32) | (h & 0xffffffff), (top << 32) | ((h - 1) & 0xffffffff), (top << 32) | ((h + 1) & 0xffffffff)])
    for top in (0, 1, 0xfffffffd, 0xfffffffe, 0xffffffff):
        thrs.update([top << 32, (top << 32) | 0xffffffff])
    for thr in sorted(t for t in thrs if 0 < t < U64):
        on, off = _lane31(lib, s, thr, True), _lane31(lib, s, thr, False)
        assert np.array_equal(on, off), hex(thr)
        assert np.array_equal(np.sort(on), allh[allh <= np.uint64(thr)]), hex(thr)


@pytest.mark.parametrize("seed", [0, 42, 2**32 - 1, 2**63 + 5])
def test_folded_seed_block(lib, seed):
    "mmh3_h1_words<K> (seed folded into the first block's constant) == mmh3_h1_bytes == the oracle (seeds below 2^32)"
    rng = np.random.default_rng(seed % 1000)
    w, b = C.c_uint64(), C.c_uint64()
    for k in (15, 16, 31, 32, 47):
        for rep in range(50):
            key = bytes(rng.integers(0, 256, k, dtype=np.uint8)) if rep % 2 else bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), k))
            assert lib.emul_h1_pair(key, k, seed, C.byref(w), C.byref(b)) == 0
            assert w.value == b.value, (k, seed, key)
            if rep % 2 == 0 and seed < 2**32:
                assert w.value == oracle.hash_murmur(key, seed), (k, seed, key)
