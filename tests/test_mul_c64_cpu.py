"""CPU checks of the limb-wise 64-bit constant multiply of the hash (sourmash_amd/csrc/murmur3.hpp, mul_c64, compiled for the
host): the limb form equals x * c mod 2^64 for every constant of murmur3.hpp, on edge values and on a seeded sweep, and the hash
built on it -- mmh3_h1_words<K>, limb form and plain form -- still equals mmh3_h1_bytes and the oracle.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "mul_c64_emul.cpp")
SO = os.path.join(HERE, "native", "libmul_c64_emul.so")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", "murmur3.hpp")]
U64 = 2**64
M32 = 2**32 - 1

CONSTANTS = (0x87c37b91114253d5, 0x4cf5ad432745937f, 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53, 0x52dce729, 0x38495ab5)
EDGES = (0, 1, 2, M32 - 1, M32, 2**32, 2**32 + 1, 2**63 - 1, 2**63, 2**63 + 1, U64 - 2, U64 - 1,
         M32 << 32,                       # high limb all ones, low limb zero
         (M32 << 32) | 1, (1 << 32) | M32,  # one limb all ones, the other 1
         (0x12345678 << 32) | M32, (M32 << 32) | 0x9abcdef0,
         0x8000000080000000, 0x7fffffff7fffffff, 0x0000000100000001, 0xaaaaaaaa55555555)
KS = (1, 7, 8, 9, 15, 16, 17, 21, 24, 25, 31, 32, 33, 47, 48, 51, 63, 64, 65, 88, 89, 128)


@pytest.fixture(scope="module")
def lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    lib = C.CDLL(SO)
    lib.emul_n_consts.restype = C.c_int
    lib.emul_const.restype = C.c_uint64
    lib.emul_const.argtypes = [C.c_int]
    lib.emul_mul_c64.restype = C.c_int
    lib.emul_mul_c64.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.emul_sweep_violations.restype = C.c_uint64
    lib.emul_sweep_violations.argtypes = [C.c_uint64, C.c_uint64]
    lib.emul_fmix_violations.restype = C.c_uint64
    lib.emul_fmix_violations.argtypes = [C.c_uint64, C.c_uint64]
    lib.emul_h1_forms.restype = C.c_int
    lib.emul_h1_forms.argtypes = [C.c_char_p, C.c_uint32, C.c_uint64, C.c_void_p]
    return lib


def test_constants_are_the_headers(lib):
    assert lib.emul_n_consts() == len(CONSTANTS)
    assert tuple(lib.emul_const(i) for i in range(len(CONSTANTS))) == CONSTANTS


@pytest.mark.parametrize("ci", range(len(CONSTANTS)))
def test_limb_form_on_edge_values(lib, ci):
    "x * c mod 2^64 (Python integers) == the limb form == the plain form, for every edge value and each constant as x too"
    a, b = C.c_uint64(), C.c_uint64()
    for x in EDGES + CONSTANTS:
        assert lib.emul_mul_c64(ci, x, C.byref(a), C.byref(b)) == 0
        want = (x * CONSTANTS[ci]) % U64
        assert a.value == want, (hex(x), hex(CONSTANTS[ci]), hex(a.value), hex(want))
        assert b.value == want, (hex(x), hex(CONSTANTS[ci]))


def test_limb_form_on_a_seeded_sweep(lib):
    "2 * 10^6 pseudo-random x (two in five with an all-ones limb) times the six constants, both forms"
    assert lib.emul_sweep_violations(2_000_000, 42) == 0
    # and the same x against Python integers, for a sample
    rng = np.random.default_rng(7)
    a, b = C.c_uint64(), C.c_uint64()
    for x in map(int, rng.integers(0, U64, 2000, dtype=np.uint64)):
        for ci, c in enumerate(CONSTANTS):
            lib.emul_mul_c64(ci, x, C.byref(a), C.byref(b))
            assert a.value == b.value == (x * c) % U64


def test_fmix64_and_its_halves(lib):
    assert lib.emul_fmix_violations(500_000, 3) == 0


@pytest.mark.parametrize("seed", [0, 42, 2**32 - 1, 2**63 + 5])
def test_h1_words_equals_h1_bytes(lib, seed):
    "mmh3_h1_words<K> in the limb form and in the plain form == mmh3_h1_bytes == the oracle (seeds below 2^32), K = 1 .. 128"
    rng = np.random.default_rng(seed % 1000 + 1)
    out = (C.c_uint64 * 3)()
    for k in KS:
        for rep in range(40):
            if rep == 0:
                key = b"\xff" * k
            elif rep == 1:
                key = b"\x00" * k
            elif rep % 2:
                key = bytes(rng.integers(0, 256, k, dtype=np.uint8))
            else:
                key = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), k))
            assert lib.emul_h1_forms(key, k, seed, out) == 0
            assert out[0] == out[2], (k, seed, key)
            assert out[1] == out[2], (k, seed, key)
            if seed < 2**32:
                assert out[2] == oracle.hash_murmur(key, seed), (k, seed, key)
