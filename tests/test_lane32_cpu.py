"""CPU check of the appending sketch kernel's lanes of 32 start positions (sourmash_amd/csrc/kmer_core.hpp: LaneGeom and TileGeom
at P = 32, read_window with a lane stride of 32 bytes, process_lane_staged with the last key dword masked behind the strand select)
and of the words form of the hash for every key length (murmur3.hpp: mmh3_open_words), through a host emulation that walks a buffer
the way the kernel does (tests/native/lane32_emul.cpp).  Two references: the distinct values against oracle.sketch_dna_bulk, every
value with its duplicates against oracle.seq_to_hashes.  No GPU needed."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from lane32_inputs import KS, OFFSETS, ROUNDS, WINDOW, bad_byte_inputs, boundary_lengths, lower_case_input, palindrome_inputs, random_dna

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "lane32_emul.cpp")
SO = os.path.join(HERE, "native", "liblane32_emul.so")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", h) for h in ("kmer_core.hpp", "murmur3.hpp")]
FULL = 2**64 - 1


@pytest.fixture(scope="module")
def lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    so = C.CDLL(SO)
    so.emul_lane32_sketch.restype = C.c_uint64
    so.emul_lane32_sketch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                      C.c_void_p, C.c_uint64, C.c_void_p]
    so.emul_lane32_murmur.restype = C.c_uint64
    so.emul_lane32_murmur.argtypes = [C.c_uint64]
    return so


@pytest.fixture(scope="module")
def emul(lib):
    def run(buf, k, skip, rounds, seed=42, thr=FULL):
        a = np.frombuffer(bytes(buf), dtype=np.uint8)
        out = np.zeros(max(len(a), 1), dtype=np.uint64)
        dirty = C.c_uint64(0)
        n = lib.emul_lane32_sketch(a.ctypes.data, len(a), k, skip, rounds, seed, thr, out.ctypes.data, len(out), C.byref(dirty))
        assert n != FULL, "ksize or rounds not instantiated"
        assert n <= len(out)
        run.dirty_tiles = dirty.value
        return np.sort(out[:n])
    return run


@functools.lru_cache(maxsize=None)
def want_all(buf, k, thr=FULL):
    "every kept hash with its duplicates, sorted (bad k-mers and zeros dropped by the oracle)"
    hs = np.array(oracle.seq_to_hashes(buf, k, seed=42, force=True), dtype=np.uint64) if len(buf) >= k else np.zeros(0, dtype=np.uint64)
    return np.sort(hs[hs <= np.uint64(thr)])


@functools.lru_cache(maxsize=None)
def want_set(buf, k, thr=FULL):
    return oracle.sketch_dna_bulk(buf, k, max_hash=0 if thr == FULL else thr)


def check(emul, buf, k, skip, rounds, thr=FULL, what=None):
    got = emul(buf, k, skip, rounds, thr=thr)
    assert np.array_equal(np.unique(got), want_set(buf, k, thr)), ("set", k, rounds, skip, what)
    assert np.array_equal(got, want_all(buf, k, thr)), ("multiset", k, rounds, skip, what)
    return got


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("k", KS)
def test_boundary_lengths(emul, k, rounds):
    "every hash of random DNA at lengths on either side of a lane, a window, a tile and their halos, prefixes 0, 1 and 15"
    for n in boundary_lengths(k, rounds):
        s = random_dna(n, seed=k)
        assert (len(want_all(s, k)) > 0) == (n >= k), n
        for skip in OFFSETS:
            check(emul, s, k, skip, rounds, what=n)


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("k", KS)
def test_bad_byte_on_a_seam(emul, k, rounds):
    "one invalid byte on the last position in front of a lane, window or tile seam: every k-mer over it is dropped"
    for skip in OFFSETS:
        for name, s in bad_byte_inputs(k, rounds, skip).items():
            assert len(want_all(s, k)) < len(s) - k + 1 - (k - 1)          # the k k-mers over the byte are gone
            check(emul, s, k, skip, rounds, what=name)


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("k", KS)
def test_palindrome_across_a_seam(emul, k, rounds):
    "a 62-base palindrome with its middle on a seam: first-8-byte ties, so the strand is picked on whole keys with the late mask"
    for skip in OFFSETS:
        for name, s in palindrome_inputs(rounds, skip).items():
            check(emul, s, k, skip, rounds, what=name)


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("k", KS)
def test_lower_case(emul, k, rounds):
    s = lower_case_input(rounds)
    for skip in OFFSETS:
        check(emul, s, k, skip, rounds)


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("k", KS)
def test_thresholds_around_real_hashes(emul, k, rounds):
    "thr on a hash the input has, one under and one over it: the early reject's window and the keep rule h <= thr"
    s = random_dna(rounds * WINDOW + 40, seed=300 + k, alphabet=b"ACGT")
    every = want_all(s, k)
    for h in (int(every[0]), int(every[len(every) // 1000]), int(every[len(every) // 2]), int(every[-1])):
        for thr in (h - 1, h, h + 1):
            got = check(emul, s, k, 1, rounds, thr=thr, what=(h, thr))
            assert (h in got) == (thr >= h)


@pytest.mark.parametrize("rounds", ROUNDS)
def test_scaled_1000_and_the_tile_flag(emul, rounds):
    "the early reject on clean and on dirty tiles; the flag is one per tile"
    thr = oracle.max_hash_for_scaled(1000)
    tile = rounds * WINDOW
    s = bytearray(random_dna(6 * tile + 100, seed=rounds, alphabet=b"ACGT"))
    emul(bytes(s), 31, 0, rounds, thr=thr)
    assert emul.dirty_tiles == 1                                   # only the zero fill behind the end
    s[4 * tile + 10] = ord("N")                                    # inside tile 4 and inside the halo of tile 3
    want = want_all(bytes(s), 31, thr)
    assert 20 * rounds < len(want) < 100 * rounds
    assert np.array_equal(emul(bytes(s), 31, 0, rounds, thr=thr), want)
    assert emul.dirty_tiles == 3
    assert np.array_equal(emul(bytes(s), 31, 4, rounds, thr=thr), want)
    assert emul.dirty_tiles == 4                                   # the blanked prefix dirties tile 0


def test_every_tail_of_the_words_hash(lib):
    "mmh3_open_words<K> and mmh3_h1_words<K> == mmh3_h1_bytes for K = 1 .. 88: no tail, tails of at most 8 bytes and longer ones"
    assert lib.emul_lane32_murmur(300) == 0

