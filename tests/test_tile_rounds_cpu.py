"""CPU check of the appending sketch kernel's tiles of several window rounds (sourmash_amd/csrc/kmer_core.hpp: TileGeom with its
rounds parameter, stage_tile with a run-time chunk count, read_window at lane index tid + r * 256, sk_tile_rounds) through a host
emulation that walks long tiles the way the kernel does (tests/native/tile_rounds_emul.cpp), against the oracle.  No GPU needed."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from tile_rounds_inputs import KS, OFFSETS, ROUNDS, WINDOW, bad_byte_inputs, boundary_lengths, lower_case_input, palindrome_inputs, random_dna

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "tile_rounds_emul.cpp")
SO = os.path.join(HERE, "native", "libtile_rounds_emul.so")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", h) for h in ("kmer_core.hpp", "murmur3.hpp")]
FULL = 2**64 - 1


@pytest.fixture(scope="module")
def lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    so = C.CDLL(SO)
    so.emul_tile_rounds_sketch.restype = C.c_uint64
    so.emul_tile_rounds_sketch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                           C.c_void_p, C.c_uint64, C.c_void_p]
    so.emul_tile_rounds_rule.restype = C.c_uint32
    so.emul_tile_rounds_rule.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    return so


@pytest.fixture(scope="module")
def emul(lib):
    def run(buf, k, skip, rounds, seed=42, thr=FULL):
        a = np.frombuffer(bytes(buf), dtype=np.uint8)
        out = np.zeros(max(len(a), 1), dtype=np.uint64)
        dirty = C.c_uint64(0)
        n = lib.emul_tile_rounds_sketch(a.ctypes.data, len(a), k, skip, rounds, seed, thr, out.ctypes.data, len(out), C.byref(dirty))
        assert n != FULL, "ksize or rounds not instantiated"
        assert n <= len(out)
        run.dirty_tiles = dirty.value
        return np.sort(out[:n])
    return run


@functools.lru_cache(maxsize=None)
def want_all(buf, k, thr=FULL):
    hs = np.array(oracle.seq_to_hashes(buf, k, seed=42, force=True), dtype=np.uint64) if len(buf) >= k else np.zeros(0, dtype=np.uint64)
    return np.sort(hs[hs <= np.uint64(thr)])                      # bad k-mers and zeros dropped by the oracle


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("k", KS)
def test_boundary_lengths(emul, k, rounds):
    "every hash of random DNA at lengths on either side of a round, of a tile and of their halos, prefixes 0, 1 and 15"
    for n in boundary_lengths(k, rounds):
        s = random_dna(n, seed=k)
        want = want_all(s, k)
        assert (len(want) > 0) == (n >= k), n
        for skip in OFFSETS:
            assert np.array_equal(emul(s, k, skip, rounds), want), (k, rounds, n, skip)


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("k", KS)
def test_bad_byte_on_a_seam(emul, k, rounds):
    "one invalid byte on the last position in front of a seam, round seams and tile seams alike: every k-mer over it is dropped"
    for skip in OFFSETS:
        for name, s in bad_byte_inputs(k, rounds, skip).items():
            want = want_all(s, k)
            assert len(want) < len(s) - k + 1 - (k - 1)            # the k k-mers over the byte are gone
            assert np.array_equal(emul(s, k, skip, rounds), want), (k, rounds, name, skip)


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("k", KS)
def test_palindrome_across_a_seam(emul, k, rounds):
    "a 62-base palindrome (its own reverse complement) with its middle on a seam: first-8-byte ties, both strands equal at even k"
    for skip in OFFSETS:
        for name, s in palindrome_inputs(rounds, skip).items():
            assert np.array_equal(emul(s, k, skip, rounds), want_all(s, k)), (k, rounds, name, skip)


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("k", KS)
def test_lower_case(emul, k, rounds):
    s = lower_case_input(rounds)
    for skip in OFFSETS:
        assert np.array_equal(emul(s, k, skip, rounds), want_all(s, k)), (k, rounds, skip)


@pytest.mark.parametrize("rounds", ROUNDS)
def test_scaled_1000_and_the_tile_flag(emul, rounds):
    "the early reject on clean and on dirty long tiles; the flag is one per long tile"
    thr = oracle.max_hash_for_scaled(1000)
    tile = rounds * WINDOW
    s = bytearray(random_dna(6 * tile + 100, seed=rounds, alphabet=b"ACGT"))
    emul(bytes(s), 31, 0, rounds, thr=thr)
    assert emul.dirty_tiles == 1                                   # only the zero fill behind the end
    s[4 * tile + 10] = ord("N")                                    # inside tile 4 and inside the halo of tile 3
    want = want_all(bytes(s), 31, thr)
    assert 10 * rounds < len(want) < 50 * rounds
    assert np.array_equal(emul(bytes(s), 31, 0, rounds, thr=thr), want)
    assert emul.dirty_tiles == 3
    assert np.array_equal(emul(bytes(s), 31, 4, rounds, thr=thr), want)
    assert emul.dirty_tiles == 4                                   # the blanked prefix dirties tile 0


def test_launcher_rounds_rule(lib):
    """sk_tile_rounds: the long tile wherever the hashes it is expected to keep stay under a quarter of the sink (2 rounds with
    2,048 entries, 3 with 1,024), one round for small scaled values and for num sketches (thr = 2^64 - 1)"""
    for r_max, cap in ((2, 2048), (3, 1024)):
        for scaled, want in ((1, 1), (2, 1), (500, r_max), (1000, r_max)):
            assert lib.emul_tile_rounds_rule(oracle.max_hash_for_scaled(scaled), r_max, cap) == want, (r_max, scaled)
        assert lib.emul_tile_rounds_rule(FULL, r_max, cap) == 1
        assert lib.emul_tile_rounds_rule(0, r_max, cap) == r_max
        # the edge itself: expected appends of the long tile against cap / 4
        positions = r_max * WINDOW
        at = ((cap // 4 - 1) << 64) // positions                   # largest thr with floor(positions * thr / 2^64) + 1 <= cap / 4, about
        assert lib.emul_tile_rounds_rule(at - (1 << 33), r_max, cap) == r_max
        assert lib.emul_tile_rounds_rule(at + (1 << 33) + (1 << 64) // positions, r_max, cap) == 1
    for scaled in (1, 1000):
        assert lib.emul_tile_rounds_rule(oracle.max_hash_for_scaled(scaled), 1, 2048) == 1
