"""CPU check of the appending sketch kernel's staged form (sourmash_amd/csrc/kmer_core.hpp: load_chunk, stage_chunk,
process_lane_staged) through a host emulation that walks tiles the way the kernel does (tests/native/strand_lds_emul.cpp), against
the oracle.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from strand_inputs import TILE, inputs, rand_dna

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "strand_lds_emul.cpp")
SO = os.path.join(HERE, "native", "libstrand_lds_emul.so")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", h) for h in ("kmer_core.hpp", "murmur3.hpp")]
FULL = 2**64 - 1


@pytest.fixture(scope="module")
def emul():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])   # 88 unrolled instantiations: -O0 halves the build
    lib = C.CDLL(SO)
    lib.emul_strand_sketch.restype = C.c_uint64
    lib.emul_strand_sketch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p,
                                       C.c_uint64, C.c_void_p]

    def run(buf, k, skip=0, seed=42, thr=FULL):
        a = np.frombuffer(bytes(buf), dtype=np.uint8)
        out = np.zeros(max(len(a), 1), dtype=np.uint64)
        dirty = C.c_uint64(0)
        n = lib.emul_strand_sketch(a.ctypes.data, len(a), k, skip, seed, thr, out.ctypes.data, len(out), C.byref(dirty))
        assert n != FULL, "ksize not instantiated"
        assert n <= len(out)
        run.dirty_tiles = dirty.value
        return np.sort(out[:n])
    return run


def _oracle_all(buf, k, seed=42, thr=FULL):
    hs = np.array(oracle.seq_to_hashes(bytes(buf), k, seed=seed, force=True), dtype=np.uint64)   # bad k-mers and zeros dropped
    return np.sort(hs[hs <= np.uint64(thr)])


@pytest.mark.parametrize("k", range(1, 89))
def test_every_ksize_every_hash(emul, k):
    "k = 1 .. 88, every hash kept: the inputs of strand_inputs.py, the alignment prefix cycling through 0 .. 15"
    for i, (name, s) in enumerate(inputs(k).items()):
        skip = (5 * i + k) % 16
        assert np.array_equal(emul(s, k, skip), _oracle_all(s, k)), (k, name, skip)


def test_every_alignment_prefix(emul):
    "k = 31 with every prefix 0 .. 15: the blanked bytes are invalid, and everything behind them shifts through the lanes"
    for name in ("random_4096", "n_edges", "ties"):
        s = inputs(31)[name]
        want = _oracle_all(s, 31)
        for skip in range(16):
            assert np.array_equal(emul(s, 31, skip), want), (name, skip)


@pytest.mark.parametrize("k", [21, 31, 32, 51])
def test_scaled_1000_threshold(emul, k):
    "the early reject on the top dword, on clean and on dirty tiles"
    thr = oracle.max_hash_for_scaled(1000)
    rng = np.random.default_rng(k)
    s = bytearray(rand_dna(rng, 100_000))
    for i in range(20 * TILE + 7, len(s), 9973):               # the first 20 tiles stay clean
        s[i] = ord("N")
    want = _oracle_all(bytes(s), k, thr=thr)
    assert 50 < len(want) < 200
    assert np.array_equal(emul(bytes(s), k, 3, 42, thr), want)
    for name, t in inputs(k).items():
        assert np.array_equal(emul(t, k, 0, 42, thr), _oracle_all(t, k, thr=thr)), (k, name)


def test_tile_flag(emul):
    "a tile is dirty iff one of its staged bytes (its 4,096 positions and the halo behind them) is not ACGT; the last one always is"
    rng = np.random.default_rng(5)
    s = bytearray(rand_dna(rng, 3 * TILE + 100))
    emul(bytes(s), 31)
    assert emul.dirty_tiles == 1                               # only the zero fill behind the end
    s[2 * TILE + 10] = ord("N")                                # inside tile 2 and inside the halo of tile 1
    emul(bytes(s), 31)
    assert emul.dirty_tiles == 3
    emul(bytes(s), 31, 4)                                      # the blanked prefix dirties tile 0
    assert emul.dirty_tiles == 4
