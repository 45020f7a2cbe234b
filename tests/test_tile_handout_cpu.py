"""CPU check of the appending sketch kernel's tile hand-out (sourmash_amd/csrc/kmer_core.hpp: tile_first, tile_from_ticket,
tile_end; sketch_kernel.hpp: the ticket taken in front of a tile's hashing) through a stand-alone host emulation
(tests/native/tile_handout_emul.cpp) in which G workgroups take tickets in a chosen order: the index rule alone, and whole walks
with the kernel's own stage_tile, read_window and process_lane_staged against the oracle.  The program is also built and run
once with AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU needed."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "tile_handout_emul.cpp")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", h) for h in ("kmer_core.hpp", "murmur3.hpp")]
FULL = 2**64 - 1
WINDOW = 256 * 16
ORDERS = {"one_takes_all": 0, "round_robin": 1, "shuffle": 2, "static_stride": 3}
G = 3


def build(name, *flags):
    exe = os.path.join(HERE, "native", name)
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def exe():
    return build("tile_handout_emul", "-O1")


def walk(exe, tmp_path, seq, k, rounds, order, thr, skip=0, g=G):
    "the kept hashes of a walk, in the order they were kept"
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(seq)
    subprocess.check_call([exe, "walk", str(k), str(rounds), str(g), str(ORDERS[order]), str(skip), str(thr), str(src), str(dst)])
    return np.fromfile(dst, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def sequence(rounds):
    """11 tiles and a bit of random ACGT for three workgroups: tiles 3 .. 10 are reached by ticket.  Tile 5 holds a bad byte,
    tile 6 a lower-case stretch that runs over the seam into tile 7; the tiles behind them on the same workgroup are clean."""
    tile = rounds * WINDOW
    rng = np.random.default_rng(5 + rounds)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=10 * tile + 777)].copy()
    s[5 * tile + 1234] = ord("N")
    s[7 * tile - 300:7 * tile + 200] |= 0x20
    return s.tobytes()


@functools.lru_cache(maxsize=None)
def want(rounds, k, thr):
    hs = np.array(oracle.seq_to_hashes(sequence(rounds), k, seed=42, force=True), dtype=np.uint64)   # bad k-mers and zeros dropped
    return np.sort(hs[hs <= np.uint64(thr)])


def test_index_rule(exe):
    """G in {1, 3, 8}, n_tiles in {0, 1, G - 1, G, G + 1, 5 G + 3}, tickets granted to one workgroup, round-robin and shuffled:
    every tile once, none behind the end, the counter at n_tiles - G + G (asserted by the program)"""
    out = subprocess.run([exe, "index"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "index ok: 72 cases"


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("k", [12, 31, 88])
def test_order_independence(exe, tmp_path, k, rounds):
    "every hash (thr = 2^64 - 1) and the kept ones at scaled = 100: the same multiset and the same set whatever the order"
    for thr in (FULL, oracle.max_hash_for_scaled(100)):
        w = want(rounds, k, thr)
        assert len(w) > 100
        for order in ORDERS:
            got = walk(exe, tmp_path, sequence(rounds), k, rounds, order, thr)
            assert np.array_equal(np.sort(got), w), (k, rounds, order, thr)
            assert np.array_equal(np.unique(got), np.unique(w)), (k, rounds, order, thr)


def test_bad_byte_and_lower_case_are_seen(exe, tmp_path):
    "the inputs do what they are there for: the N kills k k-mers of a tile reached by ticket, the lower-case stretch none"
    k, rounds = 31, 3
    n = len(sequence(rounds))
    assert len(want(rounds, k, FULL)) <= n - k + 1 - k
    clean = bytearray(sequence(rounds).upper())
    clean[5 * rounds * WINDOW + 1234] = ord("A")
    lower = bytearray(sequence(rounds))
    lower[5 * rounds * WINDOW + 1234] = ord("a")
    a = walk(exe, tmp_path, bytes(clean), k, rounds, "shuffle", FULL)
    b = walk(exe, tmp_path, bytes(lower), k, rounds, "shuffle", FULL)
    assert len(a) >= n - k and np.array_equal(np.sort(a), np.sort(b))


def test_pointer_offset_and_other_grids(exe, tmp_path):
    "the blanked alignment prefix (tile 0 is dirty, tile 3 on the same workgroup is not) and grids of 1, 2 and 8 workgroups"
    k, rounds, thr = 31, 3, oracle.max_hash_for_scaled(100)
    w = want(rounds, k, thr)
    for skip in (1, 15):
        assert np.array_equal(np.sort(walk(exe, tmp_path, sequence(rounds), k, rounds, "shuffle", thr, skip=skip)), w), skip
    for g in (1, 2, 8, 11, 12):
        assert np.array_equal(np.sort(walk(exe, tmp_path, sequence(rounds), k, rounds, "shuffle", thr, g=g)), w), g


def test_under_the_sanitizers(tmp_path):
    "the stand-alone program with -fsanitize=address,undefined: the index rule and one walk of each k, any report fails the run"
    exe = build("tile_handout_emul_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    out = subprocess.run([exe, "index"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "index ok: 72 cases", out.stderr
    thr = oracle.max_hash_for_scaled(100)
    for k, rounds in ((12, 1), (31, 3), (88, 3)):
        assert np.array_equal(np.sort(walk(exe, tmp_path, sequence(rounds), k, rounds, "shuffle", thr, skip=15)), want(rounds, k, thr))
