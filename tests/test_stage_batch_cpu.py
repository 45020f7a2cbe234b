"""CPU check of the appending sketch kernel's batched tile staging (sourmash_amd/csrc/kmer_core.hpp: stage_batch_ok,
stage_lane_batched beside the loop of stage_tile) through a stand-alone host emulation (tests/native/stage_batch_emul.cpp): every
tile is staged both ways and s_in, s_comp and the flag are compared word for word by the program itself, and the walk's hashes
are compared with the oracle here.  Inputs: k = 19, 31, 37, 51, 88 with the lane geometry the kernel gives them, tiles of one and
two rounds (and of three at k = 37, whose tiles have three: only a tile of all the rounds the kernel holds takes the batch, a
launch of fewer rounds stays on the loop), alignment prefixes 0, 1 and 15, lengths on both
sides of every chunk, round and tile seam -- a tile whose staged bytes end exactly with the buffer among them --, a newline and an
N on bytes 15 and 16 of a chunk and on a tile seam, and lower case.  The program is built plain and with AddressSanitizer and
UndefinedBehaviorSanitizer; its buffer ends with its last byte, so a load of the batch past the end is reported.  No GPU needed."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "stage_batch_emul.cpp")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", h) for h in ("kmer_core.hpp", "murmur3.hpp")]
FULL = 2**64 - 1
BLOCK = 256
KS = [19, 31, 37, 51, 88]
ROUNDS = [1, 2]
CASES = [(k, r) for k in KS for r in ROUNDS] + [(37, 3)]
SKIPS = [0, 1, 15]


def rounds_max(k):
    "sk_rounds_max of sketch_kernel.hpp for the ksizes of this test"
    return 2 if lane_positions(k) == 32 else 3


def lane_positions(k):
    "sk_lane_positions of sketch_kernel.hpp for the ksizes of this test"
    return 16 if 35 <= k <= 40 or 53 <= k <= 56 else 32


def geometry(k, rounds):
    "TileGeom of kmer_core.hpp -> (positions per round, positions per tile, 16-byte chunks staged per tile)"
    p = lane_positions(k)
    lane_rd = ((p + k - 1 + 3) // 4 + 3) // 4 * 4
    chunks = ((rounds * BLOCK - 1) * (p // 4) + lane_rd + 3) // 4
    return BLOCK * p, rounds * BLOCK * p, chunks


def build(name, *flags):
    exe = os.path.join(HERE, "native", name)
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def exe():
    return build("stage_batch_emul", "-O2")


def walk(exe, tmp_path, seq, k, rounds, skip, thr=FULL):
    "-> (sorted hashes, tiles, tiles staged in one batch, dirty tiles); the program fails where the two stagings differ"
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(seq)
    run = subprocess.run([exe, str(k), str(rounds), str(skip), str(thr), str(src), str(dst)], capture_output=True, text=True)
    assert run.returncode == 0, (k, rounds, skip, len(seq), run.stderr[-2000:])
    tiles, batched, dirty = map(int, re.fullmatch(r"tiles (\d+) batched (\d+) dirty (\d+)", run.stdout.strip()).groups())
    return np.sort(np.fromfile(dst, dtype=np.uint64)), tiles, batched, dirty


def batched_tiles(total, k, rounds, skip):
    """the rule, counted here: tiles of all the kernel's rounds whose staged chunks end inside the buffer, but for the first one
    behind an alignment prefix"""
    return inside_tiles(total, k, rounds, skip) if rounds == rounds_max(k) else 0


def inside_tiles(total, k, rounds, skip):
    "tiles whose staged chunks end inside the buffer, but for the first one behind an alignment prefix"
    _, tile, chunks = geometry(k, rounds)
    n_tiles = -(-total // tile)
    return sum(1 for t in range(n_tiles) if t * tile + 16 * chunks <= total and not (t == 0 and skip))


@functools.lru_cache(maxsize=None)
def random_dna(n, seed=0, alphabet=b"ACGT"):
    rng = np.random.default_rng(8100 + 131 * seed + n)
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n))


@functools.lru_cache(maxsize=None)
def want(seq, k, thr=FULL):
    hs = np.array(oracle.seq_to_hashes(seq, k, seed=42, force=True), dtype=np.uint64) if len(seq) >= k else np.zeros(0, dtype=np.uint64)
    return np.sort(hs[hs <= np.uint64(thr)])                      # bad k-mers and zeros dropped by the oracle


def seam_totals(k, rounds):
    """lengths of the walk (prefix included) on both sides of: a chunk seam, the round seam, the tile seam, the end of a tile's
    staged chunks (the last tile that may take the batch, and one byte short of it, the first that may not), for the first
    tile and for the second"""
    window, tile, chunks = geometry(k, rounds)
    staged = 16 * chunks
    at = {16, 32, window, tile, staged - 16, staged, tile + 16, tile + staged - 16, tile + staged, 2 * tile}
    return sorted({n + d for n in at for d in (-1, 0, 1)} | {k - 1, k, 2 * tile + staged})


@pytest.mark.parametrize("k,rounds", CASES)
def test_lengths_on_every_seam(exe, tmp_path, k, rounds):
    "every hash of random DNA; the number of batched tiles is the rule's, and a tile that ends exactly at len is one of them"
    _, tile, chunks = geometry(k, rounds)
    exact = 0
    for total in seam_totals(k, rounds):
        for skip in SKIPS:
            if total < skip:
                continue
            seq = random_dna(total - skip, seed=k)
            got, tiles, batched, dirty = walk(exe, tmp_path, seq, k, rounds, skip)
            assert np.array_equal(got, want(seq, k)), (k, rounds, total, skip)
            assert tiles == -(-total // tile)
            assert batched == batched_tiles(total, k, rounds, skip), (k, rounds, total, skip)
            exact += total == tile + 16 * chunks and batched == (2 if skip == 0 else 1)
            # clean input: dirty are the tiles that reach the zero fill, and the first behind a prefix
            assert dirty == tiles - inside_tiles(total, k, rounds, 0) + (1 if skip and total >= 16 * chunks else 0), (k, rounds, total, skip)
    assert exact == (len(SKIPS) if rounds == rounds_max(k) else 0)


@pytest.mark.parametrize("k,rounds", CASES)
def test_bad_bytes_on_chunk_and_tile_seams(exe, tmp_path, k, rounds):
    "a newline and an N on the last byte of a chunk, on the first of the next and on either side of a tile seam, in batched tiles"
    _, tile, chunks = geometry(k, rounds)
    total = 2 * tile + 16 * chunks + 40                           # three batched tiles (two behind a prefix) and a last one on the loop
    # byte 15 and byte 16 (the next chunk's first) with either character, both sides of a tile seam with either, the halo's end
    spots = [(16 * 7 + 15, b"\n"), (16 * 7 + 16, b"N"), (16 * 300 + 15, b"N"), (16 * 300 + 16, b"\n"), (tile - 1, b"\n"), (tile, b"N"),
             (2 * tile - 1, b"N"), (2 * tile, b"\n"), (tile + 16 * chunks - 1, b"N")]
    for skip in SKIPS:
        for at, bad in spots:
            s = bytearray(random_dna(total - skip, seed=k + rounds))
            s[at - skip] = bad[0]
            s = bytes(s)
            w = want(s, k)
            assert len(w) <= len(s) - k + 1 - k                    # the k k-mers over the byte are gone
            got, tiles, batched, dirty = walk(exe, tmp_path, s, k, rounds, skip)
            assert np.array_equal(got, w), (k, rounds, skip, bad, at)
            assert (tiles, batched) == (4, batched_tiles(total, k, rounds, skip))
            assert inside_tiles(total, k, rounds, skip) == (3 if skip == 0 else 2)
            assert dirty >= 2                                      # the tile of the byte and the last one, at the least


@pytest.mark.parametrize("k,rounds", CASES)
def test_lower_case(exe, tmp_path, k, rounds):
    "lower and mixed case: upper-cased at staging in both forms, no tile dirty but the last"
    _, tile, chunks = geometry(k, rounds)
    total = tile + 16 * chunks + 5
    for skip in SKIPS:
        for alphabet in (b"acgt", b"ACGTacgt"):
            s = random_dna(total - skip, seed=3 * k + rounds, alphabet=alphabet)
            got, tiles, batched, dirty = walk(exe, tmp_path, s, k, rounds, skip)
            assert np.array_equal(got, want(s, k)), (k, rounds, skip, alphabet)
            assert np.array_equal(got, want(s.upper(), k))
            assert (tiles, batched, dirty) == (3, batched_tiles(total, k, rounds, skip), 1 if skip == 0 else 2)
            assert inside_tiles(total, k, rounds, skip) == (2 if skip == 0 else 1)


def test_scaled_1000_clean_and_dirty_tiles_in_turn(exe, tmp_path):
    "the early reject on clean and dirty batched tiles in turn: the flag is the tile's own"
    k, rounds = 31, 2
    _, tile, chunks = geometry(k, rounds)
    thr = oracle.max_hash_for_scaled(1000)
    s = bytearray(random_dna(6 * tile + 20, seed=1))              # tile 5's halo reaches 12 bytes past the end
    for t in (1, 2, 4):                                            # dirty tiles next to each other and next to clean ones
        s[t * tile + 5000] = ord("N")
    s = bytes(s)
    got, tiles, batched, dirty = walk(exe, tmp_path, s, k, rounds, 0, thr)
    assert np.array_equal(got, want(s, k, thr)) and len(got) > 50
    assert (tiles, batched, dirty) == (7, 5, 5)                    # tiles 1, 2, 4 and the two that reach the zero fill


def test_under_the_sanitizers(tmp_path):
    "the stand-alone program with -fsanitize=address,undefined on inputs that end with a batched tile's last chunk; any report fails"
    exe = build("stage_batch_emul_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    for k, rounds in ((19, 1), (31, 2), (37, 3), (51, 2), (88, 2)):
        _, tile, chunks = geometry(k, rounds)
        for skip in SKIPS:
            for total in (16 * chunks - 1, 16 * chunks, tile + 16 * chunks, tile + 16 * chunks + 1):
                s = random_dna(total - skip, seed=k, alphabet=b"ACGTacgtN")
                got, tiles, batched, _ = walk(exe, tmp_path, s, k, rounds, skip)
                assert np.array_equal(got, want(s, k)), (k, rounds, skip, total)
                assert batched == batched_tiles(total, k, rounds, skip)
