"""Inputs for the checks of the sketch kernel's tiles of several window rounds (tests/test_tile_rounds_cpu.py on the host
emulation, tests/test_gpu_tile_rounds.py on the GPU).  A round is 4,096 start positions and a tile is `rounds` of them; the lanes
of round r read the staged tile from position r * 4,096 on, so what can go wrong sits at the seams: between two rounds of a tile
(no halo is staged there, the next round's bytes are the halo) and between two tiles (the halo is staged again)."""
import functools

import numpy as np

from strand_inputs import revcomp

WINDOW = 4096
ROUNDS = [1, 2, 3]
OFFSETS = [0, 1, 15]
KS = [12, 21, 31, 51, 88]


@functools.lru_cache(maxsize=None)
def random_dna(n, seed=0, alphabet=b"ACGTacgt"):
    rng = np.random.default_rng(7000 + 31 * seed + n)
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n))


def boundary_lengths(k, rounds):
    return sorted({0, k - 1, k, 4095, 4096, 4097, 4096 + k - 1, 8191, 8192, 8193, 8192 + k - 1, 12287, 12289,
                   2 * rounds * WINDOW + 17})


def seams(rounds):
    "name -> position of the first byte behind a seam, two tiles' worth: round seams inside a tile, tile seams between two"
    return {("tile_seam_%d" if r % rounds == 0 else "round_seam_%d") % r: r * WINDOW for r in range(1, 2 * rounds)}


def bad_byte_inputs(k, rounds, skip):
    """one N per input, on the last position in front of a seam of the walk (which starts `skip` bytes in front of the buffer), so
    that the k-mers over it straddle the seam"""
    out = {}
    for name, at in seams(rounds).items():
        s = bytearray(random_dna(2 * rounds * WINDOW + 17, seed=k + rounds))
        s[at - 1 - skip] = ord("N")
        out[name] = bytes(s)
    return out


def palindrome_inputs(rounds, skip):
    "a 62-base palindrome with its middle on a seam of the walk, upper case on one seam and lower case on the next"
    h = random_dna(31, seed=62, alphabet=b"ACGT")
    pal = h + revcomp(h)
    out = {}
    for i, (name, at) in enumerate(seams(rounds).items()):
        s = bytearray(random_dna(2 * rounds * WINDOW + 17, seed=100 + rounds, alphabet=b"ACGT"))
        lo = at - 31 - skip
        s[lo:lo + 62] = pal if i % 2 == 0 else pal.lower()
        out[name] = bytes(s)
    return out


def lower_case_input(rounds):
    "all lower case but a few upper-case stretches over the seams"
    s = bytearray(random_dna(2 * rounds * WINDOW + 17, seed=200 + rounds, alphabet=b"acgt"))
    for at in seams(rounds).values():
        s[at - 5:at + 3] = bytes(s[at - 5:at + 3]).upper()
    return bytes(s)
