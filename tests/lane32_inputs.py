"""Inputs for the checks of the sketch kernel's lanes of 32 start positions (tests/test_lane32_cpu.py on the host emulation,
tests/test_gpu_lane32.py on the GPU).  A lane takes 32 consecutive positions, a window is 256 lanes = 8,192 positions, and a tile
is `rounds` windows staged together.  What can go wrong sits at the seams: between two lanes (the next lane's bytes are this
lane's halo), between two windows of a tile (no halo is staged there) and between two tiles (the halo is staged again)."""
import functools

import numpy as np

from strand_inputs import revcomp

LANE = 32
WINDOW = 256 * LANE            # 8,192
R_MAX = 2                      # the committed rounds of a long tile at 32 positions per lane (sketch_kernel.hpp)
ROUNDS = [1, R_MAX]
OFFSETS = [0, 1, 15]
KS = [19, 21, 31, 32, 33, 47, 48, 51, 64, 88]     # tails: none (32, 48, 64), <= 8 bytes (19, 21, 33, 51, 88), > 8 (31, 47); K % 4 = 0 .. 3


@functools.lru_cache(maxsize=None)
def random_dna(n, seed=0, alphabet=b"ACGTacgt"):
    rng = np.random.default_rng(3200 + 31 * seed + n)
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n))


def boundary_lengths(k, rounds):
    "either side of a lane, of a window, of a window and its halo, and the same around one and two tiles"
    tile = rounds * WINDOW
    out = {31, 32, 33}
    for at in (WINDOW, tile, 2 * tile):
        out |= {at - 1, at, at + 1, at + k - 1}
    return sorted(out)


def seams(rounds):
    "name -> position of the first byte behind a seam: a lane seam inside a window, then two tiles' worth of window and tile seams"
    out = {"lane_seam": 77 * LANE}
    for r in range(1, 2 * rounds):
        out[("tile_seam_%d" if r % rounds == 0 else "window_seam_%d") % r] = r * WINDOW
    return out


def total(rounds):
    return 2 * rounds * WINDOW + 17


def bad_byte_inputs(k, rounds, skip):
    """one N per input, on the last position in front of a seam of the walk (which starts `skip` bytes in front of the buffer), so
    that the k-mers over it straddle the seam"""
    out = {}
    for name, at in seams(rounds).items():
        s = bytearray(random_dna(total(rounds), seed=k + rounds))
        s[at - 1 - skip] = ord("N")
        out[name] = bytes(s)
    return out


def palindrome_inputs(rounds, skip):
    """a 62-base palindrome with its middle on a seam of the walk, upper case on one seam and lower case on the next: its k-mers tie
    on their first 8 bytes with their reverse complements, so the strand is picked on whole keys (the tie-break, which masks its own
    copies of the last key dword)"""
    h = random_dna(31, seed=62, alphabet=b"ACGT")
    pal = h + revcomp(h)
    out = {}
    for i, (name, at) in enumerate(seams(rounds).items()):
        s = bytearray(random_dna(total(rounds), seed=100 + rounds, alphabet=b"ACGT"))
        lo = at - 31 - skip
        s[lo:lo + 62] = pal if i % 2 == 0 else pal.lower()
        out[name] = bytes(s)
    return out


def lower_case_input(rounds):
    "all lower case but a few upper-case stretches over the seams"
    s = bytearray(random_dna(total(rounds), seed=200 + rounds, alphabet=b"acgt"))
    for at in seams(rounds).values():
        s[at - 5:at + 3] = bytes(s[at - 5:at + 3]).upper()
    return bytes(s)
