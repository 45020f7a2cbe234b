"""GPU parity of the appending sketch kernel's tiles of several window rounds (sketch_kernel.hpp: a staged tile is `rounds`
consecutive windows of 4,096 positions, read back at lane index tid + r * 256): the lengths, pointer offsets and seam inputs of
tile_rounds_inputs.py through DeviceSketcher.sketch against oracle.sketch_dna_bulk -- at scaled = 1,000, where the launcher takes
the long tile, and at scaled = 1, where it takes one round and the sink spills.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import oracle
from test_gpu_sketch_dense_input import env  # noqa: F401  (env is the fixture)
from test_gpu_tile_edges import device_view
from tile_rounds_inputs import KS, OFFSETS, WINDOW, bad_byte_inputs, boundary_lengths, lower_case_input, palindrome_inputs, random_dna

pytestmark = pytest.mark.gpu

R_MAX = 3                      # the inputs cover the seams of tiles of up to three rounds, whichever the library was built with


@functools.lru_cache(maxsize=None)
def want(seq, k, scaled, seed=42):
    return oracle.sketch_dna_bulk(seq, k, scaled=scaled, seed=seed)


def got(torch, smd, seq, off, k, scaled, seed=42):
    return smd.DeviceSketcher(k, scaled, seed).sketch(device_view(torch, seq, off)).cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def cases(k):
    "name -> bytes: the boundary lengths, and per pointer offset the bad-byte and palindrome inputs of tiles of two and three rounds"
    out = {"random_%d" % n: (random_dna(n, seed=k), OFFSETS) for n in boundary_lengths(k, R_MAX) + [2 * 2 * WINDOW + 17]}
    for rounds in (2, 3):
        for off in OFFSETS:
            for name, s in bad_byte_inputs(k, rounds, off).items():
                out["bad_%d_%s_off%d" % (rounds, name, off)] = (s, [off])
            for name, s in palindrome_inputs(rounds, off).items():
                out["pal_%d_%s_off%d" % (rounds, name, off)] = (s, [off])
        out["lower_%d" % rounds] = (lower_case_input(rounds), OFFSETS)
    return out


@pytest.mark.parametrize("k", KS)
def test_scaled_1000_long_tiles(env, k):
    "rounds are on: about one kept hash in 1,000 positions, so the long inputs keep a few dozen"
    torch, smd = env
    kept = 0
    for name, (seq, offs) in cases(k).items():
        w = want(seq, k, 1000)
        kept += len(w)
        for off in offs:
            assert np.array_equal(got(torch, smd, seq, off, k, 1000), w), (k, name, off)
    assert kept > 100


@pytest.mark.parametrize("k", KS)
def test_scaled_1_one_round_and_spills(env, k):
    "every k-mer kept: the launcher falls back to one round and the sink spills within every tile"
    torch, smd = env
    for name, (seq, offs) in cases(k).items():
        w = want(seq, k, 1)
        assert (len(w) > 0) == (len(seq) >= k), name
        for off in offs:
            assert np.array_equal(got(torch, smd, seq, off, k, 1), w), (k, name, off)


def test_poly_a_overfills_the_sink_inside_a_long_tile(env):
    """3 x 12,288 A at scaled = 1,000: every k-mer has the same hash, so a long tile appends one hash per position -- far more than
    the sink holds between two flush checks (the spill), and far more than the capacity sized from `scaled` (the retry) -- and the
    sketch is still that one hash.  Under the default seed 42 the hash of A x 31 is above the threshold of scaled = 1,000 for every
    k = 12 .. 88 and nothing at all would be kept; under seed 1051 it is below it (oracle), so the test runs with that seed."""
    torch, smd = env
    k, seed, seq = 31, 1051, b"A" * (3 * 12288)
    w = want(seq, k, 1000, seed)
    assert len(w) == 1 and w[0] == oracle.seq_to_hashes(b"A" * k, k, seed=seed, force=True)[0]
    for off in OFFSETS:
        sk = smd.DeviceSketcher(k, 1000, seed)
        assert sk.capacity_for(len(seq)) < len(seq) - k + 1      # the first attempt cannot hold what the kernel keeps
        assert np.array_equal(sk.sketch(device_view(torch, seq, off)).cpu().numpy().view(np.uint64), w), off
        assert sk.cap >= len(seq) - k + 1                          # grown by the retry
