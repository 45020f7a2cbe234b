"""GPU parity of the appending sketch kernel's lanes of 32 start positions (sketch_kernel.hpp, sk_lane_positions: a window is 256
lanes x 32 positions, a tile two of them at scaled = 1,000 and one at scaled = 1) with the late mask of the last key dword: the
lengths, pointer offsets and seam inputs of lane32_inputs.py through DeviceSketcher.sketch against oracle.sketch_dna_bulk.  k = 19, 31, 51 and 88 take 32 positions; k = 12 (one round) and k = 36 (past a register step at 32) stay
at 16 and see the same inputs.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import oracle
from lane32_inputs import OFFSETS, R_MAX, WINDOW, bad_byte_inputs, lower_case_input, palindrome_inputs, random_dna
from test_gpu_sketch_dense_input import _oracle_kept, env  # noqa: F401  (env is the fixture)
from test_gpu_tile_edges import device_view

pytestmark = pytest.mark.gpu

TILE = R_MAX * WINDOW          # 16,384 positions
KS = [12, 19, 31, 36, 51, 88]


@functools.lru_cache(maxsize=None)
def want(seq, k, scaled, seed=42):
    return oracle.sketch_dna_bulk(seq, k, scaled=scaled, seed=seed)


def got(torch, smd, seq, off, k, scaled, seed=42):
    return smd.DeviceSketcher(k, scaled, seed).sketch(device_view(torch, seq, off)).cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def cases(k):
    "name -> (bytes, pointer offsets): the lengths, and per pointer offset the seam inputs of tiles of two windows"
    out = {"random_%d" % n: (random_dna(n, seed=k), OFFSETS) for n in (0, k - 1, k, 33, WINDOW + 1, TILE + 1, 2 * TILE + 5)}
    for off in OFFSETS:
        for name, s in bad_byte_inputs(k, R_MAX, off).items():
            out["bad_%s_off%d" % (name, off)] = (s, [off])
        for name, s in palindrome_inputs(R_MAX, off).items():
            out["pal_%s_off%d" % (name, off)] = (s, [off])
    out["lower"] = (lower_case_input(R_MAX), OFFSETS)
    return out


@pytest.mark.parametrize("k", KS)
def test_scaled_1000(env, k):
    "the long tile: about one kept hash in 1,000 positions, so the long inputs keep a few dozen"
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
    "every k-mer kept: the launcher takes one round and the sink spills within every tile"
    torch, smd = env
    for name, (seq, offs) in cases(k).items():
        w = want(seq, k, 1)
        assert (len(w) > 0) == (len(seq) >= k), name
        for off in offs:
            assert np.array_equal(got(torch, smd, seq, off, k, 1), w), (k, name, off)


def test_poly_a_overfills_the_sink_inside_a_tile(env):
    """3 x 16,384 A at scaled = 1,000 under seed 1051, where the hash of A x 31 is below the threshold (oracle): a tile appends one
    hash per position -- far more than its sink of 512 entries holds (the spill), and far more than the capacity sized from `scaled`
    (the retry) -- and the sketch is still that one hash."""
    torch, smd = env
    k, seed, seq = 31, 1051, b"A" * (3 * TILE)
    w = want(seq, k, 1000, seed)
    assert len(w) == 1 and w[0] == oracle.seq_to_hashes(b"A" * k, k, seed=seed, force=True)[0]
    for off in OFFSETS:
        sk = smd.DeviceSketcher(k, 1000, seed)
        assert sk.capacity_for(len(seq)) < len(seq) - k + 1      # the first attempt cannot hold what the kernel keeps
        assert np.array_equal(sk.sketch(device_view(torch, seq, off)).cpu().numpy().view(np.uint64), w), off
        assert sk.cap >= len(seq) - k + 1                          # grown by the retry


@pytest.mark.parametrize("k", [31, 36])
def test_twenty_tiles_on_two_workgroups(env, k):
    "kernel_only(grid = 2): 18 of the 20 tiles are reached by ticket; every appended hash with its duplicates"
    torch, smd = env
    seq = random_dna(20 * TILE + 7, seed=20, alphabet=b"ACGT")
    w = _oracle_kept(smd, seq, k, 1000)
    assert len(w) > 200
    for off in (0, 15):
        view = device_view(torch, seq, off)
        out = torch.zeros(view.numel() + 16, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        smd.DeviceSketcher(k, 1000).kernel_only(view, out, cnt, grid=2)
        torch.cuda.synchronize()
        kept = int(cnt[0].item())
        assert kept <= view.numel()
        assert np.array_equal(np.sort(out[:kept].cpu().numpy().view(np.uint64)), w), (k, off)
