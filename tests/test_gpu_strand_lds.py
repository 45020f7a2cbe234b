"""GPU parity of the appending sketch kernel's staged form (sketch_kernel.hpp: the tile goes to LDS upper-cased and complemented,
validity is decided per tile, lanes read both copies): every kept hash against the oracle on the inputs of strand_inputs.py,
with the harness of test_gpu_sketch_dense_input.py.  Run with -m gpu."""
import numpy as np
import pytest

import oracle
from strand_inputs import TILE, inputs, rand_dna
from test_gpu_sketch_dense_input import _kernel_only, _oracle_kept, env  # noqa: F401  (env is the fixture)

pytestmark = pytest.mark.gpu

KS = [21, 31, 32, 51, 70, 88]


def _kernel_only_at(torch, smd, dev, k, scaled):
    "_kernel_only for a tensor that is already on the device (a slice: the pointer need not be aligned)"
    sk = smd.DeviceSketcher(k, scaled)
    out = torch.zeros(dev.numel() + 16, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    sk.kernel_only(dev, out, cnt)
    torch.cuda.synchronize()
    kept = int(cnt[0].item())
    assert kept <= dev.numel()
    return np.sort(out[:kept].cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("k", KS)
def test_every_hash(env, k):
    "scaled = 1: lengths around the tile, N on tile edges and in the halo, separators, first-8-byte ties, palindromes"
    torch, smd = env
    for name, seq in inputs(k).items():
        if len(seq) == 0:
            continue
        assert np.array_equal(_kernel_only(torch, smd, seq, k, 1), _oracle_kept(smd, seq, k, 1)), (k, name)


@pytest.mark.parametrize("k", [31, 88])
def test_pointer_alignment(env, k):
    "device pointers 1, 7 and 15 bytes past a 16-byte boundary: the kernel backs up and blanks the bytes in front"
    torch, smd = env
    for name in ("random_%d" % (TILE + k - 1), "n_edges", "ties"):
        seq = inputs(k)[name]
        want = _oracle_kept(smd, seq, k, 1)
        for off in (1, 7, 15):
            whole = torch.frombuffer(bytearray(b"ACGT" * 4 + seq), dtype=torch.uint8).cuda()   # valid bases in front
            part = whole[off:off + len(seq)]
            part.copy_(torch.frombuffer(bytearray(seq), dtype=torch.uint8))
            assert part.data_ptr() % 16 == off
            assert np.array_equal(_kernel_only_at(torch, smd, part, k, 1), want), (k, name, off)


def test_reject_path(env):
    "scaled = 1000 on 10^6 random bases, the whole step: nearly every wave-step leaves at the early reject; all tiles but the last are clean"
    torch, smd = env
    seq = rand_dna(np.random.default_rng(31), 1_000_000)
    d = torch.frombuffer(bytearray(seq), dtype=torch.uint8).cuda()
    got = smd.DeviceSketcher(31, 1000).sketch(d).cpu().numpy().view(np.uint64)
    want = oracle.sketch_dna_bulk(seq, 31, scaled=1000)
    assert 800 < len(want) < 1200
    assert np.array_equal(got, want)


def test_every_tile_dirty(env):
    "3 x 10^5 bases with a newline every 150: every tile rebuilds its bad-byte masks"
    torch, smd = env
    s = bytearray(rand_dna(np.random.default_rng(150), 300_000))
    s[149::150] = b"\n" * len(s[149::150])
    seq = bytes(s)
    for scaled in (1, 1000):
        assert np.array_equal(_kernel_only(torch, smd, seq, 31, scaled), _oracle_kept(smd, seq, 31, scaled)), scaled
