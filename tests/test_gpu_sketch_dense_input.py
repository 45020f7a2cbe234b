"""GPU parity of the register-window sketch kernel on inputs that keep (nearly) every k-mer: the workgroup's LDS staging
buffer for kept hashes overflows within a single tile, so the flush path and the direct spill to HBM both run.
Run with -m gpu."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import sourmash_amd
    from sourmash_amd import device as smd
    assert sourmash_amd.gpu_available(), "these tests need a real GPU"
    return torch, smd


def _inputs():
    rng = np.random.default_rng(77)
    rand = bytearray(rng.choice(np.frombuffer(b"ACGTacgt", dtype=np.uint8), 300_000))
    for i in range(1000, len(rand), 9973):
        rand[i] = ord("N")
    rand[150_000] = ord("\n")
    return {"poly_a": b"A" * 100_000, "random": bytes(rand), "mixed": b"A" * 20_000 + bytes(rand[:50_000]) + b"N" + b"T" * 9_000}


def _kernel_only(torch, smd, seq, k, scaled):
    "every hash the kernel appends (duplicates kept), sorted"
    d = torch.frombuffer(bytearray(seq), dtype=torch.uint8).cuda()
    sk = smd.DeviceSketcher(k, scaled)
    out = torch.zeros(len(seq) + 16, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    sk.kernel_only(d, out, cnt)
    torch.cuda.synchronize()
    kept = int(cnt[0].item())
    assert kept <= len(seq)
    return np.sort(out[:kept].cpu().numpy().view(np.uint64))


def _oracle_kept(smd, seq, k, scaled):
    thr = smd.DeviceSketcher(k, scaled).max_hash             # the very threshold the kernel is given
    hs = np.array(oracle.seq_to_hashes(seq, k, seed=42, force=True), dtype=np.uint64)      # bad k-mers and zeros dropped
    return np.sort(hs[hs <= np.uint64(thr)])


@pytest.mark.parametrize("k", [21, 31, 51, 70])
@pytest.mark.parametrize("name", ["poly_a", "random", "mixed"])
def test_every_kmer_kept(env, name, k):
    "scaled = 1: 4,096 kept hashes per tile against a staging buffer of 2,048 entries: half of them spill"
    torch, smd = env
    seq = _inputs()[name]
    want = _oracle_kept(smd, seq, k, 1)
    assert len(want) > 50_000
    assert np.array_equal(_kernel_only(torch, smd, seq, k, 1), want)


@pytest.mark.parametrize("scaled", [2, 20])
def test_staging_and_spill_in_one_launch(env, scaled):
    "scaled = 2: a tile fills the staging buffer about to the brim; scaled = 20: it is flushed every few tiles, never spilled"
    torch, smd = env
    seq = _inputs()["random"]
    for k in (31, 33):
        want = _oracle_kept(smd, seq, k, scaled)
        assert len(want) > 10_000
        assert np.array_equal(_kernel_only(torch, smd, seq, k, scaled), want)


def test_sketch_of_dense_input(env):
    "the whole step (kernel + sort + unique) at scaled = 1 equals the oracle's sketch"
    torch, smd = env
    for name, seq in _inputs().items():
        d = torch.frombuffer(bytearray(seq), dtype=torch.uint8).cuda()
        got = smd.DeviceSketcher(31, 1).sketch(d).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, oracle.sketch_dna_bulk(seq, 31, scaled=1)), name
