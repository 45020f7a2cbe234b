"""GPU parity of the appending sketch kernel's tile hand-out (sketch_kernel.hpp: a workgroup's first tile is its index, every
later one comes by ticket from the launch's own counter) through DeviceSketcher.kernel_only(..., grid=g), which launches exactly g
workgroups: many tiles per workgroup on a few hundred kilobytes.  Two references: the sorted distinct values against
oracle.sketch_dna_bulk, the multiset against the library's own per-position form (MinHash.seq_to_hashes) filtered by
1 <= h <= max_hash.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import oracle
from test_gpu_sketch_dense_input import env  # noqa: F401  (env is the fixture)
from test_gpu_tile_edges import device_view

pytestmark = pytest.mark.gpu

TILE = 3 * 4096                # positions of a tile of three rounds (k >= 19 at scaled = 64); one round is 4,096
SCALED = 64                    # the long tile is still taken (kmer_core.hpp, sk_tile_rounds) and the sink flushes every few tiles
FORTY = 40 * TILE              # 40 long tiles (120 short ones): on 3 workgroups 37 (117) of them are reached by ticket


@functools.lru_cache(maxsize=None)
def dna(n, seed=0, newline_every=0):
    rng = np.random.default_rng(900 + n + seed)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    if newline_every:
        s[newline_every - 1::newline_every] = ord("\n")
    return s.tobytes()


@functools.lru_cache(maxsize=None)
def want_set(seq, k, scaled):
    return oracle.sketch_dna_bulk(seq, k, scaled=scaled)


@functools.lru_cache(maxsize=None)
def want_multiset(seq, k, scaled):
    "every kept hash, duplicates included, sorted: the per-position form of the library, which has no tiles handed out"
    import sourmash_amd as sm
    hs = np.array(sm.MinHash(0, k, scaled=1).seq_to_hashes(seq, force=True, bad_kmers_as_zeroes=True), dtype=np.uint64)
    max_hash = np.uint64(oracle.max_hash_for_scaled(scaled)) if scaled > 1 else np.uint64(2**64 - 1)
    return np.sort(hs[(hs >= 1) & (hs <= max_hash)])


def launch(torch, smd, view, k, scaled, grid):
    "one launch, not waited for -> (out, count)"
    out = torch.zeros(view.numel() + 16, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    smd.DeviceSketcher(k, scaled).kernel_only(view, out, cnt, grid=grid)
    return out, cnt


def collect(out, cnt, n):
    kept = int(cnt[0].item())
    assert kept <= n
    return np.sort(out[:kept].cpu().numpy().view(np.uint64))


def got(torch, smd, view, k, scaled, grid):
    out, cnt = launch(torch, smd, view, k, scaled, grid)
    torch.cuda.synchronize()
    return collect(out, cnt, view.numel())


def check(torch, smd, seq, k, scaled, grid, off=0, what=None):
    g = got(torch, smd, device_view(torch, seq, off), k, scaled, grid)
    assert np.array_equal(g, want_multiset(seq, k, scaled)), ("multiset", k, scaled, grid, off, what)
    assert np.array_equal(np.unique(g), want_set(seq, k, scaled)), ("set", k, scaled, grid, off, what)
    return g


@pytest.mark.parametrize("tiles", [1, 2, 3, 7])
def test_k31_tiles_and_grids(env, tiles):
    "1, 2, 3 and 7 tiles, a base short of the seam, on it and a base behind it, on 1, 2, 3 and 8 workgroups"
    torch, smd = env
    for d in (-1, 0, 1):
        seq = dna(tiles * TILE + d)
        assert len(want_multiset(seq, 31, SCALED)) > 100 * tiles
        for grid in (1, 2, 3, 8):
            check(torch, smd, seq, 31, SCALED, grid, what=(tiles, d))


@pytest.mark.parametrize("k", [31, 21, 51, 88, 12, 18, 5])
def test_forty_tiles_on_three_workgroups(env, k):
    "three rounds (k = 21, 31, 51, 88), one round staged (12) and at a register step (18), unstaged (5)"
    torch, smd = env
    g = check(torch, smd, dna(FORTY), k, SCALED, 3)
    assert len(g) > FORTY // SCALED // 2


def test_dense_output(env):
    "scaled = 1: the launcher falls to one round, every k-mer is kept and the sink spills within every tile"
    torch, smd = env
    seq = dna(30 * 4096 + 5)
    g = check(torch, smd, seq, 31, 1, 3)
    assert len(g) == len(seq) - 30


def test_bad_bytes(env):
    "a newline every 150 bytes: every tile is dirty, the k-mers over a newline are dropped"
    torch, smd = env
    seq = dna(FORTY, newline_every=150)
    g = check(torch, smd, seq, 31, SCALED, 3)
    assert 0 < len(g) < len(want_multiset(dna(FORTY), 31, SCALED))


@pytest.mark.parametrize("off", [1, 15])
def test_alignment(env, off):
    "the buffer starts 1 and 15 bytes behind a 16-byte boundary: the blanked prefix belongs to tile 0 alone"
    torch, smd = env
    check(torch, smd, dna(FORTY), 31, SCALED, 3, off=off)
    check(torch, smd, dna(7 * TILE - off), 31, SCALED, 2, off=off)      # the prefix makes it 7 tiles exactly


def test_counter_lifetime_one_stream(env):
    "three launches back to back on one stream, nothing waited for in between: each has its own zeroed counter"
    torch, smd = env
    seq = dna(FORTY)
    view = device_view(torch, seq, 0)
    single = got(torch, smd, view, 31, SCALED, 3)
    assert np.array_equal(single, want_multiset(seq, 31, SCALED))
    runs = [launch(torch, smd, view, 31, SCALED, grid) for grid in (3, 3, 2)]
    torch.cuda.synchronize()
    for out, cnt in runs:
        assert np.array_equal(collect(out, cnt, len(seq)), single)


def test_counter_lifetime_two_streams(env):
    "the same launch on two streams at once: neither sees the other's counter"
    torch, smd = env
    seq = dna(FORTY)
    view = device_view(torch, seq, 0)
    single = got(torch, smd, view, 31, SCALED, 3)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        for s in streams:
            with torch.cuda.stream(s):
                runs.append(launch(torch, smd, view, 31, SCALED, 3))
    torch.cuda.synchronize()
    for out, cnt in runs:
        assert np.array_equal(collect(out, cnt, len(seq)), single)


def test_whole_path_default_grid(env):
    "DeviceSketcher.sketch on 2 x 10^8 bases, 16,276 tiles of 12,288 positions: more tiles than any grid, so tickets are taken"
    torch, smd = env
    seq = oracle.synth_dna(0, 200_000_000, seed=7)
    assert len(seq) // TILE == 16_276
    want = oracle.sketch_dna_bulk(seq, 31, scaled=1000, nthreads=16)
    have = smd.DeviceSketcher(31, 1000).sketch(torch.from_numpy(seq).cuda()).cpu().numpy().view(np.uint64)
    assert len(want) > 190_000
    assert np.array_equal(have, want)
