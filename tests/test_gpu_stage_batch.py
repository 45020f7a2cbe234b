"""GPU parity of the appending sketch kernel's batched tile staging (sketch_kernel.hpp: sk_stage_batched; kmer_core.hpp:
stage_batch_ok, stage_lane_batched): a tile of all the kernel's rounds that lies wholly inside the buffer is staged with all of
a lane's loads issued at once, every other tile -- the last one, the first behind an alignment prefix, every tile of a one-round
launch -- by the loop.  Inputs of at most 50 KB: exactly 1, 2 and 3 tiles of 16,384 positions, each - 1, + 1 and + 30 bytes, and
+ 32 and + 96 bytes, where the staged chunks of the last whole tile end exactly with the buffer at k = 19 and 31 (1,026 chunks)
and at k = 88 (1,030); device pointers 0, 1 and 15 bytes behind a 16-byte boundary, a separator on chunk and tile seams, and a
newline every 150 bytes, which makes every tile dirty.  DeviceSketcher.sketch against oracle.sketch_dna_bulk at scaled = 1,000
and at scaled = 1 (the one-round path), and the same buffers through kernel_only(grid = 1) and kernel_only(grid = 2), where one
workgroup walks every tile or every other one by ticket, batched and looped, clean and dirty tiles in turn, the kept multiset
against the oracle's.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import oracle
from test_gpu_sketch_dense_input import _oracle_kept, env  # noqa: F401  (env is the fixture)
from test_gpu_tile_edges import device_view
from test_gpu_tile_handout import got as kernel_got

pytestmark = pytest.mark.gpu

TILE = 16384                   # 2 rounds of 256 lanes x 32 positions (k = 19, 31, 88); k = 37 and 55 walk 3 x 4,096
KS = [19, 31, 37, 55, 88]
SCALEDS = [1000, 1]
OFFSETS = [0, 1, 15]
LENGTHS = [t * TILE + d for t in (1, 2, 3) for d in (-1, 0, 1, 30, 32, 96)]
LONG = 3 * TILE + 30


@functools.lru_cache(maxsize=None)
def dna(n, seed=0):
    rng = np.random.default_rng(4100 + n + seed)
    return np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, 8, size=n)].tobytes()


@functools.lru_cache(maxsize=None)
def cases():
    "name -> (bytes, pointer offsets)"
    out = {"random_%d" % n: (dna(n), OFFSETS) for n in LENGTHS}
    for off in OFFSETS:
        # separators on the walk's seams (it starts `off` bytes in front of the buffer): the last byte of a chunk and the first of
        # the next, either side of both tile seams, of the 12,288-position seams of k = 37 and 55, and of a round seam
        s = bytearray(dna(LONG, seed=1))
        for at in (16 * 100 + 15, 16 * 201, 8192 - 1, 12288, TILE - 1, 2 * TILE, 2 * 12288 - 1, 3 * TILE):
            s[at - off] = ord("\n") if at % 2 else ord("N")
        out["seams_off%d" % off] = (bytes(s), [off])
    s = bytearray(dna(LONG, seed=2))
    s[149::150] = b"\n" * len(s[149::150])
    out["newline_every_150"] = (bytes(s), OFFSETS)
    return out


@functools.lru_cache(maxsize=None)
def want_sketch(seq, k, scaled):
    return oracle.sketch_dna_bulk(seq, k, scaled=scaled)


@functools.lru_cache(maxsize=None)
def want_kept(seq, k, scaled):
    from sourmash_amd import device as smd
    return _oracle_kept(smd, seq, k, scaled)


@pytest.mark.parametrize("scaled", SCALEDS)
@pytest.mark.parametrize("k", KS)
def test_sketch(env, k, scaled):
    "the whole step on every input and pointer offset"
    torch, smd = env
    kept = 0
    for name, (seq, offs) in cases().items():
        w = want_sketch(seq, k, scaled)
        kept += len(w)
        for off in offs:
            have = smd.DeviceSketcher(k, scaled).sketch(device_view(torch, seq, off)).cpu().numpy().view(np.uint64)
            assert np.array_equal(have, w), (k, scaled, name, off)
    assert kept > (300 if scaled == 1000 else 300_000)


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("scaled", SCALEDS)
@pytest.mark.parametrize("k", KS)
def test_few_workgroups_walk_many_tiles(env, k, scaled, grid):
    "exactly `grid` workgroups: tiles by ticket, clean and dirty tiles in turn on one workgroup; every appended hash with duplicates"
    torch, smd = env
    for name, (seq, offs) in cases().items():
        if len(seq) < 2 * TILE:
            continue                                               # the shorter ones have a single tile at k = 31
        w = want_kept(seq, k, scaled)
        for off in offs:
            have = kernel_got(torch, smd, device_view(torch, seq, off), k, scaled, grid)
            assert np.array_equal(have, w), (k, scaled, grid, name, off)
