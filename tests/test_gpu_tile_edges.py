"""GPU parity of every DNA k-mer kernel family on the smallest inputs on which a wrong tile stager, window read-back or LDS
flush shows (csrc/kmer_core.hpp: stage_tile, read_window, LdsSink; csrc/tile_launch.hpp: align_to_tiles).  A tile is 4,096 start
positions: the lengths sit on either side of a 16-byte chunk, of a tile, of a tile plus its halo, and reach a second seam; the
device pointer sits 0, 1 and 15 bytes behind a 16-byte boundary wherever the entry point takes a device tensor.  Expected values
come from the CPU oracle through the helpers of each family's own GPU test.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import oracle
from test_gpu_hll import _hll, _regs, _want as hll_want
from test_gpu_ingest import _oracle_sig
from test_gpu_nodegraph import assert_model, kmer_hashes as ng_hashes
from test_gpu_records import check as records_check, sm  # noqa: F401  (sm is the fixture)
from test_gpu_sketch_dense_input import _oracle_kept, env  # noqa: F401  (env is the fixture)

pytestmark = pytest.mark.gpu

TILE = 4096
OFFSETS = [0, 1, 15]
TWO_TILES = 2 * TILE + 5


def lengths(k):
    return sorted({0, k - 1, k, 15, 16, 17, TILE - 1, TILE, TILE + 1, TILE + k - 1, TWO_TILES})


def scaled_for(n):
    "every k-mer kept on the short inputs (a single k-mer must show); about 500 a tile on the long ones (flushes between tiles)"
    return 1 if n < TILE - 1 else 8


@functools.lru_cache(maxsize=None)
def content(n):
    "random ACGT; an N on the last byte of the first tile; a lower-case stretch across the tile seam (and its shifted places)"
    rng = np.random.default_rng(1000 + n)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    lo, hi = min(TILE - 30, n), min(TILE + 20, n)
    s[lo:hi] |= 0x20
    if n >= TILE:
        s[TILE - 1] = ord("N")
    return s.tobytes()


def device_view(torch, seq, off):
    "seq on the device, its first byte `off` bytes behind a 16-byte boundary (an empty tensor has no address: torch gives 0)"
    base = torch.zeros(len(seq) + 32, dtype=torch.uint8, device="cuda")
    view = base[off:off + len(seq)]
    if len(seq):
        view.copy_(torch.frombuffer(bytearray(seq), dtype=torch.uint8))
        assert view.data_ptr() % 16 == off
    return view


# ---- the appending forms: register window (k = 8 unstaged, 20 unstaged at a register edge, 31 staged), run-time k (100) ---------
@functools.lru_cache(maxsize=None)
def want_appended(n, k, scaled):
    from sourmash_amd import device as smd
    return _oracle_kept(smd, content(n), k, scaled) if n >= k else np.zeros(0, dtype=np.uint64)


def got_appended(torch, smd, view, k, scaled):
    "every hash the kernel appends (duplicates kept), sorted"
    out = torch.zeros(view.numel() + 16, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    smd.DeviceSketcher(k, scaled).kernel_only(view, out, cnt)
    torch.cuda.synchronize()
    kept = int(cnt[0].item())
    assert kept <= view.numel()
    return np.sort(out[:kept].cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("k", [8, 20, 31, 100])
def test_appending_sketch(env, k):
    torch, smd = env
    for n in lengths(k):
        want = want_appended(n, k, scaled_for(n))
        assert (len(want) > 0) == (n >= k), n
        for off in OFFSETS:
            got = got_appended(torch, smd, device_view(torch, content(n), off), k, scaled_for(n))
            assert np.array_equal(got, want), (n, off)


@pytest.mark.parametrize("k", [8, 20, 31, 100])
def test_appending_sketch_spills(env, k):
    "scaled = 1: 4,096 kept hashes a tile against 2,048 LDS entries: the spill branch, a flush between the tiles, the last flush"
    torch, smd = env
    want = want_appended(TWO_TILES, k, 1)
    assert len(want) > TILE
    for off in OFFSETS:
        assert np.array_equal(got_appended(torch, smd, device_view(torch, content(TWO_TILES), off), k, 1), want), off


# ---- the per-position form ------------------------------------------------------------------------------------------------------
def test_per_position(sm):
    k = 31
    mh = sm.MinHash(0, k, scaled=1)
    for n in lengths(k):
        s = content(n)
        want = [h or 0 for h in oracle.seq_to_hashes(s, k, force=True, bad_kmers_as_zeroes=True)] if n >= k else []
        assert any(want) == (n >= k), n
        assert mh.seq_to_hashes(s.decode(), force=True, bad_kmers_as_zeroes=True) == want, n


# ---- k = 21 / 31 / 51 in one pass, through the file ingest --------------------------------------------------------------------------
def _multi(tmp_path, n, scaled):
    from sourmash_amd.sketch import sketch_file
    s = content(n).decode()
    path = tmp_path / f"n{n}_s{scaled}.fa"
    path.write_text(f">r\n{s}\n")
    sig, = sketch_file(str(path), f"k=21,k=31,k=51,scaled={scaled},abund")
    mhs = list(sig.minhashes())
    assert [mh.ksize for mh in mhs] == [21, 31, 51]
    for mh in mhs:
        want = _oracle_sig([("r", s)], mh.ksize, scaled=scaled, abund=True)
        assert (len(want.mins) > 0) == (n >= mh.ksize), (n, mh.ksize)
        assert np.array_equal(mh._mins_array(), want.mins), (n, mh.ksize)
        assert list(mh.hashes.values()) == want.abunds.tolist(), (n, mh.ksize)


def test_three_ksizes_in_one_pass(sm, tmp_path):
    for n in sorted(set(lengths(21)) | set(lengths(31)) | set(lengths(51))):
        _multi(tmp_path, n, scaled_for(n))


def test_three_ksizes_in_one_pass_spills(sm, tmp_path):
    "scaled = 1: each ksize's 1,024 LDS entries overflow within a tile"
    _multi(tmp_path, TWO_TILES, 1)


# ---- HyperLogLog: registers in LDS (p = 10) and in device memory (p = 15) -----------------------------------------------------------
@pytest.mark.parametrize("p", [10, 15])
def test_hll(sm, p):
    import torch
    k = 21
    for n in lengths(k):
        want = hll_want([content(n)], k, p)
        assert want.any() == (n >= k), n
        for off in OFFSETS:
            h = _hll(sm, k, p)
            h.add_device(device_view(torch, content(n), off))
            assert np.array_equal(_regs(h), want), (n, off)


# ---- Nodegraph: tables in LDS (4 x 100,000 bits) and in device memory (2 x 1,000,000 bits) -------------------------------------------
@pytest.mark.parametrize("size,n_tables", [(100_000, 4), (1_000_000, 2)])
def test_nodegraph(sm, size, n_tables):
    import torch
    k = 21
    for n in lengths(k):
        want = ng_hashes(content(n), k)
        assert (len(want) > 0) == (n >= k), n
        for off in OFFSETS:
            g = sm.Nodegraph(k, size, n_tables)
            g.add_device(device_view(torch, content(n), off))
            assert_model(g, want)


# ---- one sketch per record: two records, the first empty on the short inputs so that the second holds a k-mer --------------------
def _two_records(n, k):
    return [0, n - 3 * k if n >= 4 * k else 0, n]


def test_sketch_records(sm):
    import torch
    k = 21
    for n in lengths(k):
        buf = np.frombuffer(content(n), dtype=np.uint8)
        for off in OFFSETS:
            want_h, _, _ = records_check(sm, buf, _two_records(n, k), k, scaled_for(n), seq_t=device_view(torch, content(n), off))
            assert (len(want_h) > 0) == (n >= k), n


def test_sketch_records_spills(sm):
    "scaled = 1: 4,096 (hash, position) pairs a tile against 1,024 LDS entries"
    import torch
    buf = np.frombuffer(content(TWO_TILES), dtype=np.uint8)
    for off in OFFSETS:
        want_h, _, _ = records_check(sm, buf, _two_records(TWO_TILES, 21), 21, 1, seq_t=device_view(torch, content(TWO_TILES), off))
        assert len(want_h) > TILE
