"""GPU parity of sourmash_amd.Nodegraph (csrc/nodegraph.hip) through every bulk entry point -- queued add_sequence,
add_device, add_file, update_many / matches_many over a SketchSet, and the device paths of update / matches -- against
tables built in numpy from a vectorised model of khmer's two-bit hash, and against the SBT internal nodes khmer wrote.
Run with -m gpu."""
import gzip
import os

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

NG = golden("nodegraph")
SBT = os.path.join(NG, "sbt_v3")
LEAVES = {6: "6d6e87e1154e95b279e5e7db414bc37b", 7: "60f7e23c24a8d94791cc7a8680c493f9", 8: "0107d767a345eff67ecdaed2ee5cd7ba",
          9: "f71e78178af9e45e6f1d87a0c53c465c", 10: "f0c834bc306651d2b9321fb21d3e8d8f",
          11: "4e94e60265e04f0763142e20b52c0da1", 12: "b59473c94ff2889eca5d7165936e64b3"}
KS = [1, 2, 3, 15, 16, 17, 21, 31, 32]
GRAPHS = [(100000, 4), (10**7, 4), (1000, 8)]


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    assert sourmash_amd.gpu_available(), "these tests need a real GPU"
    return sourmash_amd


def _leaves_under(i):
    return [i] if i in LEAVES else _leaves_under(2 * i + 1) + _leaves_under(2 * i + 2)


def _leaf_mh(sm, i):
    with open(os.path.join(SBT, LEAVES[i])) as f:
        return list(sm.load_signatures_from_json(f.read()))[0].minhash


def _read(path):
    with open(path, "rb") as f:
        return f.read()


# ---- the numpy model ----------------------------------------------------------------------------------------------------------
_LUT = np.full(256, 255, dtype=np.uint8)
for _c, _v in zip(b"ATCG", range(4)):
    _LUT[_c] = _LUT[_c + 32] = _v


def kmer_hashes(seq, k, chunk=1 << 23):
    "canonical two-bit hashes of every k-mer of seq (bytes or uint8 array) made of ACGTacgt only"
    a = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else seq
    out = []
    for lo in range(0, max(len(a) - k + 1, 0), chunk):
        hi = min(lo + chunk + k - 1, len(a))
        c = _LUT[a[lo:hi]]
        n = hi - lo - k + 1
        bad = np.concatenate([[0], np.cumsum(c == 255)])
        ok = (bad[k:k + n] - bad[:n]) == 0
        code = np.where(c == 255, 0, c).astype(np.uint64)
        fw = np.zeros(n, dtype=np.uint64)
        rv = np.zeros(n, dtype=np.uint64)
        for j in range(k):
            fw = (fw << np.uint64(2)) | code[j:j + n]
            rv |= (code[j:j + n] ^ np.uint64(1)) << np.uint64(2 * j)
        out.append(np.minimum(fw, rv)[ok])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


def model_tables(hashes, sizes):
    "the bytes of every table (size / 8 + 1 each) and the bits set in table 0"
    tabs, occ = [], None
    for t, size in enumerate(sizes):
        bits = np.zeros(size, dtype=bool)
        if len(hashes):
            bits[(hashes % np.uint64(size)).astype(np.int64)] = True
        packed = np.packbits(bits, bitorder="little")
        nb = size // 8 + 1
        tabs.append(np.concatenate([packed, np.zeros(nb - len(packed), dtype=np.uint8)]).tobytes())
        if t == 0:
            occ = int(bits.sum())
        del bits
    return tabs, occ


def graph_tables(g):
    raw = memoryview(g.to_bytes(0))
    pos, tabs = 19, []
    for size in g.hashsizes():
        assert int.from_bytes(raw[pos:pos + 8], "little") == size
        pos += 8
        tabs.append(bytes(raw[pos:pos + size // 8 + 1]))
        pos += size // 8 + 1
    return tabs


def assert_model(g, hashes):
    tabs, occ = model_tables(hashes, g.hashsizes())
    got = graph_tables(g)
    for t, (a, b) in enumerate(zip(got, tabs)):
        assert a == b, f"table {t} differs"
    assert g.n_occupied() == occ


def rand_records(rng, n_records, lo=0, hi=3000):
    recs = []
    for _ in range(n_records):
        n = int(rng.integers(lo, hi))
        s = rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=n, p=[.23, .23, .23, .23, .02, .02, .02, .01, .01])
        if n > 100 and rng.random() < 0.3:
            p = int(rng.integers(0, n - 50))
            s[p:p + int(rng.integers(1, 50))] = ord("N")
        recs.append(s.tobytes())
    return recs


def all_hashes(recs, k):
    return np.concatenate([kmer_hashes(r, k) for r in recs] + [np.zeros(0, dtype=np.uint64)])


# ---- SBT and khmer fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(6))
def test_update_many_of_leaves_gives_internal_node(sm, i):
    g = sm.Nodegraph(1, 100000, 4)
    leaves = [_leaf_mh(sm, j) for j in _leaves_under(i)]
    g.update_many(leaves)
    assert g.to_bytes(0) == _read(os.path.join(SBT, f"internal.{i}"))
    assert list(g.matches_many(leaves)) == [len(mh.hashes) for mh in leaves]


def test_add_sequence_gives_khmer_file(sm):
    g = sm.Nodegraph(3, 23, 6)
    g.add_sequence("ACGA")
    g.add_sequence("TTA")
    assert g.to_bytes(0) == _read(os.path.join(NG, "khmer_3_23_6.ng"))


# ---- k-mer parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,n_tables", GRAPHS)
@pytest.mark.parametrize("k", KS)
def test_add_sequence_and_add_device_parity(sm, k, size, n_tables):
    import torch
    rng = np.random.default_rng(k * 1000 + n_tables)
    recs = rand_records(rng, 40)
    want = all_hashes(recs, k)
    g = sm.Nodegraph(k, size, n_tables)
    for r in recs:
        g.add_sequence(r, force=True)
    assert_model(g, want)
    d = sm.Nodegraph(k, size, n_tables)
    buf = b"\n".join(recs)
    d.add_device(torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda())
    assert_model(d, want)
    # unaligned start
    e = sm.Nodegraph(k, size, n_tables)
    e.add_device(torch.frombuffer(bytearray(b"\n" * 3 + buf), dtype=torch.uint8).cuda()[3:])
    assert graph_tables(e) == graph_tables(d) and e.n_occupied() == d.n_occupied()


@pytest.mark.parametrize("k", [1, 17, 31, 32])
def test_big_table_parity(sm, k):
    "one table of 4,294,967,311 bits: 64-bit bins and a divisor above 2^32"
    import torch
    rng = np.random.default_rng(k)
    recs = rand_records(rng, 30, 1000, 20000)
    g = sm.Nodegraph(k, 2**32 + 16, 1)
    assert g.hashsizes() == [4294967311]
    g.add_device(torch.frombuffer(bytearray(b"\n".join(recs)), dtype=torch.uint8).cuda())
    h = all_hashes(recs, k)
    raw = graph_tables(g)[0]
    bins = np.unique(h % np.uint64(4294967311))
    got = np.frombuffer(raw, dtype=np.uint8)
    nz = np.flatnonzero(got)
    set_bits = (nz[:, None] * 8 + np.flatnonzero(np.ones(8))[None, :])[(got[nz, None] >> np.arange(8)) & 1 == 1]
    assert np.array_equal(np.sort(set_bits).astype(np.uint64), bins)
    assert g.n_occupied() == len(bins)


def _write_fastx(path, recs, fmt, gz):
    lines = []
    for i, r in enumerate(recs):
        if fmt == "fa":
            lines.append(b">r%d\n%s\n" % (i, r))
        else:
            lines.append(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    data = b"".join(lines)
    with open(path, "wb") as f:
        f.write(gzip.compress(data) if gz else data)


@pytest.mark.parametrize("fmt,gz", [("fa", False), ("fq", False), ("fa", True), ("fq", True)])
@pytest.mark.parametrize("k,size,n_tables", [(21, 100000, 4), (31, 10**7, 4), (3, 1000, 8), (32, 10**7, 4)])
def test_add_file_parity(sm, tmp_path, monkeypatch, fmt, gz, k, size, n_tables):
    monkeypatch.setenv("SMG_INGEST_CHUNK", "4096")
    rng = np.random.default_rng(k + size)
    recs = [r for r in rand_records(rng, 60, 1, 4000) if r]
    path = str(tmp_path / ("x." + fmt + (".gz" if gz else "")))
    _write_fastx(path, recs, fmt, gz)
    g = sm.Nodegraph(k, size, n_tables)
    n_rec, n_bases = g.add_file(path)
    assert n_rec == len(recs) and n_bases == sum(len(r) for r in recs)
    assert_model(g, all_hashes(recs, k))


# ---- API contracts ---------------------------------------------------------------------------------------------------------------
def test_force_false_counts_prefix_then_raises(sm):
    g = sm.Nodegraph(5, 100000, 4)
    seq = "ACGTTGCAacgtAGGT" + "N" + "CCCCGGGGTTTT"
    with pytest.raises(ValueError):
        g.add_sequence(seq)
    assert_model(g, kmer_hashes(seq[:16].encode(), 5))
    h = sm.Nodegraph(5, 100000, 4)
    h.add_sequence(seq, force=True)
    assert_model(h, kmer_hashes(seq.encode(), 5))


def test_count_interleaved_with_queued_records(sm):
    rng = np.random.default_rng(3)
    recs = rand_records(rng, 20, 10, 500)
    g = sm.Nodegraph(11, 1000, 3)
    host = sm.Nodegraph(11, 1000, 3)
    for r in recs:
        g.add_sequence(r, force=True)
        for h in kmer_hashes(r, 11).tolist():
            host.count(h)
        x = int(rng.integers(0, 2**64, dtype=np.uint64))
        x2 = int(kmer_hashes(r, 11)[0]) if len(kmer_hashes(r, 11)) else x
        for v in (x, x2):
            assert g.count(v) == host.count(v)
    assert g.to_bytes(0) == host.to_bytes(0)
    assert g.n_occupied() == host.n_occupied()


def test_bulk_k_above_32_raises(sm, tmp_path):
    import torch
    g = sm.Nodegraph(33, 1000, 2)
    with pytest.raises(ValueError, match="32"):
        g.add_sequence("ACGT" * 20)
    with pytest.raises(ValueError, match="32"):
        g.add_device(torch.zeros(100, dtype=torch.uint8).cuda())
    g.count("ACGT" * 20)                 # the single-k-mer path takes any length
    assert g.get("ACGT" * 20) == 1


def _random_sketches(sm, rng, n, max_len):
    lens = np.minimum(rng.exponential(1500, size=n).astype(np.int64), max_len)
    lens[:3] = [0, max_len, 1]
    mhs = []
    for L in lens:
        mh = sm.MinHash(0, 21, scaled=1)
        if L:
            mh.add_many(np.unique(rng.integers(0, 2**62, size=int(L), dtype=np.uint64) * np.uint64(3)).tolist())
        mhs.append(mh)
    return mhs


def test_update_many_and_matches_many(sm):
    from sourmash_amd.index import SketchSet
    rng = np.random.default_rng(5)
    mhs = _random_sketches(sm, rng, 10000, 20000)
    for size, nt in [(100000, 4), (10**7, 3)]:
        g = sm.Nodegraph(21, size, nt)
        g.update_many(SketchSet(mhs[:5000]))
        host = sm.Nodegraph(21, size, nt)
        for mh in mhs[:5000]:
            host.update(mh)
        allh = np.concatenate([np.array(mh.hashes, dtype=np.uint64) for mh in mhs[:5000]])
        assert_model(g, allh)
        assert g.to_bytes(0) == host.to_bytes(0)
        got = g.matches_many(mhs)
        assert got.dtype == np.uint64 and len(got) == len(mhs)
        assert got.tolist() == [host.matches(mh) for mh in mhs]


def test_large_sketch_device_paths(sm):
    rng = np.random.default_rng(9)
    hs = np.unique(rng.integers(0, 2**64 - 1, size=100000, dtype=np.uint64))
    big = sm.MinHash(0, 21, scaled=1)
    big.add_many(hs.tolist())
    assert len(big) >= 65536
    g = sm.Nodegraph(21, 10**6, 4)
    g.update(big)                           # hash kernel
    host = sm.Nodegraph(21, 10**6, 4)
    for part in np.array_split(hs, 4):      # < 65536 hashes each: host path
        mh = sm.MinHash(0, 21, scaled=1)
        mh.add_many(part.tolist())
        host.update(mh)
    assert g.to_bytes(0) == host.to_bytes(0)
    assert_model(g, hs)
    probe = sm.MinHash(0, 21, scaled=1)
    probe.add_many(np.concatenate([hs[:50000], rng.integers(0, 2**64 - 1, size=60000, dtype=np.uint64)]).tolist())
    want = sum(host.get(int(h)) for h in probe.hashes)
    assert g.matches(probe) == want        # matches kernel
    assert g.matches_many([probe]).tolist() == [want]


def test_1e8_resident_bases(sm):
    import torch
    n = 10**8
    gen = torch.Generator(device="cuda").manual_seed(31)
    codes = torch.randint(0, 64, (n,), device="cuda", dtype=torch.uint8, generator=gen)
    lut = torch.tensor(list(b"ACGT" * 15 + b"acgN"), dtype=torch.uint8, device="cuda")
    seq = lut[codes.long()]
    g = sm.Nodegraph(31, 10**9, 4)
    g.add_device(seq)
    host_seq = seq.cpu().numpy()
    del codes, seq
    assert_model(g, kmer_hashes(host_seq, 31))
