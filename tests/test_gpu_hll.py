"""GPU parity of the HyperLogLog registers (csrc/hll.hip) through every entry point -- the queued add_sequence, add_device,
add_file and the long-k route -- against registers built in numpy from the oracle's per-k-mer hashes, plus the constants
of the reference's HLL tests.  Run with -m gpu."""
import gzip

import numpy as np
import pytest

import oracle
from conftest import golden

pytestmark = pytest.mark.gpu

KS = [1, 2, 15, 16, 21, 31, 32, 33, 51, 64, 65, 88, 89, 128, 200]
PS = [4, 10, 14, 16, 18]


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    assert sourmash_amd.gpu_available(), "these tests need a real GPU"
    return sourmash_amd


def _hashes(buf, k):
    "nonzero canonical k-mer hashes (seed 42) of buf, bad k-mers skipped (force = true)"
    b = bytes(buf)
    if len(b) < k:
        return np.zeros(0, dtype=np.uint64)
    out = np.zeros(len(b) - k + 1, dtype=np.uint64)
    r = oracle.lib().orc_seq_to_hashes_dna(b, len(b), k, 42, 1, oracle._ptr(out))
    out = out[:r]
    return out[out != 0]


def _fold(regs, hs, p):
    "regs[h & (2^p-1)] = max(regs, clz64(h >> p) + 1 - p)"
    if hs.size == 0:
        return regs
    v = hs >> np.uint64(p)
    bitlen = np.zeros(v.shape, dtype=np.int64)
    t = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = t >= (np.uint64(1) << np.uint64(s))
        bitlen[big] += s
        t[big] >>= np.uint64(s)
    bitlen[t > 0] += 1
    rank = (64 - bitlen + 1 - p).astype(np.uint8)
    idx = (hs & np.uint64((1 << p) - 1)).astype(np.int64)
    np.maximum.at(regs, idx, rank)
    return regs


def _want(records, k, p):
    regs = np.zeros(1 << p, dtype=np.uint8)
    for r in records:
        _fold(regs, _hashes(r, k), p)
    return regs


def _hll(sm, k, p):
    "an empty counter of 2^p registers at ksize k (made through the file format, which keeps k in one byte)"
    from sourmash_amd.hll import HLL
    assert 0 < k < 256
    return HLL.from_buffer(b"HLL" + bytes([1, p, 64 - p, k]) + bytes(1 << p))


def _regs(h):
    return np.frombuffer(h.registers(), dtype=np.uint8)


def _records(seed, n=40):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        L = int(rng.integers(0, 3000)) if i % 5 else int(rng.integers(0, 40))
        s = rng.choice(np.frombuffer(b"ACGTacgt", dtype=np.uint8), size=L)
        if L and i % 3 == 0:
            for _ in range(int(rng.integers(1, 6))):
                s[int(rng.integers(0, L))] = ord(rng.choice(list("NRYKMnx")))
        recs.append(s.tobytes())
    return recs


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("p", PS)
def test_registers_equal_oracle(sm, k, p):
    recs = _records(k * 100 + p)
    h = _hll(sm, k, p)
    for r in recs:
        h.add_sequence(r, force=True)
    assert np.array_equal(_regs(h), _want(recs, k, p))


@pytest.mark.parametrize("k", [21, 31, 89])
def test_queue_buffer_device_agree(sm, k):
    import torch
    recs = _records(k)
    p = 12
    a = _hll(sm, k, p)
    for r in recs:
        a.add_sequence(r, force=True)
    b = _hll(sm, k, p)
    b.add_sequence(b"\n".join(recs), force=True)
    c = _hll(sm, k, p)
    c.add_device(torch.frombuffer(bytearray(b"\n".join(recs)), dtype=torch.uint8).cuda())
    ra = _regs(a)
    assert np.array_equal(ra, _regs(b)) and np.array_equal(ra, _regs(c))
    assert ra.any()


@pytest.mark.parametrize("k", [21, 100])
def test_force_false_prefix_then_raise(sm, k):
    rng = np.random.default_rng(5)
    seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=600).tobytes()
    bad = seq[:300] + b"N" + seq[301:]
    h = _hll(sm, k, 10)
    mh = sm.MinHash(0, k, scaled=1)
    with pytest.raises(ValueError) as e1:
        h.add_sequence(bad)
    with pytest.raises(ValueError) as e2:
        mh.add_sequence(bad)
    assert str(e1.value) == str(e2.value)
    assert np.array_equal(_regs(h), _want([bad[:300]], k, 10))
    h2 = _hll(sm, k, 10)
    h2.update(mh)
    assert np.array_equal(_regs(h), _regs(h2))


def _write_fasta(path, recs, fastq=False, gz=False):
    lines = []
    for i, r in enumerate(recs):
        if fastq:
            lines += [b"@r%d" % i, r, b"+", b"I" * len(r)]
        else:
            lines += [b">r%d" % i] + [r[j:j + 70] for j in range(0, len(r), 70)]
    data = b"\n".join(lines) + b"\n"
    (open(path, "wb") if not gz else gzip.open(path, "wb")).write(data)


@pytest.mark.parametrize("fmt", ["fa", "fa.gz", "fq"])
def test_add_file(sm, tmp_path, fmt):
    recs = [r for r in _records(77, 60) if r]
    f = tmp_path / ("x." + fmt)
    _write_fasta(str(f), recs, fastq=fmt == "fq", gz=fmt.endswith("gz"))
    for k in (21, 95):
        a = _hll(sm, k, 14)
        n, _ = a.add_file(str(f))
        assert n == len(recs)
        b = _hll(sm, k, 14)
        for r in recs:
            b.add_sequence(r, force=True)
        assert np.array_equal(_regs(a), _regs(b))
        assert np.array_equal(_regs(a), _want(recs, k, 14))


def test_larger_input(sm):
    import torch
    n = 100_000_000
    buf = oracle.synth_dna(0, n, seed=11, record_len=1_000_003)
    for k, p in ((21, 14), (31, 18)):
        h = _hll(sm, k, p)
        h.add_device(torch.from_numpy(buf).cuda())
        want = np.zeros(1 << p, dtype=np.uint8)
        step = 10_000_000
        for off in range(0, n, step):           # chunks cut at record separators: the k-mers of a chunk stay in it
            end = min(n, off + step)
            while end < n and buf[end] != ord("\n"):
                end += 1
            start = off
            while start > 0 and buf[start - 1] != ord("\n"):
                start -= 1
            _fold(want, _hashes(buf[start:end].tobytes(), k), p)
        assert np.array_equal(_regs(h), want)


def _reads(path):
    return [s for _, s in oracle.read_fasta(path)]


def test_reference_constants(sm):
    from sourmash_amd.hll import HLL
    genes = _reads(golden("genes", "ecoli.genes.fna"))
    h = HLL(0.01, 21)
    for s in genes:
        h.add_sequence(s)
    assert abs(1 - h.cardinality() / 3356) < 0.01
    h2 = HLL(0.01, 21)
    for s in genes[:40]:
        for i in range(len(s) - 21 + 1):
            h2.add(s[i:i + 21])
    h3 = HLL(0.01, 21)
    for s in genes[:40]:
        h3.add_sequence(s)
    assert h2.registers() == h3.registers()

    h1, h2, hu = HLL(0.01, 21), HLL(0.01, 21), HLL(0.01, 21)
    for s in _reads(golden("num", "genome-s10.fa.gz")):
        h1.add_sequence(s)
        hu.add_sequence(s)
    for s in _reads(golden("hll", "genome-s10+s11.fa.gz")):
        h2.add_sequence(s)
        hu.add_sequence(s)
    assert abs(1 - h1.cardinality() / 500741) < 0.01
    assert abs(1 - h2.cardinality() / 995845) < 0.01
    assert abs(1 - h1.similarity(h2) / 0.502783) < 0.01
    assert abs(1 - h1.containment(h2) / 1.0) < 0.01
    assert abs(1 - h2.containment(h1) / 0.502783) < 0.01
    assert abs(1 - h1.intersection(h2) / 500838) < 0.01
    f1 = HLL(0.01, 21)
    f1.add_file(golden("num", "genome-s10.fa.gz"))
    assert f1.registers() == h1.registers()


@pytest.mark.parametrize("n", [2000, 200_000])
def test_update_and_matches(sm, n):
    from sourmash_amd.hll import HLL
    mh = sm.MinHash(0, 21, scaled=1)
    buf = oracle.synth_dna(0, n, seed=3, record_len=0).tobytes()
    mh.add_sequence(buf, force=True)
    mins = np.asarray(mh._mins_array(), dtype=np.uint64)
    h = HLL(0.01, 21)
    h.update(mh)
    want = _fold(np.zeros(1 << 14, dtype=np.uint8), mins, 14)
    assert np.array_equal(_regs(h), want)
    other = HLL(0.01, 21)
    other.add_sequence(buf[: n // 2], force=True)
    ref = HLL.from_buffer(b"HLL" + bytes([1, 14, 50, 21]) + want.tobytes())
    assert other.matches(mh) == other.intersection(ref)
