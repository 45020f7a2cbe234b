"""GPU parity of per-record sketching (csrc/sketch_records.hip): every record of a buffer or of a file as a sketch of its own,
from the raw entry point up to `sketch_file(singleton=True)`, against rows cut in numpy from the oracle's per-k-mer hashes of
the whole buffer.  Run with -m gpu."""
import ctypes as C
import gzip

import numpy as np
import pytest

import oracle
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    import sourmash_amd.device  # noqa: F401
    import sourmash_amd.index  # noqa: F401
    import sourmash_amd.sketch  # noqa: F401
    assert sourmash_amd.gpu_available(), "these tests need a real GPU"
    return sourmash_amd


# ---- expected rows: the oracle's hashes of the whole buffer, cut by the starts ---------------------------------------------------
def dense_hashes(buf, k):
    "hash of the canonical k-mer at every start position of buf (seed 42), 0 for a k-mer with a byte outside ACGTacgt"
    b = bytes(buf)
    if len(b) < k:
        return np.zeros(0, dtype=np.uint64)
    out = np.zeros(len(b) - k + 1, dtype=np.uint64)
    r = oracle.lib().orc_seq_to_hashes_dna(b, len(b), k, 42, 1, oracle._ptr(out))
    assert r == len(out)
    return out


def expected_csr(dense, starts, k, max_hash):
    """-> (hashes, offsets, abundances): per record the sorted distinct hashes 0 < h <= max_hash of the k-mers that lie inside it
    (record of a position: the last one starting at or before it; the k-mer must end inside that record)"""
    starts = np.asarray(starts, dtype=np.int64)
    n = len(starts) - 1
    pos = np.flatnonzero((dense > 0) & (dense <= np.uint64(max_hash)))
    h = dense[pos]
    r = np.searchsorted(starts, pos, side="right") - 1
    ok = (r >= 0) & (r < n)
    ok &= pos + k <= starts[np.clip(r, 0, max(n - 1, 0)) + 1] if n else False
    r, h = r[ok], h[ok]
    order = np.lexsort((h, r))
    r, h = r[order], h[order]
    head = np.ones(len(r), dtype=bool)
    head[1:] = (r[1:] != r[:-1]) | (h[1:] != h[:-1])
    idx = np.flatnonzero(head)
    counts = np.diff(np.append(idx, len(r))).astype(np.uint64)
    offsets = np.searchsorted(r[idx], np.arange(n + 1), side="left").astype(np.uint64)
    return h[idx], offsets, counts


def to_dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def got_csr(res):
    return tuple(t.cpu().numpy().view(np.uint64) for t in res)


def check(sm, buf, starts, k, scaled, dense=None, seq_t=None):
    "flat and with abundances through DeviceSketcher.sketch_records, against the expected rows"
    import torch
    dense = dense_hashes(buf, k) if dense is None else dense
    want_h, want_o, want_a = expected_csr(dense, starts, k, oracle.max_hash_for_scaled(scaled))
    if seq_t is None:
        seq_t = to_dev(torch, np.frombuffer(bytes(buf), dtype=np.uint8))
    starts_t = to_dev(torch, np.asarray(starts, dtype=np.int64))
    sk = sm.device.DeviceSketcher(ksize=k, scaled=scaled)
    h, o = got_csr(sk.sketch_records(seq_t, starts_t))
    assert np.array_equal(o, want_o)
    assert np.array_equal(h, want_h)
    h, o, a = got_csr(sk.sketch_records(seq_t, starts_t, abund=True))
    assert np.array_equal(o, want_o) and np.array_equal(h, want_h) and np.array_equal(a, want_a)
    return want_h, want_o, want_a


# ---- 1. boundaries ---------------------------------------------------------------------------------------------------------------
def boundary_buffer(k):
    """~200 kB with hand-placed records: bytes in front of the first start; records that end / start at bytes 4095, 4096 and 4097
    (the kernel's tile is 256 x 16 start positions); two consecutive empty records; records of 1, k - 1, k, k + 1, 4095, 4096,
    4097 and 10,000 bases; records that touch with no separator byte and records that end in one; N, IUPAC and lower-case bytes;
    the last record ends exactly at len."""
    rng = np.random.default_rng(100 + k)

    def dna(n):
        return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()

    lens = [4095 - 37, 1, 1, 0, 0, 1, k - 1, k, k + 1, 4095, 4096, 4097, 10_000, 5_000, 3 * k, 30_000, 50_000, 0, 41_000]
    parts, starts = [dna(37)], [37]
    for i, n in enumerate(lens):
        rec = dna(n)
        if n >= 1000 and i % 2 == 0:
            rec[-1] = ord("\n")                                    # this record ends in a separator; the others touch the next
        if n == 5_000:
            rec[100:400] = np.frombuffer(bytes(rec[100:400]).lower(), dtype=np.uint8)
            rec[1000] = ord("N"); rec[1001] = ord("n"); rec[2000] = ord("R"); rec[2500:2503] = np.frombuffer(b"YKM", dtype=np.uint8)
            rec[3000:3000 + k] = ord("A")                          # a repeated k-mer: abundances above 1 at any scaled
            rec[3200:3200 + 2 * k] = ord("a")
        parts.append(rec)
        starts.append(starts[-1] + n)
    buf = np.concatenate(parts)
    assert starts[1] == 4095 and starts[2] == 4096 and starts[3] == 4097 and starts[-1] == len(buf)
    return buf, starts


@pytest.mark.parametrize("scaled", [1, 10, 1000])
@pytest.mark.parametrize("k", [11, 21, 31, 51, 88])
def test_boundaries(sm, k, scaled):
    buf, starts = boundary_buffer(k)
    want_h, want_o, want_a = check(sm, buf, starts, k, scaled)
    assert want_o[3] == want_o[4] == want_o[5]                             # empty records: empty rows
    assert scaled != 1 or want_a.max() > k                                # the repeated k-mer is counted
    # the oracle's own sketch of a record by itself, for the short rows
    for r in (0, 1, 7, 8, 9, 13, 15):
        rec = bytes(buf[starts[r]:starts[r + 1]])
        row = want_h[int(want_o[r]):int(want_o[r + 1])]
        assert np.array_equal(row, oracle.sketch_dna_bulk(rec, k, scaled=scaled) if len(rec) else np.zeros(0, dtype=np.uint64))


def test_unaligned_pointer(sm):
    "the device pointer 3 bytes behind a 16-byte boundary (a tensor slice)"
    import torch
    buf, starts = boundary_buffer(31)
    base = torch.zeros(len(buf) + 64, dtype=torch.uint8, device="cuda")
    view = base[3:3 + len(buf)]
    view.copy_(torch.from_numpy(buf))
    assert view.data_ptr() % 16 == 3
    check(sm, buf, starts, 31, 10, seq_t=view)


# ---- 2. many short records -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads():
    n = 100_000
    buf = oracle.synth_dna(0, n * 151, seed=7, record_len=150)
    return buf, dense_hashes(buf, 21)


@pytest.mark.parametrize("n_records,scaled", [(100_000, 100), (100_000, 1000), (1000, 1000), (500, 1000)])
def test_many_short_records(sm, reads, n_records, scaled):
    """150-base reads, starts at the separator positions.  100,000 and 1,000 records take the wide form of the sort (record and
    hash bits exceed 64: at scaled = 1000 a hash has 55 bits), 500 records the packed one."""
    buf, dense = reads
    n = n_records * 151
    starts = np.arange(n_records + 1, dtype=np.int64) * 151
    check(sm, buf[:n], starts, 21, scaled, dense=dense[:n - 20])


def test_sketchset_of_reads(sm, reads):
    import torch
    buf, dense = reads
    n_records = 2000
    n = n_records * 151
    starts = np.arange(n_records + 1, dtype=np.int64) * 151
    want_h, want_o, _ = expected_csr(dense[:n - 20], starts, 21, oracle.max_hash_for_scaled(100))
    ss = sm.index.SketchSet.sketch_records(to_dev(torch, buf[:n]), to_dev(torch, starts), ksize=21, scaled=100)
    assert len(ss) == n_records and ss.total_hashes == len(want_h)
    assert np.array_equal(ss.sizes, np.diff(want_o))
    assert ss.params == (21, "DNA", 42, 100, 0)
    for r in (0, 1, 999, 1999):
        assert np.array_equal(ss.minhash(r)._mins_array(), want_h[int(want_o[r]):int(want_o[r + 1])])


# ---- 3. files ---------------------------------------------------------------------------------------------------------------------------
def make_records(seed, n=300, empty=True):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        length = int(rng.integers(0, 20_001)) if i % 7 else int(rng.integers(0, 60))
        if i in (5, 6, n - 1):
            length = 0 if empty else 25
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=length)].copy()
        if length > 500 and i % 5 == 0:
            seq[100] = ord("N")
            seq[200:260] = np.frombuffer(bytes(seq[200:260]).lower(), dtype=np.uint8)
        if length > 100 and i % 11 == 0:
            seq[50] = ord(">")                                      # a stray '>' inside a sequence line splits nothing
        recs.append((f"rec{i} len={length} some description", bytes(seq)))
    return recs


def fasta_text(recs, width=70, eol=b"\n", last_newline=True):
    out = []
    for name, seq in recs:
        out.append(b">" + name.encode() + eol)
        for i in range(0, len(seq), width):
            out.append(seq[i:i + width] + eol)
    text = b"".join(out)
    return text if last_newline else text.rstrip(b"\r\n")


def fastq_text(recs):
    return b"".join(b"@" + n.encode() + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in recs)


FORMS = ["fasta_crlf", "fasta_no_final_newline", "fasta_empty_record", "fastq", "fasta_gz", "fastq_gz"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("records")
    with_empty, without = make_records(1), make_records(2, empty=False)
    # a '>' at a line start would be a header: keep the stray ones off the line starts (width 70, position 50)
    out = {}
    for form in FORMS:
        if form == "fasta_crlf":
            recs, data, name = without, fasta_text(without, eol=b"\r\n"), "crlf.fa"
        elif form == "fasta_no_final_newline":
            recs, data, name = without, fasta_text(without, last_newline=False), "nonl.fa"
        elif form == "fasta_empty_record":
            recs, data, name = with_empty, fasta_text(with_empty), "empty.fa"
        elif form == "fastq":
            recs, data, name = without, fastq_text(without), "reads.fq"
        elif form == "fasta_gz":
            recs, data, name = with_empty, gzip.compress(fasta_text(with_empty), 6), "empty.fa.gz"
        else:
            recs, data, name = without, gzip.compress(fastq_text(without), 6), "reads.fq.gz"
        path = d / name
        path.write_bytes(data)
        out[form] = (str(path), recs)
    return out


def rows_of_records(recs, k, scaled):
    "expected CSR of a list of (name, sequence) records: the records joined, the oracle's hashes of the whole, cut by the starts"
    buf = b"".join(s for _, s in recs)
    starts = np.concatenate([[0], np.cumsum([len(s) for _, s in recs])]).astype(np.int64)
    return expected_csr(dense_hashes(buf, k), starts, k, oracle.max_hash_for_scaled(scaled))


def assert_set_equals(ss, want_h, want_o):
    assert len(ss) == len(want_o) - 1 and ss.total_hashes == len(want_h)
    assert np.array_equal(ss.sizes, np.diff(want_o))
    for r in range(len(ss)):
        assert np.array_equal(ss.minhash(r)._mins_array(), want_h[int(want_o[r]):int(want_o[r + 1])]), r


@pytest.mark.parametrize("form", FORMS)
def test_sketchset_from_file(sm, files, form):
    path, recs = files[form]
    assert [n for n, _ in sm.sketch.read_records(path)] == [n for n, _ in recs]
    assert [s for _, s in sm.sketch.read_records(path)] == [s for _, s in recs]
    ss = sm.index.SketchSet.sketch_file(path, ksize=31, scaled=100)
    want_h, want_o, _ = rows_of_records(recs, 31, 100)
    assert_set_equals(ss, want_h, want_o)
    assert [m["name"] for m in ss.manifest] == [n for n, _ in recs]
    assert all(m["filename"] == path and m["ksize"] == 31 and m["scaled"] == 100 for m in ss.manifest)


def assert_same_signatures(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.name == b.name and a.filename == b.filename
        ma, mb = a.minhashes(), b.minhashes()
        assert len(ma) == len(mb)
        for x, y in zip(ma, mb):
            assert (x.ksize, x.scaled, x.seed, x.track_abundance, x.moltype) == (y.ksize, y.scaled, y.seed, y.track_abundance, y.moltype)
            assert x.md5sum() == y.md5sum()
            assert np.array_equal(x._mins_array(), y._mins_array())
            if x.track_abundance:
                assert x.hashes == y.hashes


@pytest.mark.parametrize("form", FORMS)
def test_singleton_signatures_from_file(sm, files, form):
    path, recs = files[form]
    params = "k=21,k=31,k=51,scaled=100,abund"
    got = sm.sketch.sketch_file(path, params, singleton=True)
    want = sm.sketch.sketch_records(list(sm.sketch.read_records(path)), params, filename=path, singleton=True)
    assert len(got) == len(recs)
    assert_same_signatures(got, want)
    # ... and the rows the oracle expects, with their abundances
    want_h, want_o, want_a = rows_of_records(recs, 51, 100)
    for r in (0, 1, 5, 150, len(recs) - 1):
        mh = got[r].minhashes()[2]
        lo, hi = int(want_o[r]), int(want_o[r + 1])
        assert mh.hashes == dict(zip(want_h[lo:hi].tolist(), want_a[lo:hi].tolist()))


def test_singleton_golden_genes(sm):
    path = golden("genes", "ecoli.genes.fna")
    recs = list(sm.sketch.read_records(path))
    assert len(recs) == 2
    params = "k=21,k=31,k=51,scaled=10,abund"
    got = sm.sketch.sketch_file(path, params, singleton=True)
    assert_same_signatures(got, sm.sketch.sketch_records(recs, params, filename=path, singleton=True))
    for q, k in enumerate((21, 31, 51)):
        for r, (_, seq) in enumerate(recs):
            assert np.array_equal(got[r].minhashes()[q]._mins_array(), oracle.sketch_dna_bulk(seq, k, scaled=10))
    ss = sm.index.SketchSet.sketch_file(path, ksize=31, scaled=10)
    assert_set_equals(ss, *rows_of_records(recs, 31, 10)[:2])


# ---- 4. downstream -------------------------------------------------------------------------------------------------------------------
def test_compare_and_search_of_a_file_set(sm, files):
    path, recs = files["fasta_empty_record"]
    ss = sm.index.SketchSet.sketch_file(path, ksize=31, scaled=100)
    want_h, want_o, _ = rows_of_records(recs, 31, 100)
    common, _ = ss.compare(jaccard=False)
    want_common, _ = oracle.compare_all_pairs(want_h, want_o)
    assert np.array_equal(common, want_common)
    row = int(np.argmax(np.diff(want_o)))
    hits = ss.search(ss.minhash(row), do_containment=True, threshold=0.5)
    assert hits and hits[0] == (1.0, row)


# ---- 5. limits -------------------------------------------------------------------------------------------------------------------------
def test_k89_goes_record_by_record(sm, files):
    path, recs = files["fasta_empty_record"]
    recs = recs[:40]
    short = path + ".k89.fa"
    with open(short, "wb") as f:
        f.write(fasta_text(recs))
    ss = sm.index.SketchSet.sketch_file(short, ksize=89, scaled=100)
    want_h, want_o, _ = rows_of_records(recs, 89, 100)
    assert len(ss) == 40 and np.array_equal(ss.sizes, np.diff(want_o))
    assert [m["name"] for m in ss.manifest] == [n for n, _ in recs]
    got = sm.sketch.sketch_file(short, "k=89,scaled=100", singleton=True)
    for r in range(40):
        assert np.array_equal(got[r].minhash._mins_array(), want_h[int(want_o[r]):int(want_o[r + 1])])
    import torch
    with pytest.raises(sm.exceptions.SourmashError, match="ksize 1 .. 88"):
        sm.device.DeviceSketcher(ksize=89, scaled=100).sketch_records(torch.zeros(200, dtype=torch.uint8, device="cuda"),
                                                                      to_dev(torch, np.array([0, 200], dtype=np.int64)))


def test_bad_starts_raise_value_error(sm):
    import torch
    seq = to_dev(torch, oracle.synth_dna(0, 10_000, seed=3))
    sk = sm.device.DeviceSketcher(ksize=21, scaled=10)
    for bad in ([0, 5000, 4000, 10_000], [0, 5000, 10_001], [20_000, 30_000]):
        starts = to_dev(torch, np.array(bad, dtype=np.int64))
        with pytest.raises(ValueError, match="record starts"):
            sk.sketch_records(seq, starts)
        with pytest.raises(ValueError, match="record starts"):
            sm.index.SketchSet.sketch_records(seq, starts, ksize=21, scaled=10)
    with pytest.raises(ValueError, match="record starts"):
        sk.sketch_records(seq, torch.zeros(0, dtype=torch.int64, device="cuda"))
    h, o = got_csr(sk.sketch_records(seq, to_dev(torch, np.array([0, 5000, 5000, 10_000], dtype=np.int64))))      # equal starts are fine
    assert o[1] == o[2] and o[3] == len(h)


def raw_bad_starts(bad):
    """smgpu_sketch_records_raw over 200 bases, k = 21, three records whose starts are `bad` -> (returned, code, message).  Only the
    checking kernel reads the starts (d_starts[0 .. 3], nothing they point at); the error is raised on the host from its flag."""
    import torch
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.utils import decode_str
    assert len(bad) == 4
    seq = to_dev(torch, oracle.synth_dna(0, 200, seed=5))
    starts = to_dev(torch, np.array(bad, dtype=np.int64))
    cap = 256
    hashes = torch.zeros(cap, dtype=torch.int64, device="cuda")
    offsets = torch.zeros(4, dtype=torch.int64, device="cuda")
    result = torch.zeros(4, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.smgpu_sketch_records_workspace_bytes(cap, 3)), dtype=torch.uint8, device="cuda")
    lib.sourmash_err_clear()
    n = lib.smgpu_sketch_records_raw(C.c_void_p(seq.data_ptr()), 200, C.c_void_p(starts.data_ptr()), 3, 21, 42, 0,
                                     C.c_void_p(hashes.data_ptr()), None, cap, C.c_void_p(offsets.data_ptr()),
                                     C.c_void_p(result.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    code = lib.sourmash_err_get_last_code()
    msg = decode_str(lib.sourmash_err_get_last_message()) if code else ""
    lib.sourmash_err_clear()
    return n, code, msg


ERROR_CODE_INTERNAL = 2                                   # SOURMASH_ERROR_CODE_INTERNAL (include/sourmash_amd.h)


def test_raw_starts_not_ascending_message(sm):
    n, code, msg = raw_bad_starts([0, 120, 60, 200])
    assert n == 2**64 - 1 and code == ERROR_CODE_INTERNAL
    assert msg == 'internal error: "record starts: the offsets are not ascending"'


def test_raw_last_offset_beyond_len_message(sm):
    n, code, msg = raw_bad_starts([0, 60, 120, 201])
    assert n == 2**64 - 1 and code == ERROR_CODE_INTERNAL
    assert msg == 'internal error: "record starts: the last offset lies behind the end of the buffer (200 bytes)"'


def test_raw_capacity_error_names_the_count(sm):
    import torch
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.utils import decode_str
    buf = oracle.synth_dna(0, 50_000, seed=9)
    seq = to_dev(torch, buf)
    starts = to_dev(torch, np.array([0, 20_000, 50_000], dtype=np.int64))
    max_hash = oracle.max_hash_for_scaled(10)
    dense = dense_hashes(buf, 31)
    kept = int(np.count_nonzero((dense > 0) & (dense <= np.uint64(max_hash))))

    def run(cap):
        hashes = torch.zeros(cap, dtype=torch.int64, device="cuda")
        offsets = torch.zeros(3, dtype=torch.int64, device="cuda")
        result = torch.zeros(4, dtype=torch.int64, device="cuda")
        ws = torch.empty(int(lib.smgpu_sketch_records_workspace_bytes(cap, 2)), dtype=torch.uint8, device="cuda")
        lib.sourmash_err_clear()
        n = lib.smgpu_sketch_records_raw(C.c_void_p(seq.data_ptr()), 50_000, C.c_void_p(starts.data_ptr()), 2, 31, 42, max_hash,
                                         C.c_void_p(hashes.data_ptr()), None, cap, C.c_void_p(offsets.data_ptr()),
                                         C.c_void_p(result.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        code = lib.sourmash_err_get_last_code()
        return n, code, (decode_str(lib.sourmash_err_get_last_message()) if code else ""), int(result[0].item())

    n, code, msg, pairs = run(kept)
    assert code == 0 and pairs == kept and n == len(expected_csr(dense, [0, 20_000, 50_000], 31, max_hash)[0])
    n, code, msg, pairs = run(kept - 1)
    assert n == 2**64 - 1 and code != 0 and pairs == kept
    assert f"output capacity too small: {kept} kept pairs > capacity {kept - 1}" in msg
    # a workspace sized for less is refused before anything runs
    lib.sourmash_err_clear()
    assert lib.smgpu_sketch_records_workspace_bytes(kept, 2) > lib.smgpu_sketch_records_workspace_bytes(kept // 2, 2)


def test_retry_when_the_estimate_is_exceeded(sm):
    """The pair buffer is sized from len / scaled (twice the expectation plus slack, never more than len).  At scaled = 1 that is
    len itself, which no buffer exceeds -- the estimate cannot fail there.  It fails by construction for a buffer of one repeated
    k-mer whose hash is kept at a scaled of 8 or more: every position emits, eight times the expectation."""
    import torch
    found = None
    for k in range(15, 64):
        for unit in (b"A", b"C"):
            hs = set(oracle.seq_to_hashes(unit * 100, k))
            if found is None and len(hs) == 1 and 2**64 // max(hs) >= 8:
                found = (k, unit, hs.pop())
    assert found, "no homopolymer with a small enough hash among the candidates"
    k, unit, h = found
    scaled = min(2**64 // h, 1000)
    assert h <= oracle.max_hash_for_scaled(scaled)
    n = 200_000 - 200_000 % len(unit)
    buf = unit * (n // len(unit))
    half = n // 2
    seq = to_dev(torch, np.frombuffer(buf, dtype=np.uint8))
    starts = to_dev(torch, np.array([0, half, n], dtype=np.int64))
    expect = n / scaled
    assert n - k + 1 > expect * 2 + 16 * (expect + 1) ** 0.5 + 4096               # the estimate is exceeded
    hh, o, a = got_csr(sm.device.DeviceSketcher(ksize=k, scaled=scaled).sketch_records(seq, starts, abund=True))
    assert hh.tolist() == [h, h] and o.tolist() == [0, 1, 2] and a.tolist() == [half - k + 1, n - half - k + 1]
    ss = sm.index.SketchSet.sketch_records(seq, starts, ksize=k, scaled=scaled)
    assert ss.sizes.tolist() == [1, 1] and ss.minhash(1)._mins_array().tolist() == [h]
