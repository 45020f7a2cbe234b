"""GPU parity of k-mer finding (csrc/sketch_find.hip, sourmash_amd/kmers.py): the k-mers of a buffer or a file that hash into a
query sketch, from the kernel-only entry up to `find_kmers`, against rows cut in numpy from the oracle's per-k-mer hashes of the
whole buffer.  Run with -m gpu."""
import csv
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
    import sourmash_amd.kmers  # noqa: F401
    import sourmash_amd.sketch  # noqa: F401
    assert sourmash_amd.gpu_available(), "these tests need a real GPU"
    return sourmash_amd


# ---- expected rows: the oracle's hashes of the whole buffer, numpy.isin, the assign rule ---------------------------------------
def dense_hashes(buf, k):
    "hash of the canonical k-mer at every start position of buf (seed 42), 0 for a k-mer with a byte outside ACGTacgt"
    b = bytes(buf)
    if len(b) < k:
        return np.zeros(0, dtype=np.uint64)
    out = np.zeros(len(b) - k + 1, dtype=np.uint64)
    r = oracle.lib().orc_seq_to_hashes_dna(b, len(b), k, 42, 1, oracle._ptr(out))
    assert r == len(out)
    return out


def matched_pairs(dense, max_hash, query):
    "-> (positions, hashes) of every k-mer of the buffer whose hash is in the query, by position"
    pos = np.flatnonzero((dense > 0) & (dense <= np.uint64(max_hash)) & np.isin(dense, query))
    return pos, dense[pos]


def expected_rows(buf, dense, starts, k, max_hash, query):
    """-> (offsets, positions in the record, hashes, k-mer text as an n x k byte array): the matched k-mers that lie inside a
    record (record of a position: the last one starting at or before it; the k-mer must end inside that record), by position"""
    starts = np.asarray(starts, dtype=np.int64)
    n = len(starts) - 1
    pos, h = matched_pairs(dense, max_hash, np.asarray(query, dtype=np.uint64))
    r = np.searchsorted(starts, pos, side="right") - 1
    ok = (r >= 0) & (r < n)
    ok &= pos + k <= starts[np.clip(r, 0, max(n - 1, 0)) + 1] if n else False
    pos, h, r = pos[ok], h[ok], r[ok]
    offsets = np.searchsorted(r, np.arange(n + 1), side="left").astype(np.uint64)
    upper = np.frombuffer(bytes(buf).upper(), dtype=np.uint8)
    text = upper[pos[:, None] + np.arange(k)[None, :]] if len(pos) else np.zeros((0, k), dtype=np.uint8)
    return offsets, (pos - starts[r]).astype(np.uint64), h, text


def to_dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def make_query(sm, hashes, k, scaled):
    mh = sm.MinHash(0, k, scaled=scaled)
    mh.add_many(np.unique(np.asarray(hashes, dtype=np.uint64)))              # ascending: every add is an append
    return sm.KmerQuery([mh])


def assert_rows(m, want):
    offsets, positions, hashes, text = want
    assert np.array_equal(m.offsets, offsets)
    assert np.array_equal(m.positions, positions)
    assert np.array_equal(m.hashes, hashes)
    assert np.array_equal(m._kmer_bytes, text)
    assert m.kmers() == [bytes(t).decode() for t in text]
    assert np.array_equal(m.records, np.repeat(np.arange(len(offsets) - 1), np.diff(offsets).astype(np.int64)))
    assert np.array_equal(m.found_hashes, np.unique(hashes))


# ---- 1. boundaries ---------------------------------------------------------------------------------------------------------------
def boundary_buffer(k):
    """~200 kB with hand-placed records: bytes in front of the first start; records that end / start at bytes 4095, 4096 and 4097
    (the kernel's tile is 256 x 16 start positions); two consecutive empty records; records of 1, k - 1, k, k + 1, 4095, 4096,
    4097 and 10,000 bases; records that touch with no separator byte and records that end in one; N, IUPAC and lower-case bytes; a
    poly-A and a poly-T run of 3 k bases (one canonical hash at 2 k + 1 positions of each, on either strand); the last record
    ends exactly at len."""
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
        if n == 10_000:
            rec[3000:3000 + 3 * k] = ord("A")
            rec[6000:6000 + 3 * k] = ord("T")
            rec[8000:8000 + 2 * k] = ord("a")
        parts.append(rec)
        starts.append(starts[-1] + n)
    buf = np.concatenate(parts)
    assert starts[1] == 4095 and starts[2] == 4096 and starts[3] == 4097 and starts[-1] == len(buf)
    return buf, starts


_RANDOM = {}


def random_hashes(max_hash):
    "10^6 random hashes within the sketch's range, made once per range"
    if max_hash not in _RANDOM:
        _RANDOM[max_hash] = np.random.default_rng(11).integers(1, max_hash, size=10**6, dtype=np.uint64, endpoint=True)
    return _RANDOM[max_hash]


@pytest.mark.parametrize("scaled", [1, 10, 1000])
@pytest.mark.parametrize("k", [11, 21, 31, 51, 88])
def test_boundaries(sm, k, scaled):
    import torch
    buf, starts = boundary_buffer(k)
    max_hash = oracle.max_hash_for_scaled(scaled)
    dense = dense_hashes(buf, k)
    sketch = np.unique(dense[(dense > 0) & (dense <= np.uint64(max_hash))])
    assert len(sketch) >= 100
    rng = np.random.default_rng(k * 1000 + scaled)
    seq_t, starts_t = to_dev(torch, buf), to_dev(torch, np.asarray(starts, dtype=np.int64))
    poly_a = int(dense[starts[12] + 3000])                                       # the poly-A run's hash; the poly-T run has the same
    assert poly_a == int(dense[starts[12] + 6000]) == int(dense[starts[12] + 3000 + 2 * k])
    present = poly_a if poly_a <= max_hash else int(sketch[len(sketch) // 2])
    absent = np.setdiff1d(rng.integers(1, max_hash, size=1000, dtype=np.uint64, endpoint=True), sketch)
    run_start = min(max(1, present - 2500), max_hash - 4999)
    queries = {
        "whole": sketch,                                                         # scaled = 1: the sink's over-capacity path
        "half": rng.permutation(sketch)[:len(sketch) // 2],
        "one": np.array([present], dtype=np.uint64),
        "absent": absent,
        "run": np.arange(run_start, run_start + 5000, dtype=np.uint64),          # one bucket of the directory
        "ends": np.array([sketch[0], sketch[-1], 1, max_hash], dtype=np.uint64),
        "large": np.concatenate([random_hashes(max_hash), sketch]),
    }
    for name, q in queries.items():
        query = make_query(sm, q, k, scaled)
        assert len(query) == len(np.unique(q))
        m = query.find(seq_t, starts_t)
        want = expected_rows(buf, dense, starts, k, max_hash, q)
        assert_rows(m, want)
        if name == "whole":                                                      # every kept position inside a record matches
            all_kept = expected_rows(buf, dense, starts, k, max_hash, sketch)[0][-1]
            assert len(m) == all_kept and len(m) > len(sketch) // 2
        if name == "absent":
            assert len(m) == 0 and not m.offsets.any() and m.matched_records == []
        if name == "one" and present == poly_a:
            assert len(m) >= 2 * (2 * k + 1)                                     # every position of both runs, either strand
        if name in ("one", "run", "ends", "large"):
            assert len(m) >= 1
        assert m.offsets[3] == m.offsets[4] == m.offsets[5]                      # empty records: no rows
    # a matched record's sequence comes back as the buffer holds it
    m = make_query(sm, queries["half"], k, scaled).find(seq_t, starts_t)
    r = m.matched_records[0][0]
    assert m.sequence(r) == bytes(buf[starts[r]:starts[r + 1]]).decode()


# ---- 2. staging edges ------------------------------------------------------------------------------------------------------------
def kernel_pairs(sm, query, seq_t, grid, cap):
    "the multiset of (hash, position) the find kernel alone appends, sorted"
    import torch
    hashes = torch.zeros(cap, dtype=torch.int64, device="cuda")
    positions = torch.zeros(cap, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    query.kernel_only(seq_t, hashes, positions, count, grid=grid)
    n = int(count.item())
    assert n <= cap
    h, p = hashes[:n].cpu().numpy().view(np.uint64), positions[:n].cpu().numpy().view(np.uint64)
    order = np.lexsort((h, p))
    return p[order], h[order]


@pytest.mark.parametrize("staged", [511, 512, 513, 1023, 1024, 1025])
def test_staging_edges_one_workgroup(sm, staged):
    """One workgroup, scaled = 1, k = 21: the first tile (4,096 start positions) stages exactly `staged` pairs -- a run of valid
    DNA, then N up to the tile's end -- around the flush threshold (512) and the capacity (1,024) of the LDS staging, and a second
    tile lies behind it."""
    import torch
    k = 21
    rng = np.random.default_rng(staged)
    buf = np.full(4096 + 10 + 300, ord("N"), dtype=np.uint8)
    buf[:staged + k - 1] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=staged + k - 1)]
    buf[4096 + 10:] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=300)]
    dense = dense_hashes(buf, k)
    assert np.count_nonzero(dense[:4096]) == staged and np.count_nonzero(dense[4096:]) == 300 - k + 1
    max_hash = oracle.max_hash_for_scaled(1)
    sketch = np.unique(dense[dense > 0])
    seq_t = to_dev(torch, buf)
    for q in (sketch, np.random.default_rng(1).permutation(sketch)[:len(sketch) // 2], sketch[:1]):
        want_p, want_h = matched_pairs(dense, max_hash, q)
        got_p, got_h = kernel_pairs(sm, make_query(sm, q, k, 1), seq_t, 1, len(buf))
        assert np.array_equal(got_p, want_p.astype(np.uint64)) and np.array_equal(got_h, want_h)


def test_staging_many_tiles_per_workgroup(sm):
    "two workgroups over the 200 kB buffer at scaled = 1: some 25 tiles each, flushes between tiles, staging over capacity in each"
    import torch
    k = 21
    buf, _ = boundary_buffer(k)
    dense = dense_hashes(buf, k)
    max_hash = oracle.max_hash_for_scaled(1)
    sketch = np.unique(dense[dense > 0])
    seq_t = to_dev(torch, buf)
    for q in (sketch, np.random.default_rng(2).permutation(sketch)[:len(sketch) // 2]):
        want_p, want_h = matched_pairs(dense, max_hash, q)
        query = make_query(sm, q, k, 1)
        for grid in (2, 0):
            got_p, got_h = kernel_pairs(sm, query, seq_t, grid, len(buf))
            assert np.array_equal(got_p, want_p.astype(np.uint64)) and np.array_equal(got_h, want_h)


# ---- 3. alignment ----------------------------------------------------------------------------------------------------------------
def test_unaligned_pointer(sm):
    "the device pointer 3 bytes behind a 16-byte boundary (a tensor slice)"
    import torch
    k, scaled = 31, 10
    buf, starts = boundary_buffer(k)
    base = torch.zeros(len(buf) + 64, dtype=torch.uint8, device="cuda")
    view = base[3:3 + len(buf)]
    view.copy_(torch.from_numpy(buf))
    assert view.data_ptr() % 16 == 3
    max_hash = oracle.max_hash_for_scaled(scaled)
    dense = dense_hashes(buf, k)
    sketch = np.unique(dense[(dense > 0) & (dense <= np.uint64(max_hash))])
    q = sketch[::2]
    m = make_query(sm, q, k, scaled).find(view, to_dev(torch, np.asarray(starts, dtype=np.int64)))
    assert_rows(m, expected_rows(buf, dense, starts, k, max_hash, q))
    assert len(m) > len(q) // 2                      # (a few of the query's k-mers span two records and are dropped)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def raw_find(sm, query, seq, starts, cap, n=None):
    "smgpu_find_kmers_raw with fresh arrays of `cap` rows, pre-set to a marker -> (returned, code, message, result, positions)"
    import torch
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.utils import decode_str
    n_records = starts.numel() - 1
    k = query.ksize
    positions = torch.full((max(cap, 1),), -7, dtype=torch.int64, device="cuda")
    hashes = torch.full((max(cap, 1),), -7, dtype=torch.int64, device="cuda")
    kmers = torch.zeros(max(cap, 1) * k, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n_records + 1,), -7, dtype=torch.int64, device="cuda")
    result = torch.zeros(4, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.smgpu_find_kmers_workspace_bytes(cap, n_records)), dtype=torch.uint8, device="cuda")
    lib.sourmash_err_clear()
    got = lib.smgpu_find_kmers_raw(query._ptr, C.c_void_p(seq.data_ptr()), seq.numel() if n is None else n, C.c_void_p(starts.data_ptr()),
                                   n_records, C.c_void_p(positions.data_ptr()), C.c_void_p(hashes.data_ptr()), C.c_void_p(kmers.data_ptr()),
                                   cap, C.c_void_p(offsets.data_ptr()), C.c_void_p(result.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    code = lib.sourmash_err_get_last_code()
    msg = decode_str(lib.sourmash_err_get_last_message()) if code else ""
    lib.sourmash_err_clear()
    return got, code, msg, result.cpu().numpy().view(np.uint64), positions.cpu().numpy()


def test_bad_starts_raise_and_launch_nothing(sm):
    import torch
    buf = oracle.synth_dna(0, 10_000, seed=3)
    seq = to_dev(torch, buf)
    dense = dense_hashes(buf, 21)
    query = make_query(sm, np.unique(dense[dense > 0])[:500], 21, 1)
    for bad in ([0, 5000, 4000, 10_000], [0, 5000, 10_001], [20_000, 30_000]):
        starts = to_dev(torch, np.array(bad, dtype=np.int64))
        with pytest.raises(ValueError, match="record starts"):
            query.find(seq, starts)
        got, code, msg, result, positions = raw_find(sm, query, seq, starts, 10_000)
        assert got == 2**64 - 1 and code != 0 and "record starts" in msg
        assert result[0] == 0 and result[3] != 0 and (positions == -7).all()      # no pair was matched, nothing was written
    with pytest.raises(ValueError, match="record starts"):
        query.find(seq, torch.zeros(0, dtype=torch.int64, device="cuda"))
    m = query.find(seq, to_dev(torch, np.array([0, 5000, 5000, 10_000], dtype=np.int64)))      # equal starts are fine
    assert m.offsets[1] == m.offsets[2] and m.offsets[3] == len(m) > 0


ERROR_CODE_INTERNAL = 2                                   # SOURMASH_ERROR_CODE_INTERNAL (include/sourmash_amd.h)


def raw_find_bad_starts(sm, bad):
    """smgpu_find_kmers_raw over 200 bases, k = 21, three records whose starts are `bad` -> (returned, code, message).  Only the
    checking kernel reads the starts (d_starts[0 .. 3], nothing they point at); the error is raised on the host from its flag."""
    import torch
    assert len(bad) == 4
    buf = oracle.synth_dna(0, 200, seed=5)
    dense = dense_hashes(buf, 21)
    query = make_query(sm, dense[dense > 0][:50], 21, 1)
    got, code, msg, result, positions = raw_find(sm, query, to_dev(torch, buf), to_dev(torch, np.array(bad, dtype=np.int64)), 256)
    assert result[0] == 0 and (positions == -7).all()                          # raised in front of the pairs kernel
    return got, code, msg


def test_raw_starts_not_ascending_message(sm):
    got, code, msg = raw_find_bad_starts(sm, [0, 120, 60, 200])
    assert got == 2**64 - 1 and code == ERROR_CODE_INTERNAL
    assert msg == 'internal error: "record starts: the offsets are not ascending"'


def test_raw_last_offset_beyond_len_message(sm):
    got, code, msg = raw_find_bad_starts(sm, [0, 60, 120, 201])
    assert got == 2**64 - 1 and code == ERROR_CODE_INTERNAL
    assert msg == 'internal error: "record starts: the last offset lies behind the end of the buffer (200 bytes)"'


def test_raw_capacity_error_names_the_count(sm):
    import torch
    k, scaled = 31, 10
    buf = oracle.synth_dna(0, 50_000, seed=9)
    seq = to_dev(torch, buf)
    bounds = [0, 20_000, 50_000]
    starts = to_dev(torch, np.array(bounds, dtype=np.int64))
    max_hash = oracle.max_hash_for_scaled(scaled)
    dense = dense_hashes(buf, k)
    across = dense[20_000 - k + 1:20_000]                     # the k-mers that span the two records
    across = across[(across > 0) & (across <= np.uint64(max_hash))]
    q = np.union1d(np.unique(dense[(dense > 0) & (dense <= np.uint64(max_hash))])[::2], across)
    query = make_query(sm, q, k, scaled)
    matched = len(matched_pairs(dense, max_hash, q)[0])
    want = expected_rows(buf, dense, bounds, k, max_hash, q)
    assert len(across) >= 1 and matched >= len(want[2]) + len(across) > 100      # matched in the kernel, dropped by the assign rule
    got, code, msg, result, _ = raw_find(sm, query, seq, starts, matched - 1)
    assert got == 2**64 - 1 and code != 0 and result[0] == matched
    assert f"output capacity too small: {matched} matched pairs > capacity {matched - 1}" in msg
    got, code, msg, result, positions = raw_find(sm, query, seq, starts, matched)               # the retry with the count
    assert code == 0 and got == len(want[2]) and result[0] == matched and result[1] == got
    rel = positions[:got].astype(np.uint64) - np.repeat(np.array(bounds[:-1], dtype=np.uint64), np.diff(want[0]).astype(np.int64))
    assert np.array_equal(rel, want[1])
    # the Python layer retries by itself
    m = query.find(seq, starts)
    assert_rows(m, want)


def test_k89_is_refused_by_the_raw_entry(sm):
    import torch
    mh = sm.MinHash(0, 89, scaled=10)
    mh.add_many([5, 7])
    query = sm.KmerQuery([mh])
    seq = torch.zeros(500, dtype=torch.uint8, device="cuda")
    starts = to_dev(torch, np.array([0, 500], dtype=np.int64))
    got, code, msg, result, positions = raw_find(sm, query, seq, starts, 100)
    assert got == 2**64 - 1 and code != 0 and "ksize 1 .. 88" in msg and (positions == -7).all()
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(sm.exceptions.SourmashError, match="ksize 1 .. 88"):
        query.kernel_only(seq, torch.zeros(8, dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda"), count)
    assert int(count.item()) == 0


def test_retry_when_the_estimate_is_exceeded(sm):
    "a buffer of one repeated k-mer whose hash the query holds: every position matches, far above the expectation len / scaled"
    import torch
    k, scaled = 21, 1000
    found = None
    for kk in range(15, 64):
        for unit in (b"A", b"C"):
            hs = set(oracle.seq_to_hashes(unit * 100, kk))
            if found is None and len(hs) == 1 and max(hs) <= oracle.max_hash_for_scaled(8):
                found = (kk, unit, hs.pop())
    assert found, "no homopolymer with a small enough hash among the candidates"
    k, unit, h = found
    scaled = min(2**64 // h, 1000)
    n = 200_000
    seq = to_dev(torch, np.frombuffer(unit * n, dtype=np.uint8))
    starts = to_dev(torch, np.array([0, n // 2, n], dtype=np.int64))
    expect = n / scaled
    assert n - 2 * (k - 1) > expect * 2 + 16 * (expect + 1) ** 0.5 + 4096         # the estimate is exceeded
    m = make_query(sm, [h], k, scaled).find(seq, starts)
    assert len(m) == n - 2 * (k - 1) and m.offsets.tolist() == [0, n // 2 - k + 1, n - 2 * (k - 1)]
    assert (m.hashes == h).all() and np.array_equal(m.positions[:n // 2 - k + 1], np.arange(n // 2 - k + 1, dtype=np.uint64))


# ---- 5. files --------------------------------------------------------------------------------------------------------------------
def file_records():
    rng = np.random.default_rng(21)
    recs = []
    for i, length in enumerate([3000, 120, 0, 7001, 30, 2500, 900]):
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=length)].copy()
        if length > 500:
            seq[100] = ord("N")
            seq[200:260] = np.frombuffer(bytes(seq[200:260]).lower(), dtype=np.uint8)
        recs.append((f"rec{i} len={length} some description", bytes(seq)))
    return recs


def fasta_text(recs, width=70):
    out = []
    for name, seq in recs:
        out.append(b">" + name.encode() + b"\n")
        for i in range(0, len(seq), width):
            out.append(seq[i:i + width] + b"\n")
    return b"".join(out)


def fastq_text(recs):
    return b"".join(b"@" + n.encode() + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in recs)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("find")
    recs = file_records()
    out = {}
    for name, data in (("recs.fa", fasta_text(recs)), ("recs.fq", fastq_text(recs)), ("recs.fa.gz", gzip.compress(fasta_text(recs), 6)),
                       ("recs.fq.gz", gzip.compress(fastq_text(recs), 6))):
        (d / name).write_bytes(data)
        out[name] = str(d / name)
    return out, recs


def rows_of_records(recs, k, max_hash, query):
    "expected rows of (name, sequence) records: the records joined, the oracle's hashes of the whole, cut by the starts"
    buf = b"".join(s for _, s in recs)
    starts = np.concatenate([[0], np.cumsum([len(s) for _, s in recs])]).astype(np.int64)
    return expected_rows(buf, dense_hashes(buf, k), starts, k, max_hash, query)


def assert_file_matches(m, recs, want):
    assert_rows(m, want)
    assert m.names == [n for n, _ in recs]
    assert m.n_records == len(recs) and m.n_bases == sum(len(s) for _, s in recs)
    assert m.record_lengths.tolist() == [len(s) for _, s in recs]
    matched = [r for r in range(len(recs)) if want[0][r + 1] > want[0][r]]
    assert m.matched_records == [(r, recs[r][0]) for r in matched] and len(matched) >= 3
    for r in matched:
        assert m.sequence(r) == recs[r][1].decode()
    assert list(m.rows()) == [(recs[r][0], bytes(t).decode(), int(h)) for r, t, h in zip(m.records.tolist(), want[3], want[2])]


@pytest.mark.parametrize("name", ["recs.fa", "recs.fq", "recs.fa.gz", "recs.fq.gz"])
def test_find_file(sm, files, name, monkeypatch):
    paths, recs = files
    k, scaled = 31, 10
    assert list(sm.sketch.read_records(paths[name])) == recs
    max_hash = oracle.max_hash_for_scaled(scaled)
    buf = b"".join(s for _, s in recs)
    dense = dense_hashes(buf, k)
    q = np.unique(dense[(dense > 0) & (dense <= np.uint64(max_hash))])[::3]
    query = make_query(sm, q, k, scaled)
    want = rows_of_records(recs, k, max_hash, q)
    assert len(want[2]) >= 100
    assert sm.sketch._records_path_takes(paths[name], [k])
    m = query.find_file(paths[name])
    assert m._owner is not None                                                   # the one-pass file path
    assert_file_matches(m, recs, want)
    # a file the one-pass path refuses goes through find in pieces, with identical results
    monkeypatch.setattr(sm.sketch, "_records_path_takes", lambda path, ks: False)
    m2 = query.find_file(paths[name])
    assert m2._owner is None
    assert_file_matches(m2, recs, want)
    assert m2 == m
    monkeypatch.setattr(sm.kmers, "CHUNK_BYTES", 4000)                            # several pieces
    m3 = query.find_file(paths[name])
    assert_file_matches(m3, recs, want)
    assert m3 == m


def test_k101_goes_record_by_record(sm, files):
    paths, recs = files
    k, scaled = 101, 10
    max_hash = oracle.max_hash_for_scaled(scaled)
    buf = b"".join(s for _, s in recs)
    dense = dense_hashes(buf, k)
    q = np.unique(dense[(dense > 0) & (dense <= np.uint64(max_hash))])[::2]
    query = make_query(sm, q, k, scaled)
    want = rows_of_records(recs, k, max_hash, q)
    assert len(want[2]) >= 50
    assert not sm.sketch._records_path_takes(paths["recs.fa"], [k])
    assert_file_matches(query.find_file(paths["recs.fa"]), recs, want)
    import torch
    starts = np.concatenate([[0], np.cumsum([len(s) for _, s in recs])]).astype(np.int64)
    m = query.find(to_dev(torch, np.frombuffer(buf, dtype=np.uint8)), to_dev(torch, starts), names=[n for n, _ in recs])
    assert_file_matches(m, recs, want)


# ---- 6. the reference's own numbers ----------------------------------------------------------------------------------------------
SHORT_FA = golden("kmers", "short.fa")


@pytest.fixture(scope="module")
def short(sm):
    (name, seq), = list(sm.sketch.read_records(SHORT_FA))
    assert name == "shortName" and len(seq) == 1000
    return name, seq, dense_hashes(seq, 31)


def test_reference_numbers_scaled_1(sm, short):
    "tests/test_cmd_signature.py:4332-4390 of the reference: 970 query hashes, 970 k-mers, 970 distinct found (100.0 %)"
    name, seq, dense = short
    sig, = sm.sketch.sketch_file(SHORT_FA, "k=31,scaled=1")
    query = sm.KmerQuery([sig])
    assert len(query) == 970 == len(np.unique(dense))
    m = query.find_file(SHORT_FA)
    assert len(m) == 970 and len(m.found_hashes) == 970 and len(m.found_hashes) / len(query) == 1.0
    assert m.matched_records == [(0, "shortName")] and len(m.sequence(0)) == 1000 and m.sequence(0) == seq.decode()
    assert np.array_equal(m.positions, np.arange(970, dtype=np.uint64)) and np.array_equal(m.hashes, dense)
    assert m.kmers() == [seq[i:i + 31].decode().upper() for i in range(970)]
    # re-sketching the reported k-mer strings gives the query back
    again = sm.MinHash(0, 31, scaled=1)
    for kmer in m.kmers():
        again.add_sequence(kmer)
    assert np.array_equal(again._mins_array(), query.minhash._mins_array())


def test_reference_numbers_scaled_100_and_one_hash(sm, short):
    name, seq, dense = short
    sig, = sm.sketch.sketch_file(SHORT_FA, "k=31,scaled=100")
    m = sm.KmerQuery([sig]).find_file(SHORT_FA)
    assert m.positions.tolist() == [137, 199, 356, 796, 926] and np.array_equal(m.hashes, dense[[137, 199, 356, 796, 926]])
    # the fabricated one-hash query of test_cmd_signature.py:4480-4540
    mh = sm.MinHash(0, 31, scaled=1)
    mh.add_hash(1070961951490202715)
    m = sm.KmerQuery([mh]).find_file(SHORT_FA)
    assert m.positions.tolist() == [645] and m.hashes.tolist() == [1070961951490202715]
    assert m.kmers() == [seq[645:645 + 31].decode().upper()]


def test_find_kmers_command(sm, short, tmp_path):
    name, seq, dense = short
    sig, = sm.sketch.sketch_file(SHORT_FA, "k=31,scaled=1")
    kmers_csv, seqs_fa = tmp_path / "kmers.csv", tmp_path / "matched.fa"
    out = sm.find_kmers([sig], [SHORT_FA], save_kmers=str(kmers_csv), save_sequences=str(seqs_fa))
    assert out == dict(n_files_searched=1, n_sequences_searched=1, n_bp_searched=1000, n_kmers_found=970, n_sequences_found=1,
                       n_bp_saved=1000, n_query_hashes=970, n_found_hashes=970)
    with open(kmers_csv, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["sequence_file", "sequence_name", "kmer", "hashval"] and len(rows) == 971
    assert rows[1:] == [[SHORT_FA, "shortName", seq[i:i + 31].decode().upper(), str(int(dense[i]))] for i in range(970)]
    assert seqs_fa.read_text() == f">shortName\n{seq.decode()}\n"
    # two files, no outputs: the totals add up, the distinct hashes do not
    out = sm.find_kmers(sig, [SHORT_FA, SHORT_FA])
    assert (out["n_files_searched"], out["n_sequences_searched"], out["n_kmers_found"], out["n_found_hashes"]) == (2, 2, 1940, 970)
    empty = tmp_path / "empty.fa"
    empty.write_text("")
    with pytest.raises(ValueError, match="no sequences searched"):
        sm.find_kmers([sig], [str(empty)])
    with pytest.raises(ValueError, match="no hashes in query signature"):
        sm.find_kmers([sm.MinHash(0, 31, scaled=1)], [SHORT_FA])
