"""GPU parity of per-record protein / dayhoff / hp sketching (csrc/protein_records.hip): every record of a buffer or of a file as
a sketch of its own, for protein input and for DNA translated in six frames, from the raw entry point up to
`sketch_file(singleton=True)`.  Expected rows are built record by record from the oracle.  Run with -m gpu."""
import functools
import gzip

import numpy as np
import pytest

import oracle
from conftest import golden

pytestmark = pytest.mark.gpu

MOLTYPES = ["protein", "dayhoff", "hp"]
AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    import sourmash_amd.device  # noqa: F401
    import sourmash_amd.index  # noqa: F401
    import sourmash_amd.sketch  # noqa: F401
    assert sourmash_amd.gpu_available(), "these tests need a real GPU"
    return sourmash_amd


# ---- expected rows: the oracle's hashes of every record by itself ------------------------------------------------------------------
@functools.lru_cache(maxsize=4096)
def record_hashes(rec, k, moltype, is_protein):
    "the oracle's hashes of one record by itself (computed once per record and parameters, shared by the scaled values; read-only)"
    if not len(rec):
        return np.zeros(0, dtype=np.uint64)
    h = oracle.seq_to_hashes_protein(rec, k, moltype, 42, is_protein)
    h.setflags(write=False)
    return h


def expected_csr(records, k, moltype, scaled, is_protein):
    "records: list of bytes -> (hashes, offsets, abundances): per record the sorted distinct hashes 0 < h <= max_hash and their counts"
    max_hash = np.uint64(oracle.max_hash_for_scaled(scaled))
    hs, cs, offsets = [], [], [0]
    for rec in records:
        h = record_hashes(rec, k, moltype, is_protein)
        h = np.sort(h[(h > 0) & (h <= max_hash)])
        u, c = np.unique(h, return_counts=True)
        hs.append(u); cs.append(c.astype(np.uint64))
        offsets.append(offsets[-1] + len(u))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)   # noqa: E731
    return cat(hs).astype(np.uint64), np.asarray(offsets, dtype=np.uint64), cat(cs).astype(np.uint64)


def to_dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def got_csr(res):
    return tuple(t.cpu().numpy().view(np.uint64) for t in res)


def records_of(buf, starts, ends):
    ends = starts[1:] if ends is None else ends
    return [bytes(buf[int(s):int(e)]) for s, e in zip(starts[:-1], ends)]


def check(sm, buf, starts, ends, k, moltype, scaled, is_protein, seq_t=None, want=None):
    "flat and with abundances through DeviceSketcher.sketch_records, against the expected rows"
    import torch
    want_h, want_o, want_a = want or expected_csr(records_of(buf, starts, ends), k, moltype, scaled, is_protein)
    if seq_t is None:
        seq_t = to_dev(torch, np.frombuffer(bytes(buf), dtype=np.uint8))
    starts_t = to_dev(torch, np.asarray(starts, dtype=np.int64))
    ends_t = None if ends is None else to_dev(torch, np.asarray(ends, dtype=np.int64))
    sk = sm.device.DeviceSketcher(ksize=k, scaled=scaled)
    h, o = got_csr(sk.sketch_records(seq_t, starts_t, moltype=moltype, is_protein=is_protein, ends=ends_t))
    assert np.array_equal(o, want_o)
    assert np.array_equal(h, want_h)
    h, o, a = got_csr(sk.sketch_records(seq_t, starts_t, abund=True, moltype=moltype, is_protein=is_protein, ends=ends_t))
    assert np.array_equal(o, want_o) and np.array_equal(h, want_h) and np.array_equal(a, want_a)
    return want_h, want_o, want_a


# ---- 1. boundaries, protein input ----------------------------------------------------------------------------------------------------
def protein_record(rng, n):
    return AMINO[rng.integers(0, len(AMINO), size=n)].copy()


@functools.lru_cache(maxsize=None)
def protein_boundaries(k, gaps):
    """~100 kB with hand-placed records: 7 bytes in front of the first start; records that begin or end at bytes 7, 8, 9 and 2047,
    2048, 2049 (a lane owns 8 window starts, a workgroup round 2,048); two consecutive empty records; records of 1, k - 1, k, k + 1
    and 5,000 residues; lower case, '*', 'X', 'B' / 'Z' / 'J' and bytes >= 0x80 with 0xFF among them.  gaps: every record but the
    last is followed by a '>' byte that belongs to no record (ends given); else the records touch (ends None)."""
    rng = np.random.default_rng(300 + k)
    lens = [1, 1, 2038, 1, 1, 0, 0, 1, k - 1, k, k + 1, 5_000, 3 * k, 30_000, 0, 60_000]
    parts, starts, ends = [protein_record(rng, 7)], [7], []
    at = 7
    for i, n in enumerate(lens):
        rec = protein_record(rng, n)
        if n == 5_000:
            rec[100:400] = np.frombuffer(bytes(rec[100:400]).lower(), dtype=np.uint8)
            rec[1000] = ord("*"); rec[1003] = ord("X"); rec[1500:1503] = np.frombuffer(b"BZJ", dtype=np.uint8)
            rec[2000] = 0x80; rec[2100] = 0xff; rec[2101] = 0xff; rec[2200] = 0xfe; rec[4999] = 0xff
            rec[3000:3000 + k + 5] = ord("A")                      # a repeated window: abundances above 1 at any scaled
        if n == 60_000:
            rec[-1] = 0xff                                          # the last byte of the buffer
        parts.append(rec)
        at += n
        ends.append(at)
        if gaps and i + 1 < len(lens):
            parts.append(np.frombuffer(b">", dtype=np.uint8))
            at += 1
        starts.append(at)
    buf = np.concatenate(parts)
    assert starts[-1] == len(buf)
    if not gaps:
        assert starts[:6] == [7, 8, 9, 2047, 2048, 2049]
    return buf, np.asarray(starts, dtype=np.int64), (np.asarray(ends, dtype=np.int64) if gaps else None)


@pytest.mark.parametrize("scaled", [1, 20, 200])
@pytest.mark.parametrize("moltype", MOLTYPES)
@pytest.mark.parametrize("k", [7, 8, 9, 15, 16, 17, 25, 32, 42, 79])
def test_protein_boundaries(sm, k, moltype, scaled):
    for gaps in (False, True):
        buf, starts, ends = protein_boundaries(k, gaps)
        want_h, want_o, want_a = check(sm, buf, starts, ends, k, moltype, scaled, True)
        assert want_o[5] == want_o[6] == want_o[7]                         # empty records: empty rows
        assert want_o[8] == want_o[9] and want_o[10] - want_o[9] <= 1      # 1 and k - 1 residues: nothing; k residues: one window
        assert scaled != 1 or want_a.max() >= 6                           # the repeated window is counted


def test_gap_byte_belongs_to_no_record(sm):
    """With `ends` given the window that ends on the '>' between two records is absent; with the same starts and no ends it is
    there (the byte is a residue 'X' of the record in front of it)."""
    import torch
    k = 7
    a, b = b"MKVLAAGIVGLLLAQWERT", b"PPGHHDESTTRRKLMNAC"
    buf = np.frombuffer(a + b">" + b, dtype=np.uint8)
    starts = np.asarray([0, len(a) + 1, len(buf)], dtype=np.int64)
    ends = np.asarray([len(a), len(buf)], dtype=np.int64)
    want = expected_csr([a, b], k, "protein", 1, True)
    check(sm, buf, starts, ends, k, "protein", 1, True, want=want)
    sk = sm.device.DeviceSketcher(ksize=k, scaled=1)
    h, o = got_csr(sk.sketch_records(to_dev(torch, buf), to_dev(torch, starts), moltype="protein", is_protein=True))
    with_gap = expected_csr([a + b">", b], k, "protein", 1, True)
    assert np.array_equal(h, with_gap[0]) and np.array_equal(o, with_gap[1])
    assert with_gap[1][1] == want[1][1] + 1


# ---- 2. boundaries, translated DNA ---------------------------------------------------------------------------------------------------
def dna_record(rng, n):
    return BASES[rng.integers(0, 4, size=n)].copy()


@functools.lru_cache(maxsize=None)
def translate_boundaries(k, gaps):
    """Records of 3k - 1 .. 3k + 3 bases (frames 1 and 2 fall one residue short), of lengths = 0, 1, 2 mod 3 around 4,096, empty
    and 1-base records, N in each codon position, IUPAC, non-base bytes and lower case; bytes in front of the first start."""
    rng = np.random.default_rng(500 + k)
    lens = [3 * k - 1, 3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 3, 0, 1, 0, 4095, 4096, 4097, 2, 3, 5_000, 10_000]
    parts, starts, ends = [dna_record(rng, 5)], [5], []
    at = 5
    for i, n in enumerate(lens):
        rec = dna_record(rng, n)
        if n == 5_000:
            rec[300] = ord("N"); rec[604] = ord("N"); rec[908] = ord("n")   # positions = 0, 1, 2 mod 3
            rec[1200:1204] = np.frombuffer(b"RYKM", dtype=np.uint8)
            rec[1500] = ord("-"); rec[1600] = 0xff; rec[1700] = ord(">"); rec[1800] = 0
            rec[2000:2600] = np.frombuffer(bytes(rec[2000:2600]).lower(), dtype=np.uint8)
            rec[3000:3000 + 3 * k + 30] = ord("A")                   # a repeated window
        parts.append(rec)
        at += n
        ends.append(at)
        if gaps and i + 1 < len(lens):
            parts.append(np.frombuffer(b">", dtype=np.uint8))
            at += 1
        starts.append(at)
    buf = np.concatenate(parts)
    return buf, np.asarray(starts, dtype=np.int64), (np.asarray(ends, dtype=np.int64) if gaps else None)


@pytest.mark.parametrize("scaled", [1, 20])
@pytest.mark.parametrize("moltype", MOLTYPES)
@pytest.mark.parametrize("k", [7, 10, 16, 42])
def test_translate_boundaries(sm, k, moltype, scaled):
    for gaps in (False, True):
        buf, starts, ends = translate_boundaries(k, gaps)
        want_h, want_o, _ = check(sm, buf, starts, ends, k, moltype, scaled, False)
        assert want_o[0] == want_o[1]                                      # 3k - 1 bases: nothing
        assert want_o[5] == want_o[6] == want_o[7] == want_o[8]            # empty and 1-base records
        assert scaled != 1 or (want_o[2] > want_o[1] and want_o[5] > want_o[4])


# ---- 3. many short records -----------------------------------------------------------------------------------------------------------
def test_many_short_protein_records(sm):
    rng = np.random.default_rng(7)
    lens = rng.integers(50, 401, size=20_000)
    buf = protein_record(rng, int(lens.sum()))
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    want_h, want_o, _ = check(sm, buf, starts, None, 10, "protein", 20, True)
    assert len(want_o) == 20_001 and (np.diff(want_o) > 0).sum() > 19_000


def test_many_short_translated_reads(sm):
    rng = np.random.default_rng(8)
    n = 20_000
    buf = dna_record(rng, 150 * n)
    starts = (np.arange(n + 1) * 150).astype(np.int64)
    want_h, want_o, _ = check(sm, buf, starts, None, 10, "dayhoff", 20, False)
    assert len(want_o) == n + 1 and (np.diff(want_o) > 0).sum() > 0.9 * n


# ---- 4. unaligned input pointer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 3])
def test_unaligned_pointer(sm, shift):
    import torch
    for is_protein, (buf, starts, ends) in ((True, protein_boundaries(16, True)), (False, translate_boundaries(10, True))):
        base = torch.zeros(len(buf) + 64, dtype=torch.uint8, device="cuda")
        view = base[shift:shift + len(buf)]
        view.copy_(torch.from_numpy(buf))
        assert view.data_ptr() % 16 == shift
        check(sm, buf, starts, ends, 16 if is_protein else 10, "protein", 20, is_protein, seq_t=view)


# ---- 4b. the pair kernel alone: a workgroup appends in the round behind a flush ---------------------------------------------------------
# The staged pairs leave LDS through LdsSink, whose flush zeroes the counter behind its own last barrier: the round loop
# (csrc/residue_kernel.hpp) has to put one barrier between that and the next round's appends.  2,048 workgroups of 2,048 window
# starts make a round; workgroup 0 owns starts [0, 2048) in the first and [ROUND, ROUND + 2048) in the second.
WG_STARTS = 2048
ROUND = 2048 * WG_STARTS
FLUSH_AT = 512                      # half of the 1,024 staged pairs


@functools.lru_cache(maxsize=2)
def two_round_hashes(k):
    "n = one round + one workgroup + k residues, and the oracle's hash of every window by start (read-only)"
    data = AMINO[np.random.default_rng(40 + k).integers(0, len(AMINO), size=ROUND + WG_STARTS + k)].tobytes()
    h = oracle.seq_to_hashes_protein(data, k, "protein", 42, True)
    assert len(h) == ROUND + WG_STARTS + 1
    h.setflags(write=False)
    return data, h


@pytest.mark.parametrize("k,sep", [(10, False), (42, False), (10, True)])
def test_pair_kernel_appends_behind_a_flush(sm, k, sep):
    """sep: the size comes from the device and a 0xFF byte in workgroup 0's second round separates (the windows over it are
    dropped); otherwise every byte is a residue."""
    import torch
    from sourmash_amd.device import DeviceSketcher
    data, h = two_round_hashes(k)
    keep = (h >= 1) & (h <= np.uint64(oracle.max_hash_for_scaled(2)))
    ff = ROUND + 1000
    if sep:
        keep = keep.copy()
        keep[ff - k + 1:ff + 1] = False
    assert keep[:WG_STARTS].sum() >= FLUSH_AT, "workgroup 0 flushes behind its first round"
    assert keep[ROUND:ROUND + WG_STARTS].sum() >= 1, "workgroup 0 appends behind that flush"
    want_pos = np.flatnonzero(keep).astype(np.uint64)
    n = len(data)
    aa = torch.zeros((n + 7) // 8 * 8, dtype=torch.uint8, device="cuda")[:n]
    aa.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    if sep:
        aa[ff] = 0xFF
    cap = len(h)
    out_h = torch.zeros(cap, dtype=torch.int64, device="cuda")
    out_p = torch.zeros(cap, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    n_dev = torch.tensor([n], dtype=torch.int64, device="cuda") if sep else None
    DeviceSketcher(ksize=k, scaled=2).residue_kernel_only(aa, out_h, out_p, count, n_dev=n_dev)
    torch.cuda.synchronize()
    got_n = int(count.item())
    assert got_n == len(want_pos)
    got_p = out_p[:got_n].cpu().numpy().view(np.uint64)
    got_h = out_h[:got_n].cpu().numpy().view(np.uint64)
    order = np.argsort(got_p, kind="stable")
    assert np.array_equal(got_p[order], want_pos)
    assert np.array_equal(got_h[order], h[keep])


# ---- 5. SketchSet from a buffer and from files ---------------------------------------------------------------------------------------
def fasta_text(recs, width=60, eol=b"\n"):
    out = []
    for name, seq in recs:
        out.append(b">" + name.encode() + eol)
        for i in range(0, len(seq), width):
            out.append(seq[i:i + width] + eol)
    return b"".join(out)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    "3,000 records with CRLF line ends and wrapped lines, protein and DNA, plain and gzip"
    d = tmp_path_factory.mktemp("residue_records")
    rng = np.random.default_rng(11)
    out = {}
    for kind, make, lo, hi in (("faa", protein_record, 0, 500), ("fna", dna_record, 0, 900)):
        recs = []
        for i in range(3_000):
            n = 0 if i % 500 == 17 else int(rng.integers(lo, hi))
            seq = make(rng, n)
            if n > 100 and i % 7 == 0:
                seq[10:40] = np.frombuffer(bytes(seq[10:40]).lower(), dtype=np.uint8)
            recs.append((f"rec{i} len={n} some description", bytes(seq)))
        text = fasta_text(recs, eol=b"\r\n")
        (d / f"crlf.{kind}").write_bytes(text)
        (d / f"crlf.{kind}.gz").write_bytes(gzip.compress(text, 6))
        out[kind] = (str(d / f"crlf.{kind}"), recs)
        out[kind + "_gz"] = (str(d / f"crlf.{kind}.gz"), recs)
    out["golden_faa"] = (golden("genes", "ecoli.faa"), None)
    out["golden_fna"] = (golden("genes", "ecoli.genes.fna"), None)
    return out


def loop_signatures(sm, path, params, moltype, input_is_protein):
    "the record-by-record route: per-record sketch_records over read_records"
    return sm.sketch.sketch_records(list(sm.sketch.read_records(path)), params, filename=path, singleton=True, moltype=moltype,
                                    input_is_protein=input_is_protein)


@pytest.mark.parametrize("form", ["faa", "faa_gz", "fna", "fna_gz", "golden_faa", "golden_fna"])
def test_sketchset_from_file(sm, files, form):
    path, recs = files[form]
    is_protein = "faa" in form
    k, moltype, scaled = (10, "protein", 20) if is_protein else (16, "dayhoff", 20)
    read = list(sm.sketch.read_records(path))
    if recs is not None:
        assert read == recs
    ss = sm.index.SketchSet.sketch_file(path, ksize=k, scaled=scaled, moltype=moltype, input_is_protein=is_protein)
    want = loop_signatures(sm, path, f"{moltype},k={k},scaled={scaled}", moltype, is_protein)
    assert len(ss) == len(read) == len(want)
    assert ss.params == (k, moltype, 42, scaled, 0)
    assert np.array_equal(ss.sizes, [len(s.minhash) for s in want])
    for r in range(0, len(ss), max(1, len(ss) // 200)):
        assert np.array_equal(ss.minhash(r)._mins_array(), want[r].minhash._mins_array()), r
    man = ss.manifest
    assert [m["name"] for m in man] == [s.name for s in want] == [n for n, _ in read]
    assert all(m["filename"] == path and m["ksize"] == k and m["moltype"] == moltype and m["scaled"] == scaled for m in man)
    # ... and the oracle's rows
    want_h, want_o, _ = expected_csr([s for _, s in read], k, moltype, scaled, is_protein)
    assert ss.total_hashes == len(want_h) and np.array_equal(ss.sizes, np.diff(want_o))


def test_sketchset_from_buffer(sm):
    import torch
    buf, starts, ends = protein_boundaries(10, True)
    ss = sm.index.SketchSet.sketch_records(to_dev(torch, buf), to_dev(torch, starts), ksize=10, scaled=20, moltype="hp", is_protein=True,
                                           ends=to_dev(torch, ends))
    want_h, want_o, _ = expected_csr(records_of(buf, starts, ends), 10, "hp", 20, True)
    assert len(ss) == len(starts) - 1 and ss.total_hashes == len(want_h) and ss.params == (10, "hp", 42, 20, 0)
    for r in range(len(ss)):
        assert np.array_equal(ss.minhash(r)._mins_array(), want_h[int(want_o[r]):int(want_o[r + 1])]), r
    assert all(m["moltype"] == "hp" and m["ksize"] == 10 for m in ss.manifest)
    buf, starts, ends = translate_boundaries(7, False)
    ss = sm.index.SketchSet.sketch_records(to_dev(torch, buf), to_dev(torch, starts), ksize=7, scaled=20, moltype="protein")
    want_h, want_o, _ = expected_csr(records_of(buf, starts, None), 7, "protein", 20, False)
    assert np.array_equal(ss.sizes, np.diff(want_o))
    for r in range(len(ss)):
        assert np.array_equal(ss.minhash(r)._mins_array(), want_h[int(want_o[r]):int(want_o[r + 1])]), r


# ---- 6. sketch_file(singleton=True) ------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("form", ["faa", "fna_gz", "golden_faa", "golden_fna"])
@pytest.mark.parametrize("params", ["protein,k=10,scaled=20,abund", "dayhoff,k=16,scaled=20", "hp,k=42,scaled=20"])
def test_singleton_signatures_from_file(sm, files, form, params):
    path, _ = files[form]
    moltype, is_protein = params.split(",")[0], "faa" in form
    got = sm.sketch.sketch_file(path, params, singleton=True, moltype=moltype, input_is_protein=is_protein)
    assert_same_signatures(got, loop_signatures(sm, path, params, moltype, is_protein))


@pytest.mark.parametrize("form", ["faa_gz", "fna"])
def test_singleton_mixed_template(sm, files, form):
    "protein + dayhoff + hp sketches of two ksizes in one template: one pass per sketch over the same parsed buffer"
    import ctypes as C
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.signature import SourmashSignature
    from sourmash_amd.utils import rustcall
    path, _ = files[form]
    is_protein = "faa" in form
    params = sm.sketch.ComputeParameters(ksizes=[30, 48], seed=42, protein=True, dayhoff=True, hp=True, dna=False, num_hashes=0,
                                         track_abundance=True, scaled=20)
    n = C.c_size_t(0)
    ptr = rustcall(lib.smgpu_sketch_file_singleton_residues, path.encode(), params._get_objptr(), int(is_protein), C.byref(n))
    got = [SourmashSignature._from_objptr(ptr[i]) for i in range(n.value)]
    lib.nodegraph_buffer_free(C.cast(ptr, C.POINTER(C.c_uint8)), max(n.value, 1) * C.sizeof(C.c_void_p))
    want = []
    for name, seq in sm.sketch.read_records(path):
        sig = SourmashSignature.from_params(params)
        if is_protein:
            sig.add_protein(seq)
        else:
            sig.add_sequence(seq, True)
        sig.name, sig.filename = name, path
        want.append(sig)
    assert len(got[0].minhashes()) == 6
    assert_same_signatures(got, want)


@pytest.mark.parametrize("ext", [".zip", ".sig.gz"])
def test_sketch_file_to(sm, files, tmp_path, ext):
    path, recs = files["faa"]
    out = str(tmp_path / ("proteome" + ext))
    n = sm.sketch.sketch_file_to(path, out, "protein,k=10,scaled=20", moltype="protein", input_is_protein=True)
    assert n == len(recs)
    back = sm.index.SketchSet.load([out], moltype="protein")
    direct = sm.index.SketchSet.sketch_file(path, ksize=10, scaled=20, moltype="protein", input_is_protein=True)
    assert len(back) == len(direct) and np.array_equal(back.sizes, direct.sizes)
    assert back.params == direct.params
    assert [m["name"] for m in back.manifest] == [m["name"] for m in direct.manifest]
    for r in range(0, len(back), 37):
        assert np.array_equal(back.minhash(r)._mins_array(), direct.minhash(r)._mins_array())


# ---- 7. what stays record by record ------------------------------------------------------------------------------------------------
def test_k80_and_num_go_record_by_record(sm, files, tmp_path):
    path, recs = files["faa"]
    short = str(tmp_path / "short.faa")
    with open(short, "wb") as f:
        f.write(fasta_text(recs[:60]))
    for params in ("protein,k=80,scaled=5", "protein,k=10,num=50"):
        got = sm.sketch.sketch_file(short, params, singleton=True, moltype="protein", input_is_protein=True)
        assert_same_signatures(got, loop_signatures(sm, short, params, "protein", True))
    ss = sm.index.SketchSet.sketch_file(short, ksize=80, scaled=5, moltype="protein", input_is_protein=True)
    want_h, want_o, _ = expected_csr([s for _, s in recs[:60]], 80, "protein", 5, True)
    assert np.array_equal(ss.sizes, np.diff(want_o)) and [m["moltype"] for m in ss.manifest] == ["protein"] * 60
    import torch
    from sourmash_amd.exceptions import SourmashError
    with pytest.raises(SourmashError, match="1 .. 79"):
        sm.device.DeviceSketcher(ksize=80, scaled=5).sketch_records(torch.zeros(100, dtype=torch.uint8, device="cuda"),
                                                                    to_dev(torch, np.asarray([0, 100], dtype=np.int64)), moltype="protein",
                                                                    is_protein=True)


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(sm):
    import torch
    rng = np.random.default_rng(3)
    seq = to_dev(torch, protein_record(rng, 1000))
    sk = sm.device.DeviceSketcher(ksize=10, scaled=1)
    dev = lambda v: to_dev(torch, np.asarray(v, dtype=np.int64))   # noqa: E731
    kw = dict(moltype="protein", is_protein=True)
    for ends in ([99, 900], [500, 1001], [501, 1000]):               # in front of its start; behind the next start (twice)
        with pytest.raises(ValueError, match="record ends"):
            sk.sketch_records(seq, dev([100, 500, 1000]), ends=dev(ends), **kw)
        with pytest.raises(ValueError, match="record ends"):
            sm.index.SketchSet.sketch_records(seq, dev([100, 500, 1000]), ksize=10, scaled=1, ends=dev(ends), **kw)
    with pytest.raises(ValueError, match="record starts: the offsets are not ascending"):
        sk.sketch_records(seq, dev([0, 600, 500, 1000]), **kw)
    with pytest.raises(ValueError, match=r"record starts: the last offset lies behind the end of the buffer \(1000 bytes\)"):
        sk.sketch_records(seq, dev([0, 500, 1001]), moltype="protein", is_protein=False)
    # capacity too small: the error names the count
    from sourmash_amd._lowlevel import decode_str, lib
    from sourmash_amd.device import _ptr, _stream
    starts = dev([0, 1000])
    cap = 100
    hashes = torch.zeros(cap, dtype=torch.int64, device="cuda")
    offsets = torch.zeros(2, dtype=torch.int64, device="cuda")
    result = torch.zeros(4, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.smgpu_sketch_residue_records_workspace_bytes(cap, 1, 1000, 0)), dtype=torch.uint8, device="cuda")
    lib.sourmash_err_clear()
    got = lib.smgpu_sketch_residue_records_raw(_ptr(seq), 1000, _ptr(starts), None, 1, 10, 2, 0, 42, 0, _ptr(hashes), None, cap, _ptr(offsets),
                                               _ptr(result), _ptr(ws), ws.numel(), _stream(torch))
    assert got == 2**64 - 1 and lib.sourmash_err_get_last_code() != 0
    message = decode_str(lib.sourmash_err_get_last_message())
    assert "output capacity too small: 991 kept pairs > capacity 100" in message, message
    assert int(result[0].item()) == 991
    lib.sourmash_err_clear()


def test_residue_entries_refuse_a_dna_hash_function(sm, files):
    """The residue entries of the C-ABI serve protein, dayhoff and hp alone: hash_function 1 (DNA; also 0 and 5) is an error with
    the residue pass's text, and the window length is held to 1 .. 79 residues whatever the hash_function.  (Python sends DNA
    to the DNA entries, so only a direct call gets here.)"""
    import os
    import torch
    from sourmash_amd._lowlevel import decode_str, lib
    from sourmash_amd.device import _ptr
    seq = to_dev(torch, protein_record(np.random.default_rng(4), 1000))
    starts = to_dev(torch, np.asarray([0, 400, 1000], dtype=np.int64))
    path = os.fsencode(files["faa"][0])
    torch.cuda.synchronize()

    def refused(call, text):
        lib.sourmash_err_clear()
        ptr = call()
        assert not ptr and lib.sourmash_err_get_last_code() != 0
        message = decode_str(lib.sourmash_err_get_last_message())
        lib.sourmash_err_clear()
        assert text in message, message

    not_residue = "per-record residue sketches are protein, dayhoff or hp sketches"
    for hf in (1, 0, 5):
        for translate in (0, 1):
            refused(lambda: lib.smgpu_sketchset_sketch_residue_records(_ptr(seq), 1000, _ptr(starts), None, 2, 10, hf, translate, 42, 20), not_residue)
            refused(lambda: lib.smgpu_sketchset_sketch_residue_file(path, 10, hf, translate, 42, 20), not_residue)
    too_long = "per-record residue sketches take ksize 1 .. 79 residues, not 80"
    for hf in (1, 2):
        refused(lambda: lib.smgpu_sketchset_sketch_residue_records(_ptr(seq), 1000, _ptr(starts), None, 2, 80, hf, 0, 42, 20), too_long)
        refused(lambda: lib.smgpu_sketchset_sketch_residue_file(path, 80, hf, 0, 42, 20), too_long)


# ---- 9. downstream -----------------------------------------------------------------------------------------------------------------
def test_search_many_and_compare(sm, files):
    path, recs = files["faa"]
    ss = sm.index.SketchSet.sketch_file(path, ksize=10, scaled=20, moltype="protein", input_is_protein=True)
    loop = loop_signatures(sm, path, "protein,k=10,scaled=20", "protein", True)
    ref = sm.index.SketchSet([s.minhash for s in loop])
    a, b = ss.compare(jaccard=False), ref.compare(jaccard=False)
    assert np.array_equal(a[0], b[0])
    rows = [5, 100, 2_999]
    queries = sm.index.SketchSet([loop[r].minhash for r in rows])
    got = ss.search_many(queries, threshold=0.1, do_containment=True)
    assert got == ref.search_many(queries, threshold=0.1, do_containment=True)
    assert all(hits and hits[0][0] == 1.0 for hits, r in zip(got, rows) if len(loop[r].minhash))
