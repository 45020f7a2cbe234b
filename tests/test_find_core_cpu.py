"""CPU checks of k-mer finding (csrc/sketch_find.hip): the membership rule compiled for the host against numpy.isin, the
directory's invariants, the C interface, and the Python entry points without a device.  None of this needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sourmash_amd
from sourmash_amd._lowlevel import lib
from sourmash_amd.minhash import _get_max_hash_for_scaled

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "native", "find_core_emul.cpp")

PROTOTYPES = [
    "SmgpuKmerQuery *smgpu_kmerquery_new(const SourmashKmerMinHash *const *mhs, uintptr_t n);",
    "void smgpu_kmerquery_free(SmgpuKmerQuery *ptr);",
    "uint64_t smgpu_kmerquery_len(const SmgpuKmerQuery *ptr);",
    "uint64_t smgpu_find_kmers_workspace_bytes(uint64_t pair_capacity, uint64_t n_records);",
    "uint64_t smgpu_find_kmers_raw(const SmgpuKmerQuery *query, const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, "
    "uint64_t n_records, uint64_t *d_positions, uint64_t *d_hashes, uint8_t *d_kmers, uint64_t capacity, uint64_t *d_offsets, "
    "uint64_t *d_result, void *d_workspace, uint64_t workspace_bytes, void *stream);",
    "void smgpu_find_kmers_kernel_raw(const SmgpuKmerQuery *query, const uint8_t *d_seq, uint64_t len, uint64_t *d_hashes, "
    "uint64_t *d_positions, uint64_t capacity, uint64_t *d_count, uint32_t grid, void *stream);",
    "SmgpuKmerMatches *smgpu_find_kmers_file(const SmgpuKmerQuery *query, const char *path);",
    "void smgpu_kmermatches_free(SmgpuKmerMatches *ptr);",
    "uint64_t smgpu_kmermatches_n_records(const SmgpuKmerMatches *ptr);",
    "uint64_t smgpu_kmermatches_n_rows(const SmgpuKmerMatches *ptr);",
    "uint64_t smgpu_kmermatches_n_bases(const SmgpuKmerMatches *ptr);",
    "const uint64_t *smgpu_kmermatches_offsets(const SmgpuKmerMatches *ptr);",
    "const uint64_t *smgpu_kmermatches_positions(const SmgpuKmerMatches *ptr);",
    "const uint64_t *smgpu_kmermatches_hashes(const SmgpuKmerMatches *ptr);",
    "const uint8_t *smgpu_kmermatches_kmers(const SmgpuKmerMatches *ptr);",
    "const uint64_t *smgpu_kmermatches_record_lengths(const SmgpuKmerMatches *ptr);",
    "SourmashStr smgpu_kmermatches_record_name(const SmgpuKmerMatches *ptr, uint64_t record);",
    "const uint8_t *smgpu_kmermatches_record_sequence(const SmgpuKmerMatches *ptr, uint64_t record, uint64_t *len);",
]


def _norm(s):
    return " ".join(s.replace("( ", "(").replace(" )", ")").split())


def test_prototypes_declared_and_exported():
    with open(os.path.join(ROOT, "include", "sourmash_amd.h")) as f:
        header = _norm(f.read())
    so = C.CDLL(os.path.join(ROOT, "sourmash_amd", "libsourmash_amd.so"))
    assert len(PROTOTYPES) == 18
    for p in PROTOTYPES:
        assert _norm(p) in header, p
        name = p.split("(")[0].split()[-1].lstrip("*")
        assert hasattr(so, name), name
        assert name in lib.functions, name                     # the binding parsed it


def test_golden_fixture_is_the_recorded_file():
    """tests/golden/kmers/short.fa is data of the reference (its tests/test-data/short.fa), recorded with its checksum in the
    folder's own MANIFEST.json, in the format of tests/golden/MANIFEST.json."""
    import hashlib
    import json
    with open(os.path.join(HERE, "golden", "kmers", "MANIFEST.json")) as f:
        entries = json.load(f)
    assert [e["file"] for e in entries] == ["kmers/short.fa"]
    with open(os.path.join(HERE, "golden", entries[0]["file"]), "rb") as f:
        data = f.read()
    assert len(data) == 1012 and hashlib.sha256(data).hexdigest() == entries[0]["sha256"]
    assert entries[0]["sha256"] == "85330abbbf8845fb2ba535465641dfd9cab1d7bc02ecf81450ff14aa8ec80c3e"


# ---- the membership rule, compiled for the host -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("find_core") / "libfind_core_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so_path, SRC])
    so = C.CDLL(so_path)
    so.emul_find_dir_shift.argtypes = [C.c_uint64, C.c_uint64]
    so.emul_find_dir_shift.restype = C.c_uint32
    so.emul_find_dir_buckets.argtypes = [C.c_uint64, C.c_uint32]
    so.emul_find_dir_buckets.restype = C.c_uint64
    so.emul_find_max_buckets.restype = C.c_uint64
    so.emul_find_dir.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p]
    so.emul_find_member.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    so.emul_find_member.restype = C.c_uint64
    return so


def expected_buckets(n, max_hash):
    """The bucket count the rule asks for, from the counts the shifts offer: the smallest one >= n -- which is at most 2 n + 1 --
    and, where that is above 2^24, the largest one within 2^24."""
    offered = [(max_hash >> s) + 1 for s in range(64)]
    want = min(v for v in offered if v >= n)
    if want <= 2**24:
        assert n <= want <= 2 * n + 1
        return want
    return max(v for v in offered if v <= 2**24)


def directory(emul, q, max_hash):
    "-> (shift, nb, dir) of the sorted distinct hashes q, with the invariants every directory must keep"
    n = len(q)
    shift = emul.emul_find_dir_shift(n, max_hash)
    nb = emul.emul_find_dir_buckets(max_hash, shift)
    assert nb == (max_hash >> shift) + 1 == expected_buckets(n, max_hash)
    assert emul.emul_find_max_buckets() == 2**24
    d = np.full(nb + 1, 0xffffffff, dtype=np.uint32)
    emul.emul_find_dir(q.ctypes.data, n, shift, nb, d.ctypes.data)
    assert d[0] == 0 and d[nb] == n
    assert np.all(np.diff(d.astype(np.int64)) >= 0)                # monotone
    # dir[b] is the first index with q[i] >> shift >= b
    assert np.array_equal(d, np.searchsorted(q >> np.uint64(shift), np.arange(nb + 1, dtype=np.uint64), side="left").astype(np.uint32))
    return shift, nb, d


def members(emul, q, max_hash, probes):
    shift, nb, d = directory(emul, q, max_hash)
    probes = np.ascontiguousarray(probes, dtype=np.uint64)
    out = np.zeros(len(probes), dtype=np.uint8)
    outside = emul.emul_find_member(q.ctypes.data, d.ctypes.data, shift, nb, max_hash, probes.ctypes.data, len(probes), out.ctypes.data)
    assert outside == 0                                            # no lookup reads outside dir[0 .. nb]
    return out.astype(bool)


def check_query(emul, q, max_hash):
    "every member, member +- 1, 0, max_hash + 1 and 2^64 - 1 against numpy.isin"
    q = np.unique(np.asarray(q, dtype=np.uint64))
    assert q[0] >= 1 and q[-1] <= max_hash
    probes = np.concatenate([q, q - np.uint64(1), q + np.uint64(1),                      # (wraps at the ends: still probes)
                             np.array([0, (max_hash + 1) % 2**64, 2**64 - 1, 1, max_hash], dtype=np.uint64)])
    want = np.isin(probes, q) & (probes != 0) & (probes <= np.uint64(max_hash))
    got = members(emul, q, max_hash, probes)
    assert np.array_equal(got, want), (len(q), max_hash, np.flatnonzero(got != want)[:5])
    assert got[:len(q)].all()


SIZES = sorted({1, 2, 3} | {2**e + d for e in range(2, 18) for d in (-1, 0, 1)})


@pytest.mark.parametrize("scaled", [1, 10, 1000])
def test_member_uniform_queries(emul, scaled):
    max_hash = _get_max_hash_for_scaled(scaled)
    rng = np.random.default_rng(scaled)
    assert SIZES[-1] == 2**17 + 1
    for n in SIZES:
        q = rng.integers(1, max_hash, size=n, dtype=np.uint64, endpoint=True)
        check_query(emul, q, max_hash)


@pytest.mark.parametrize("scaled", [1, 10, 1000])
def test_member_clustered_and_end_hashes(emul, scaled):
    max_hash = _get_max_hash_for_scaled(scaled)
    rng = np.random.default_rng(7 + scaled)
    # 5,000 consecutive integers: all in one bucket, whatever the shift of a 5,000-hash query
    start = int(rng.integers(1, max_hash - 10_000, dtype=np.uint64))
    run = np.arange(start, start + 5000, dtype=np.uint64)
    shift, nb, d = directory(emul, run, max_hash)
    assert np.count_nonzero(np.diff(d.astype(np.int64))) <= 2 and np.diff(d.astype(np.int64)).max() >= 2500
    check_query(emul, run, max_hash)
    # the run inside a uniform query, and the ends of the hash range themselves
    uniform = rng.integers(1, max_hash, size=3000, dtype=np.uint64, endpoint=True)
    check_query(emul, np.concatenate([run, uniform]), max_hash)
    check_query(emul, np.array([1, max_hash], dtype=np.uint64), max_hash)
    check_query(emul, np.concatenate([np.array([1, 2, max_hash - 1, max_hash], dtype=np.uint64), uniform]), max_hash)
    check_query(emul, np.array([1], dtype=np.uint64), max_hash)
    check_query(emul, np.array([max_hash], dtype=np.uint64), max_hash)


def test_directory_bucket_count(emul):
    "the smallest bucket count >= n the shifts offer, within [n, 2 n + 1], until the 2^24 cap"
    for scaled in (1, 2, 10, 1000, 10**6):
        max_hash = _get_max_hash_for_scaled(scaled)
        for n in (1, 2, 3, 5, 1000, 5000, 2**17, 10**6, 2**23, 2**23 + 2, 2**24 - 1, 2**24, 2**24 + 1, 10**7, 10**8, 2**32 - 2):
            nb = emul.emul_find_dir_buckets(max_hash, emul.emul_find_dir_shift(n, max_hash))
            assert nb == expected_buckets(n, max_hash), (scaled, n, nb)
            assert nb <= 2**24 and (n <= nb <= 2 * n + 1 or nb > 2**23), (scaled, n, nb)   # capped: several hashes per bucket
    # tiny hash ranges
    for max_hash in (1, 2, 3, 255):
        for n in range(1, max_hash + 1):
            nb = emul.emul_find_dir_buckets(max_hash, emul.emul_find_dir_shift(n, max_hash))
            assert nb == expected_buckets(n, max_hash) and n <= nb <= 2 * n + 1


def test_member_beyond_the_cap(emul):
    "a directory at its cap holds several hashes per bucket and stays exact (max_hash small enough that 2^24 buckets are few)"
    max_hash = 2**20 - 1                       # shift 0 would give 2^20 buckets; the query fills a quarter of the range
    rng = np.random.default_rng(3)
    q = np.unique(rng.integers(1, max_hash, size=2**18, dtype=np.uint64, endpoint=True))
    check_query(emul, q, max_hash)


# ---- the Python layer without a device -----------------------------------------------------------------------------------------
def test_kmerquery_argument_errors():
    from sourmash_amd import KmerQuery, MinHash
    a = MinHash(0, 31, scaled=1000)
    a.add_many([5, 7, 11])
    with pytest.raises(ValueError, match="no hashes in query signature"):
        KmerQuery([MinHash(0, 31, scaled=1000)])
    with pytest.raises(ValueError, match="no signatures"):
        KmerQuery([])
    num = MinHash(500, 31)
    num.add_many([5, 7])
    with pytest.raises(ValueError, match="num"):
        KmerQuery([num])
    with pytest.raises(ValueError, match="num"):
        KmerQuery([a, num])
    for kw, name in ((dict(is_protein=True), "protein"), (dict(dayhoff=True), "dayhoff"), (dict(hp=True), "hp")):
        p = MinHash(0, 7, scaled=1000, **kw)
        p.add_many([5])
        with pytest.raises(ValueError, match=name):
            KmerQuery([p])
    b = MinHash(0, 21, scaled=1000)
    b.add_many([5])
    with pytest.raises(ValueError, match="ksize"):
        KmerQuery([a, b])
    c = MinHash(0, 31, scaled=100)
    c.add_many([5])
    with pytest.raises(ValueError, match="scaled"):
        KmerQuery([a, c])
    with pytest.raises(TypeError):
        KmerQuery(["not a sketch"])
    # the C entry refuses the same on its own
    for mh in (MinHash(0, 31, scaled=1000), num):
        lib.sourmash_err_clear()
        assert lib.smgpu_kmerquery_new((C.c_void_p * 1)(mh._get_objptr()), 1) is None
        assert 100 <= lib.sourmash_err_get_last_code() <= 10000            # the codes that arrive as ValueError
    lib.sourmash_err_clear()


def test_kmerquery_is_the_merged_sketch():
    from sourmash_amd import KmerQuery, MinHash, SourmashSignature
    a = MinHash(0, 31, scaled=1000, track_abundance=True)
    a.set_abundances({5: 3, 7: 2})
    b = MinHash(0, 31, scaled=1000)
    b.add_many([7, 11, 2**40])
    q = KmerQuery([SourmashSignature(a, name="a"), b])
    assert len(q) == 4 and (q.ksize, q.scaled, q.seed) == (31, 1000, 42)
    assert not q.minhash.track_abundance and list(q.minhash.hashes) == [5, 7, 11, 2**40]
    assert a.track_abundance and a.hashes[5] == 3                            # the caller's sketches are left as they were
    assert len(KmerQuery(b)) == 3


def test_entry_points_raise_without_gpu(tmp_path):
    if sourmash_amd.gpu_available():
        pytest.skip("a GPU is present: the calls succeed (covered by tests/test_gpu_find.py)")
    from sourmash_amd import KmerQuery, MinHash, find_kmers
    from sourmash_amd.exceptions import SourmashError
    fa = tmp_path / "two.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n>b\nTTTTACGTACGGGGTACGTACGTACCCCGTACGTAC\n")
    mh = MinHash(0, 21, scaled=1)
    mh.add_many([5, 7])
    q = KmerQuery([mh])
    with pytest.raises(SourmashError, match="no HIP device"):
        q.find_file(str(fa))
    with pytest.raises(SourmashError, match="no HIP device"):
        find_kmers([mh], [str(fa)])
    with pytest.raises(RuntimeError, match="HIP device"):
        q.find(None, None)
    long = MinHash(0, 101, scaled=1)
    long.add_many([5])
    fa_long = tmp_path / "long.fa"
    fa_long.write_text(">a\n" + "ACGTTGCA" * 20 + "\n")
    with pytest.raises(SourmashError, match="no HIP device"):                # k > 88 hashes on the device as well
        KmerQuery([long]).find_file(str(fa_long))
    lib.sourmash_err_clear()
    assert lib.smgpu_find_kmers_file(q._ptr, str(fa).encode()) is None
    assert lib.sourmash_err_get_last_code() != 0
    lib.sourmash_err_clear()
