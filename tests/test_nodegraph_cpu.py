"""CPU checks of sourmash_amd.Nodegraph (csrc/nodegraph_host.hpp): the C interface, table sizes, khmer's two-bit hash, the
file format against files khmer wrote, the SBT internal nodes rebuilt from their leaves, and the kernels' reduction h mod d
compiled for the host.  None of this needs a GPU."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import golden

import sourmash_amd
from sourmash_amd import Nodegraph, MinHash
from sourmash_amd._lowlevel import lib
from sourmash_amd.nodegraph import extract_nodegraph_info, calc_expected_collisions

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
NG = golden("nodegraph")
SBT = os.path.join(NG, "sbt_v3")

# the reference's nodegraph_* prototypes (include/sourmash.h), written out here
PROTOTYPES = [
    "bool nodegraph_count(SourmashNodegraph *ptr, uint64_t h);",
    "bool nodegraph_count_kmer(SourmashNodegraph *ptr, const char *kmer);",
    "double nodegraph_expected_collisions(const SourmashNodegraph *ptr);",
    "void nodegraph_free(SourmashNodegraph *ptr);",
    "SourmashNodegraph *nodegraph_from_buffer(const char *ptr, uintptr_t insize);",
    "SourmashNodegraph *nodegraph_from_path(const char *filename);",
    "uintptr_t nodegraph_get(const SourmashNodegraph *ptr, uint64_t h);",
    "uintptr_t nodegraph_get_kmer(const SourmashNodegraph *ptr, const char *kmer);",
    "const uint64_t *nodegraph_hashsizes(const SourmashNodegraph *ptr, uintptr_t *size);",
    "uintptr_t nodegraph_ksize(const SourmashNodegraph *ptr);",
    "uintptr_t nodegraph_matches(const SourmashNodegraph *ptr, const SourmashKmerMinHash *mh_ptr);",
    "SourmashNodegraph *nodegraph_new(void);",
    "uintptr_t nodegraph_noccupied(const SourmashNodegraph *ptr);",
    "uintptr_t nodegraph_ntables(const SourmashNodegraph *ptr);",
    "void nodegraph_save(const SourmashNodegraph *ptr, const char *filename);",
    "const uint8_t *nodegraph_to_buffer(const SourmashNodegraph *ptr, uint8_t compression, uintptr_t *size);",
    "void nodegraph_update(SourmashNodegraph *ptr, const SourmashNodegraph *optr);",
    "void nodegraph_update_mh(SourmashNodegraph *ptr, const SourmashKmerMinHash *optr);",
    "SourmashNodegraph *nodegraph_with_tables(uintptr_t ksize, uintptr_t starting_size, uintptr_t n_tables);",
]

# SBT v3 (d = 2): internal node i has children 2i + 1 and 2i + 2; nodes 6 .. 12 are the leaves (v3.sbt.json)
LEAVES = {6: "6d6e87e1154e95b279e5e7db414bc37b", 7: "60f7e23c24a8d94791cc7a8680c493f9", 8: "0107d767a345eff67ecdaed2ee5cd7ba",
          9: "f71e78178af9e45e6f1d87a0c53c465c", 10: "f0c834bc306651d2b9321fb21d3e8d8f",
          11: "4e94e60265e04f0763142e20b52c0da1", 12: "b59473c94ff2889eca5d7165936e64b3"}


def leaves_under(i):
    if i in LEAVES:
        return [i]
    return leaves_under(2 * i + 1) + leaves_under(2 * i + 2)


def leaf_mh(i):
    with open(os.path.join(SBT, LEAVES[i])) as f:
        sigs = sourmash_amd.load_signatures_from_json(f.read())
    sigs = list(sigs)
    assert len(sigs) == 1
    return sigs[0].minhash


def read(path):
    with open(path, "rb") as f:
        return f.read()


def _norm(s):
    return " ".join(s.replace("( ", "(").replace(" )", ")").split())


def test_prototypes_declared_and_exported():
    with open(os.path.join(ROOT, "include", "sourmash_amd.h")) as f:
        header = _norm(f.read())
    so = C.CDLL(os.path.join(ROOT, "sourmash_amd", "libsourmash_amd.so"))
    assert len(PROTOTYPES) == 19
    for p in PROTOTYPES:
        assert _norm(p) in header, p
        name = p.split("(")[0].split()[-1].lstrip("*")
        assert hasattr(so, name), name
    assert "typedef struct SourmashNodegraph SourmashNodegraph;" in header


# ---- table sizes ------------------------------------------------------------------------------------------------------------
def _is_prime(n):
    "deterministic Miller-Rabin for n < 3.3e24"
    if n < 2:
        return False
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in bases:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in bases:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _model_sizes(starting_size, n_tables):
    out = []
    i = max(starting_size - 1, 2)
    if i % 2 == 0:
        i -= 1
    while len(out) != n_tables:
        if _is_prime(i):
            out.append(i)
        if i == 1:
            break
        i -= 2
    return out


def _table_sizes(starting_size, n_tables):
    out = (C.c_uint64 * max(n_tables, 1))()
    n = lib.smgpu_nodegraph_table_sizes(starting_size, n_tables, out, n_tables)
    return [out[i] for i in range(min(n, n_tables))]


@pytest.mark.parametrize("start,n,want", [(23, 6, [19, 17, 13, 11, 7, 5]), (100000, 4, [99991, 99989, 99971, 99961]),
                                          (5, 6, [3]), (3, 6, []), (2**32 + 16, 1, [4294967311])])
def test_with_tables_sizes(start, n, want):
    assert Nodegraph(3, start, n).hashsizes() == want
    assert _table_sizes(start, n) == want


@pytest.mark.parametrize("start", [10**12, 2**40, 2**62, 2**64 - 1, 1000003])
def test_large_table_sizes_match_miller_rabin(start):
    assert _table_sizes(start, 5) == _model_sizes(start, 5)


def test_bad_starting_sizes_raise():
    with pytest.raises(Exception):
        Nodegraph(3, 0, 2)
    with pytest.raises(Exception):
        Nodegraph(3, 2**62, 1)          # 2^59 bytes


def test_new_graph_has_no_tables():
    p = lib.nodegraph_new()
    try:
        assert lib.nodegraph_ksize(p) == 0
        assert lib.nodegraph_ntables(p) == 0
        assert lib.nodegraph_get(p, 12345) == 1
    finally:
        lib.nodegraph_free(p)
    g = Nodegraph(3, 3, 6)
    assert g.hashsizes() == [] and g.get(7) == 1
    with pytest.raises(Exception):
        g.expected_collisions


# ---- two-bit hash ------------------------------------------------------------------------------------------------------------
CODE = {"A": 0, "T": 1, "C": 2, "G": 3}
M64 = 2**64 - 1


def twobit(s):
    fw = rv = 0
    for c in s:
        fw = ((fw << 2) | CODE[c]) & M64
    for c in reversed(s):
        rv = ((rv << 2) | (CODE[c] ^ 1)) & M64
    return min(fw, rv)


def set_bits(g):
    "{table index: sorted set bit positions} read from to_bytes(0)"
    raw = g.to_bytes(0)
    pos = 4 + 1 + 1 + 4 + 1 + 8
    out = []
    for size in g.hashsizes():
        assert int.from_bytes(raw[pos:pos + 8], "little") == size
        pos += 8
        nb = size // 8 + 1
        bits = np.unpackbits(np.frombuffer(raw[pos:pos + nb], dtype=np.uint8), bitorder="little")
        out.append(np.flatnonzero(bits[:size]).tolist())
        pos += nb
    assert pos == len(raw)
    return out


def test_twobit_hash_matches_model():
    rng = random.Random(7)
    for n in list(range(1, 41)) + [64, 100]:
        s = "".join(rng.choice("ACGT") for _ in range(n))
        g = Nodegraph(n, 10**6, 2)
        assert g.count(s) is True
        h = twobit(s)
        assert set_bits(g) == [[h % sz] for sz in g.hashsizes()], (n, s)
        assert g.get(s) == 1 and g.get(h) == 1
        assert g.n_occupied() == 1
        assert g.count(s) is False


def test_bad_kmer_raises_and_counts_nothing():
    g = Nodegraph(4, 10**6, 2)
    before = g.to_bytes(0)
    for bad in ("ACGN", "acgt", "AC-T", "ACGTx"):
        with pytest.raises(ValueError):
            g.count(bad)
        with pytest.raises(ValueError):
            g.get(bad)
    assert g.to_bytes(0) == before and g.n_occupied() == 0


# ---- khmer's file ------------------------------------------------------------------------------------------------------------
def test_khmer_file_bytes():
    g = Nodegraph(3, 23, 6)
    for k in ("ACG", "TTA", "CGA"):
        g.count(k)
    raw = read(os.path.join(NG, "khmer_3_23_6.ng"))
    assert len(raw) == 79
    assert g.to_bytes(0) == raw
    assert gzip.decompress(g.to_bytes()) == raw
    assert gzip.decompress(g.to_bytes(12)) == raw


@pytest.mark.parametrize("name", ["khmer_3_23_6.ng", "khmer_3_23_6.ng.gz"])
def test_khmer_file_loads(name, tmp_path):
    path = os.path.join(NG, name)
    assert len(read(path)) == (79 if name.endswith(".ng") else 69)
    for g in (Nodegraph.load(path), Nodegraph.from_buffer(read(path))):
        assert g.hashsizes() == [19, 17, 13, 11, 7, 5]
        assert g.ksize() == 3
        assert g.get("ACG") and g.get("TTA") and g.get("CGA")
        out = tmp_path / "x.ng"
        g.save(str(out))
        assert read(str(out)) == read(os.path.join(NG, "khmer_3_23_6.ng"))


def test_bad_files_raise():
    raw = read(os.path.join(NG, "khmer_3_23_6.ng"))
    for bad in (b"OXLJ" + raw[4:], raw[:4] + b"\x05" + raw[5:], raw[:5] + b"\x01" + raw[6:], raw[:40], b""):
        with pytest.raises(Exception):
            Nodegraph.from_buffer(bad)


# ---- the SBT fixtures -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(6))
def test_sbt_round_trip(i, tmp_path):
    path = os.path.join(SBT, f"internal.{i}")
    data = read(path)
    assert len(data) == 50042
    g = Nodegraph.load(path)
    assert g.to_bytes(0) == data
    out = tmp_path / "n.ng"
    g.save(str(out))
    assert read(str(out)) == data
    assert Nodegraph.from_buffer(g.to_bytes()).to_bytes(0) == data
    assert Nodegraph.from_buffer(gzip.compress(data)).to_bytes(0) == data


def test_sbt_internal0_numbers():
    path = os.path.join(SBT, "internal.0")
    g = Nodegraph.load(path)
    assert g.n_occupied() == 2416
    assert g.ksize() == 1
    assert g.hashsizes() == [99991, 99989, 99971, 99961]
    assert g.expected_collisions == 3.412442571740036e-07
    assert calc_expected_collisions(g) == 3.412442571740036e-07
    with pytest.raises(SystemExit):
        calc_expected_collisions(g, max_false_pos=1e-8)
    assert extract_nodegraph_info(path) == (1, 100000, 4, 4, 2, 2416)
    assert g.get(1877811740) == 0
    assert g.get(1877811749) == 1 and g.get(801084876663808) == 1


def test_update_of_children_gives_parent_tables():
    parent = Nodegraph.load(os.path.join(SBT, "internal.0"))
    g = Nodegraph(1, 100000, 4)
    g.update(Nodegraph.load(os.path.join(SBT, "internal.1")))
    g.update(Nodegraph.load(os.path.join(SBT, "internal.2")))
    assert set_bits(g) == set_bits(parent)
    assert g.n_occupied() == len(set_bits(parent)[0])
    with pytest.raises(TypeError):
        g.update(42)


@pytest.mark.parametrize("i", range(6))
def test_host_update_mh_of_leaves_gives_internal_node(i):
    g = Nodegraph(1, 100000, 4)
    for leaf in leaves_under(i):
        g.update(leaf_mh(leaf))
    assert g.to_bytes(0) == read(os.path.join(SBT, f"internal.{i}"))


def test_matches_host():
    g = Nodegraph.load(os.path.join(SBT, "internal.0"))
    for leaf in LEAVES:
        mh = leaf_mh(leaf)
        assert g.matches(mh) == len(mh.hashes)
    with pytest.raises(ValueError):
        g.matches(42)
    mh = MinHash(0, 31, scaled=1)
    mh.add_many([1, 2, 3, 1877811749])
    assert g.matches(mh) == sum(g.get(h) for h in (1, 2, 3, 1877811749))


def test_containment_and_similarity():
    a = Nodegraph(3, 32, 1)
    b = Nodegraph(3, 32, 1)
    assert a.hashsizes() == [31]
    for i in range(20):
        if i % 2 == 0:
            a.count(i)
        b.count(i)
    assert a.containment(b) == 1.0
    assert a.similarity(b) == 0.5


def test_bulk_ksize_limit_raises_without_gpu():
    for k in (0, 33):
        g = Nodegraph(k, 1000, 2)
        with pytest.raises(ValueError, match="32"):
            g.add_sequence("ACGT" * 20)


# ---- the kernels' reduction, compiled for the host ------------------------------------------------------------------------------
SRC = os.path.join(HERE, "native", "nodegraph_mod_emul.cpp")
SO = os.path.join(HERE, "native", "libnodegraph_mod_emul.so")
HDR = os.path.join(ROOT, "sourmash_amd", "csrc", "nodegraph_core.hpp")


@pytest.fixture(scope="module")
def emul():
    newest = max(os.path.getmtime(p) for p in (SRC, HDR))
    if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    so = C.CDLL(SO)
    so.emul_ng_mod.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    so.emul_ng_codes.argtypes = [C.c_void_p]
    return so


def test_reduction_is_exact(emul):
    rng = random.Random(11)
    ds = [3, 5, 7, 31, 99991, 2**31 - 1, 2**32 - 5, 4294967311, 2**33 + 17, 10**12 + 39, 2**62 - 57, 2**62 + 135,
          2**63 - 25, 2**63 - 1]
    ds += [rng.randrange(3, 2**63) for _ in range(40)] + [rng.randrange(3, 2**20) for _ in range(20)]
    for d in ds:
        hs = {0, 1, d - 1, d, d + 1, 2**64 - 1, 2**64 - 2, 2**63, 2**63 - 1, 2**32, 2**32 - 1}
        q_max = (2**64 - 1) // d
        for q in (1, 2, 3, q_max, q_max - 1, max(q_max // 2, 1)) + tuple(rng.randrange(1, q_max + 1) for _ in range(20)):
            for e in (-1, 0, 1):
                v = q * d + e
                if 0 <= v < 2**64:
                    hs.add(v)
        hs |= {rng.randrange(0, 2**64) for _ in range(200)}
        hs = sorted(hs)
        a = np.array(hs, dtype=np.uint64)
        out = np.zeros_like(a)
        emul.emul_ng_mod(a.ctypes.data, len(a), d, out.ctypes.data)
        assert out.tolist() == [h % d for h in hs], d


def test_base_codes(emul):
    out = np.zeros(256, dtype=np.uint8)
    emul.emul_ng_codes(out.ctypes.data)
    want = np.full(256, 255, dtype=np.uint8)
    for c, v in CODE.items():
        want[ord(c)] = want[ord(c.lower())] = v
    assert out.tolist() == want.tolist()
