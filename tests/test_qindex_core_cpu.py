"""CPU checks of the query index (csrc/qindex_core.hpp: the lookup of a u64 in a sorted query through a first-level table) compiled for
the host (tests/native/qindex_emul.cpp): its geometry against the invariants its callers' allocations assume, its table and records
against numpy, and both lookup forms against np.searchsorted over the query families of tests/qindex_cases.py.  None of this needs a
GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import qindex_cases as qc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return qc.build_emul(tmp_path_factory.mktemp("qindex_core"))


@pytest.fixture(scope="module")
def emul_old(tmp_path_factory):
    return qc.build_emul(tmp_path_factory.mktemp("qindex_core_old"), old_geometry=True)


@pytest.fixture(scope="module")
def cases():
    return qc.all_cases()                     # (the generators assert their own coverage: bucket fills 0 .. 9, 16, 300)


# ---- geometry alone ------------------------------------------------------------------------------------------------------------------
def geometry_many(so, nq, q_max):
    nq, q_max = np.ascontiguousarray(nq, dtype=np.uint64), np.ascontiguousarray(q_max, dtype=np.uint64)
    shift, buckets = np.zeros(len(nq), dtype=np.uint32), np.zeros(len(nq), dtype=np.uint32)
    so.emul_qindex_geometry_many(nq.ctypes.data, q_max.ctypes.data, len(nq), shift.ctypes.data, buckets.ctypes.data)
    return shift, buckets


def sweep_inputs():
    "nq in 1 .. 5,000 x every bit length of q_max x {all ones, top bit only, top bit plus a third}, where q_max >= nq - 1"
    q_max = [0]
    for bits in range(1, 65):
        top = 2**(bits - 1)
        q_max += [2**bits - 1, top, top + top // 3]
    q_max = np.array(sorted(set(q_max)), dtype=np.uint64)
    nq = np.arange(1, 5001, dtype=np.uint64)
    a, b = np.meshgrid(nq, q_max, indexing="ij")
    a, b = a.ravel(), b.ravel()
    keep = b >= a - np.uint64(1)
    return a[keep], b[keep]


def violations(nq, q_max, shift, buckets):
    "indices at which an invariant of the geometry is broken (numpy, in 64 bits)"
    bad = shift > 63
    s = np.minimum(shift, 63).astype(np.uint64)
    exact = (q_max >> s) + np.uint64(1)                # no wrap: q_max >> s == 2^64 - 1 needs s == 0, which a test below pins apart
    bad |= buckets.astype(np.uint64) != exact
    bad |= buckets.astype(np.uint64) > np.uint64(2) * nq + np.uint64(1)
    bad |= (nq <= np.uint64(2**26)) & (shift > 0) & (buckets.astype(np.uint64) < nq)
    return np.nonzero(bad)[0]


def test_geometry_invariants_sweep(emul):
    nq, q_max = sweep_inputs()
    assert len(nq) > 750_000 and int(nq.max()) == 5000 and int(q_max.max()) == qc.U64_MAX
    shift, buckets = geometry_many(emul, nq, q_max)
    assert not ((shift == 0) & (q_max == np.uint64(qc.U64_MAX))).any()
    bad = violations(nq, q_max, shift, buckets)
    assert len(bad) == 0, [(int(nq[i]), hex(int(q_max[i])), int(shift[i]), int(buckets[i])) for i in bad[:5]]
    # ... and it is the geometry restated in Python integers, at a sample the integer arithmetic gets through quickly
    for i in range(0, len(nq), 97):
        assert (int(shift[i]), int(buckets[i])) == qc.geometry(int(nq[i]), int(q_max[i])), (int(nq[i]), hex(int(q_max[i])))


@pytest.mark.parametrize("nq", [2**26 - 1, 2**26, 2**26 + 1, 2**27, 2**32 - 2])
def test_geometry_invariants_at_the_cap(emul, nq):
    "the 26-bit cap on the table, and the halved shift on both sides of it"
    for q_max in (nq - 1, 2**40, 2**64 - 1):
        shift, buckets = qc.emul_geometry(emul, nq, q_max)
        assert qc.geometry_violations(nq, q_max, shift, buckets) == [], (nq, hex(q_max), shift, buckets)
        assert (shift, buckets) == qc.geometry(nq, q_max)
        assert buckets <= 2**27                                     # the cap: a table never has more entries than this


def test_geometry_of_one_hash(emul):
    "family A: one bucket below 2^63, two from there on, never a shift by the operand's width"
    for v in qc.family_a_values():
        shift, buckets = qc.emul_geometry(emul, 1, v)
        assert qc.geometry_violations(1, v, shift, buckets) == [], hex(v)
        assert (shift, buckets) == (min(v.bit_length(), 63), 2 if v >= 2**63 else 1), hex(v)


def test_the_cases_catch_the_geometry_without_the_shift_bound(emul_old):
    """Teeth: with the geometry as it was before the shift was bounded (a copy inside the emulation, -DQINDEX_EMUL_OLD_GEOMETRY),
    family A breaks shift <= 63 -- one hash at or above 2^63 -- with the bucket counts that go with a shift by 0, and the lookup
    refuses to build a table on it."""
    broken = {}
    for v in qc.family_a_values():
        shift, buckets = qc.emul_geometry(emul_old, 1, v)
        bad = qc.geometry_violations(1, v, shift, buckets)
        if bad:
            broken[v] = (shift, buckets, bad)
    assert sorted(broken) == [2**63, qc.ALT]
    assert broken[2**63][:2] == (64, 1) and broken[qc.ALT][:2] == (64, 2_863_311_531)
    assert all(b[2] == ["shift <= 63"] for b in broken.values())
    assert qc.emul_geometry(emul_old, 1, qc.U64_MAX) == (63, 2)          # (rescued by a wrapped 32-bit count, not by design)
    q = qc.u64([qc.ALT])
    assert qc.emul_find(emul_old, q, qc.probes_for(q), 0)[1] == -1


# ---- table and records ---------------------------------------------------------------------------------------------------------------
def test_table_and_records_against_numpy(emul, cases):
    for name, q in cases:
        shift, buckets = qc.emul_geometry(emul, len(q), int(q[-1]))
        assert (shift, buckets) == qc.geometry(len(q), int(q[-1])), name
        assert qc.geometry_violations(len(q), int(q[-1]), shift, buckets) == [], name
        qp = qc.padded(q)
        T = np.full(buckets + 1 + 2, 0xDEADBEEF, dtype=np.uint32)        # two guard entries behind T[buckets]
        rec = np.zeros(4 * buckets, dtype=np.uint64)
        emul.emul_qindex_build(qp.ctypes.data, len(q), shift, buckets, T.ctypes.data, rec.ctypes.data)
        assert (T[buckets + 1:] == 0xDEADBEEF).all(), name
        edges = np.arange(buckets, dtype=np.uint64) << np.uint64(shift)
        want_T = np.concatenate([np.searchsorted(q, edges, side="left"), [len(q)]]).astype(np.uint32)
        assert np.array_equal(T[:buckets + 1], want_T), name
        assert T[0] == 0 and (np.diff(want_T.astype(np.int64)) >= 0).all()
        rec = rec.reshape(buckets, 4)
        pos, cnt = (rec[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.int64), (rec[:, 0] >> np.uint64(32)).astype(np.int64)
        assert np.array_equal(pos, want_T[:-1]) and np.array_equal(cnt, np.diff(want_T.astype(np.int64))), name
        for i in range(3):                                               # the first three hashes inline, zero where the bucket is shorter
            want_h = np.where(cnt > i, qp[np.minimum(pos + i, len(q) - 1)], 0)
            assert np.array_equal(rec[:, 1 + i], want_h.astype(np.uint64)), (name, i)


# ---- lookups -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(qc.FORMS))
def test_lookups_are_searchsorted(emul, cases, form):
    """Every family, every probe: the position np.searchsorted gives on the unpadded query, or NONE32, and no read outside the
    query's nq + 4 entries, the table's buckets + 1 or the bucket records.  The split form runs its match on probes above q_max with
    the record of q_max's bucket, as the index builder does, and discards the answer: those reads stay inside as well."""
    n_probes = 0
    for name, q in cases:
        probes = qc.probes_for(q)
        got, out_of_bounds = qc.emul_find(emul, q, probes, qc.FORMS[form])
        assert out_of_bounds == 0, (name, out_of_bounds)
        want = qc.expected_positions(q, probes)
        wrong = np.nonzero(got != want)[0]
        assert len(wrong) == 0, (name, [(hex(int(probes[i])), int(got[i]), int(want[i])) for i in wrong[:5]])
        assert (want != qc.NONE32).sum() >= len(q) and (want == qc.NONE32).any(), name
        n_probes += len(probes)
    assert n_probes > 500_000


def test_probe_sets_hold_what_they_promise(cases):
    for name, q in cases:
        probes = set(qc.probes_for(q).tolist())
        shift, buckets = qc.geometry(len(q), int(q[-1]))
        assert set(q.tolist()) <= probes and {0, 1, int(q[-1]), 2**63 - 1, 2**63, qc.U64_MAX} <= probes, name
        assert (int(q[-1]) + 1 in probes) == (int(q[-1]) < qc.U64_MAX), name
        assert ((buckets - 1) << shift) in probes and (buckets == 1 or ((buckets - 1) << shift) - 1 in probes), name


def test_families_hold_the_shapes_the_lookups_branch_on(cases):
    "what the generators promise, seen from the outside: shift 0, the largest shift, empty first and last buckets' neighbours, hash 0"
    by_name = dict(cases)
    shifts = {name: qc.geometry(len(q), int(q[-1]))[0] for name, q in cases}
    assert shifts["C-256-0"] == 0 and shifts["C-4096-0"] == 0 and shifts["A-0x0"] == 0
    assert shifts["A-0x8000000000000000"] == 63 and shifts["A-0xffffffffffffffff"] == 63
    assert shifts["G-dense"] >= 59                                       # ten hashes in one bucket of sixteen
    counts, _, buckets = qc.bucket_counts(by_name["G-dense"])
    assert counts.max() == 10 and (counts == 0).sum() == buckets - 1
    counts, _, buckets = qc.bucket_counts(by_name["B-ends"])            # 0 and 2^64 - 1: the first and the last bucket, nothing between
    assert counts[0] == 1 and counts[buckets - 1] == 1 and counts.sum() == 2
    counts, _, buckets = qc.bucket_counts(by_name["C-257-top"])         # a dense run at the top of the hash space: bucket 0 is empty
    assert counts[0] == 0 and counts[buckets - 1] > 0
    e54 = by_name["E-1000-54"]
    assert int(e54[-1]) <= qc.MAX_HASH_1000 and int(e54[-1]) > qc.MAX_HASH_1000 // 2
    assert len(by_name["E-8193-64"]) == 8193 and int(by_name["E-8193-64"][-1]) >= 2**63
    for name, q in cases:
        assert q.dtype == np.uint64 and len(q) >= 1 and (q[1:] > q[:-1]).all(), name


def test_emulation_under_sanitizers_as_a_program_of_its_own(tmp_path):
    "the header's own arithmetic with -fsanitize=address,undefined: no shift by the operand's width, no fill or lookup past a vector's end"
    import subprocess
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + probe.stderr.strip().splitlines()[-1])
    exe = str(tmp_path / "qindex_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DQINDEX_EMUL_MAIN", "-o", exe, os.path.join(HERE, "native", "qindex_emul.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok: ") and " 89 queries" in out.stdout, out.stdout + out.stderr


def test_debug_entry_is_declared_and_exported():
    from sourmash_amd._lowlevel import lib
    proto = ("void smgpu_debug_qindex_find(const uint64_t *d_query, uint64_t nq, const uint64_t *d_probes, uint64_t n, int32_t form, "
             "uint32_t *d_pos_out, void *stream);")
    with open(os.path.join(ROOT, "include", "sourmash_amd.h")) as f:
        header = " ".join(f.read().split())
    assert " ".join(proto.split()) in header
    assert hasattr(C.CDLL(os.path.join(ROOT, "sourmash_amd", "libsourmash_amd.so")), "smgpu_debug_qindex_find")
    assert "smgpu_debug_qindex_find" in lib.functions
