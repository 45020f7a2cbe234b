"""CPU checks of the many-queries pass (csrc/overlap_many.hip): its rules (csrc/many_core.hpp) compiled for the host against numpy and
the oracle, the C interface, and the entry points without a device.  None of this needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import many_cases as mc
import oracle
import sourmash_amd
from sourmash_amd._lowlevel import lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "native", "many_core_emul.cpp")

PROTOTYPES = [
    "void smgpu_many_geometry(uint32_t *workgroup, uint32_t *q_block, uint32_t *q_block_max);",
    "void smgpu_many_need(uint32_t mode, double threshold, const uint64_t *sizes, uint64_t m, uint32_t *need_out);",
    "uint64_t smgpu_many_overlap_workspace_bytes(uint64_t m, uint64_t q_total, uint64_t capacity);",
    "uint64_t smgpu_many_overlap_raw(const uint64_t *d_qhashes, const uint64_t *d_qoffsets, uint64_t m, uint64_t q_total, "
    "const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n_rows, const uint32_t *d_need, uint64_t cutoff, uint32_t q_block, "
    "uint32_t grid, uint32_t *d_queries, uint32_t *d_rows, uint32_t *d_common, uint64_t capacity, uint64_t *d_result, "
    "void *d_workspace, uint64_t workspace_bytes, void *stream);",
    "void smgpu_many_sizes_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n, uint64_t cutoff, uint64_t *d_sizes, void *stream);",
    "void smgpu_sketchset_sizes_at(const SmgpuSketchSet *set, uint64_t max_hash, uint64_t *sizes_out);",
    "SmgpuManyHits *smgpu_sketchset_overlaps_many(const SmgpuSketchSet *db, const SmgpuSketchSet *queries, const uint32_t *need, "
    "uint32_t need_all);",
    "void smgpu_manyhits_free(SmgpuManyHits *ptr);",
    "uint64_t smgpu_manyhits_len(const SmgpuManyHits *ptr);",
    "const uint32_t *smgpu_manyhits_queries(const SmgpuManyHits *ptr);",
    "const uint32_t *smgpu_manyhits_rows(const SmgpuManyHits *ptr);",
    "const uint32_t *smgpu_manyhits_common(const SmgpuManyHits *ptr);",
    "const uint64_t *smgpu_manyhits_query_sizes(const SmgpuManyHits *ptr);",
    "const uint64_t *smgpu_manyhits_row_sizes(const SmgpuManyHits *ptr);",
    "uint64_t smgpu_manyhits_scaled(const SmgpuManyHits *ptr);",
    "void smgpu_manyhits_stats(const SmgpuManyHits *ptr, double *out6);",
    "void smgpu_many_set_first_capacity(uint64_t capacity);",
]


def _norm(s):
    return " ".join(s.replace("( ", "(").replace(" )", ")").split())


def test_prototypes_declared_and_exported():
    with open(os.path.join(ROOT, "include", "sourmash_amd.h")) as f:
        header = _norm(f.read())
    so = C.CDLL(os.path.join(ROOT, "sourmash_amd", "libsourmash_amd.so"))
    assert len(PROTOTYPES) == 17
    for p in PROTOTYPES:
        assert _norm(p) in header, p
        name = p.split("(")[0].split()[-1].lstrip("*")
        assert hasattr(so, name), name
        assert name in lib.functions, name                     # the binding parsed it
    # the Python layer the exports carry
    for name in ("overlaps_many", "prefetch_many", "search_many"):
        assert callable(getattr(sourmash_amd.SketchSet, name))
    from sourmash_amd.index import LinearIndex
    assert callable(LinearIndex.search_many) and callable(LinearIndex.prefetch_many)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("many_core") / "libmany_core_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so_path, SRC])
    so = C.CDLL(so_path)
    so.emul_many_cutoff.argtypes = [C.c_uint64, C.c_uint64]
    so.emul_many_cutoff.restype = C.c_uint64
    so.emul_many_cut_len.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    so.emul_many_cut_len.restype = C.c_uint64
    so.emul_many_post_range.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    so.emul_many_key.argtypes = [C.c_uint32, C.c_uint32]
    so.emul_many_key.restype = C.c_uint64
    so.emul_many_key_query.argtypes = so.emul_many_key_row.argtypes = [C.c_uint64]
    so.emul_many_key_query.restype = so.emul_many_key_row.restype = C.c_uint32
    so.emul_many_need.argtypes = [C.c_uint32, C.c_double, C.c_uint64]
    so.emul_many_need.restype = C.c_uint32
    so.emul_many_compat_code.argtypes = [C.c_void_p, C.c_void_p]
    so.emul_many_compat_code.restype = C.c_uint32
    so.emul_many_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                  C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    so.emul_many_pass.restype = C.c_uint64
    return so


def test_geometry_is_the_headers(emul):
    wg, qb, qmax = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib.smgpu_many_geometry(C.byref(wg), C.byref(qb), C.byref(qmax))
    assert (wg.value, qb.value, qmax.value) == (emul.emul_many_block(), emul.emul_many_q_block(), emul.emul_many_q_block_max())
    assert wg.value % 64 == 0
    # the default block's counters leave LDS for the eight workgroups of four waves a CU holds (160 KiB a CU), the largest fits one
    assert 8 * 4 * qb.value <= 160 * 1024 and 4 * qmax.value + 64 <= 160 * 1024


# ---- the posting range of a query block ---------------------------------------------------------------------------------------------
def post_range(emul, post, a, b, q_lo, q_hi):
    ab = np.array([a, b], dtype=np.uint32)
    emul.emul_many_post_range(post.ctypes.data, ab.ctypes.data, q_lo, q_hi)
    return int(ab[0]), int(ab[1])


def test_post_range_against_numpy(emul):
    rng = np.random.default_rng(1)
    lists = [np.arange(9, dtype=np.uint32), np.array([2, 3, 4, 5, 6, 7, 8], dtype=np.uint32), np.array([3, 4], dtype=np.uint32),
             np.array([0], dtype=np.uint32), np.array([8], dtype=np.uint32)]
    lists += [np.unique(rng.integers(0, 40, size=k)).astype(np.uint32) for k in (1, 2, 5, 17, 40)]
    for lst in lists:
        # the list inside a longer array: the range must never leave [a, b)
        post = np.concatenate([np.array([0, 1000], dtype=np.uint32), lst, np.array([0, 1000], dtype=np.uint32)])
        a, b = 2, 2 + len(lst)
        top = int(lst.max()) + 2
        for q_block in (1, 4, 7, top):
            seen = []
            for q_lo in range(0, top, q_block):
                lo, hi = post_range(emul, post, a, b, q_lo, q_lo + q_block)
                assert a <= lo <= hi <= b
                want = lst[(lst >= q_lo) & (lst < q_lo + q_block)]
                assert np.array_equal(post[lo:hi], want), (lst, q_lo, q_block)
                seen.append(post[lo:hi])
            assert np.array_equal(np.concatenate(seen), lst)           # every posting belongs to exactly one block
        assert post_range(emul, post, a, a, 0, 100) == (a, a)          # an empty list stays empty


# ---- the cutoff ------------------------------------------------------------------------------------------------------------------
def test_cutoff_rule(emul):
    assert emul.emul_many_cutoff(mc.MAX_HASH_1000, mc.MAX_HASH_2000) == mc.MAX_HASH_2000 == emul.emul_many_cutoff(mc.MAX_HASH_2000, mc.MAX_HASH_1000)
    assert emul.emul_many_cutoff(mc.U64_MAX, mc.U64_MAX) == mc.U64_MAX
    rng = np.random.default_rng(2)
    rows = [mc.u64([]), mc.u64([5]), mc.u64([mc.U64_MAX]), mc.u64([1, mc.MAX_HASH_2000, mc.MAX_HASH_2000 + 1, mc.MAX_HASH_1000, mc.U64_MAX]),
            np.unique(rng.integers(1, mc.MAX_HASH_1000, size=1000, dtype=np.uint64))]
    for row in rows:
        cuts = [0, 1, 4, 5, 6, mc.MAX_HASH_2000 - 1, mc.MAX_HASH_2000, mc.MAX_HASH_2000 + 1, mc.MAX_HASH_1000, mc.U64_MAX - 1, mc.U64_MAX]
        cuts += [int(v) for v in row[:3]] + [int(v) - 1 for v in row[-3:]]
        for cutoff in cuts:
            got = emul.emul_many_cut_len(row.ctypes.data, len(row), cutoff)
            assert got == np.count_nonzero(row <= np.uint64(cutoff)), (len(row), cutoff)


def oracle_mh(hashes, scaled):
    mh = oracle.OracleMinHash(0, 21, scaled=scaled)
    mh.add_many([int(h) for h in hashes])
    return mh


def merged_index(queries, cutoff):
    "U, uoff, post of the queries at the cutoff, in numpy"
    pairs = sorted((int(h), q) for q, hs in enumerate(queries) for h in hs if int(h) <= cutoff)
    U = np.array(sorted({h for h, _ in pairs}), dtype=np.uint64)
    post = np.array([q for _, q in pairs], dtype=np.uint32)
    uoff = np.append(np.searchsorted(np.array([h for h, _ in pairs], dtype=np.uint64), U, side="left"), len(pairs)).astype(np.uint32)
    return U, uoff, post


def run_pass(emul, queries, rows, cutoff, need, q_block, capacity=None):
    U, uoff, post = merged_index(queries, cutoff)
    hashes, offsets = mc.csr(rows)
    offsets = offsets.astype(np.uint64)
    m = len(queries)
    need = np.ascontiguousarray(np.broadcast_to(np.asarray(need, dtype=np.uint32), (m,)))
    cap = m * len(rows) if capacity is None else capacity
    out = [np.full(cap + 2, 0xdeadbeef, dtype=np.uint32) for _ in range(3)]
    counters = np.zeros(max(q_block, 1), dtype=np.uint32)
    U_pad, post_pad, hashes_pad = (np.append(x, x.dtype.type(0)) for x in (U, post, hashes))
    hits = emul.emul_many_pass(U_pad.ctypes.data, uoff.ctypes.data, post_pad.ctypes.data, len(U), hashes_pad.ctypes.data, offsets.ctypes.data, len(rows),
                               cutoff, need.ctypes.data, m, q_block, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, cap, counters.ctypes.data)
    assert not counters.any()                                           # zero again behind every row
    assert all((o[cap:] == 0xdeadbeef).all() for o in out)              # nothing behind the capacity
    return hits, [o[:min(hits, cap)] for o in out]


@pytest.mark.parametrize("scaled_q,scaled_db", [(1000, 1000), (1000, 2000), (2000, 1000)])
def test_hand_case_against_numpy_and_oracle(emul, scaled_q, scaled_db):
    from sourmash_amd.minhash import _get_max_hash_for_scaled
    mq, mdb = _get_max_hash_for_scaled(scaled_q), _get_max_hash_for_scaled(scaled_db)
    assert {mq, mdb} <= {mc.MAX_HASH_1000, mc.MAX_HASH_2000}
    queries, rows, cutoff = mc.hand_case(mq, mdb)
    assert cutoff == emul.emul_many_cutoff(mq, mdb)
    counts = mc.dense_counts(queries, rows, cutoff)
    assert counts[0, 0] == mc.sizes_at(queries, cutoff)[0] == mc.sizes_at(rows, cutoff)[0]         # the identical pair
    assert (counts[1] == 0).all() and (counts[:, 3] == 0).all() and (counts[[0, 2]][:, [0, 1, 2, 4]] >= 1).all()
    # the oracle's count_common(downsample=True) says the same of every pair
    for q, a in enumerate(queries):
        for r, b in enumerate(rows):
            assert oracle_mh(a, scaled_q).count_common(oracle_mh(b, scaled_db), downsample=True) == counts[q, r], (q, r)
    for q_block in (1, 2, 3, 4096):
        hits, (hq, hr, hc) = run_pass(emul, queries, rows, cutoff, 1, q_block)
        assert hits == np.count_nonzero(counts)
        assert np.array_equal(mc.scatter(3, 5, hq, hr, hc), counts)


def test_largest_values_and_block_edges(emul):
    queries, rows, cutoff = mc.largest_values_case()
    counts = mc.dense_counts(queries, rows)
    assert counts[0, 0] == 1 and counts[2, 0] == 0 and counts[1, 1] == 2
    for a_q, a in enumerate(queries):
        for r, b in enumerate(rows):
            assert oracle_mh(a, 1).count_common(oracle_mh(b, 1), downsample=True) == counts[a_q, r]
    hits, (hq, hr, hc) = run_pass(emul, queries, rows, cutoff, 1, 2)
    assert np.array_equal(mc.scatter(3, 5, hq, hr, hc), counts)
    queries, rows = mc.block_edge_case()
    counts = mc.dense_counts(queries, rows)
    results = []
    for q_block in (4, 9, 4096):
        hits, (hq, hr, hc) = run_pass(emul, queries, rows, mc.U64_MAX, 1, q_block)
        assert np.array_equal(mc.scatter(9, len(rows), hq, hr, hc), counts), q_block
        order = np.argsort(hq.astype(np.uint64) << np.uint64(32) | hr, kind="stable")
        results.append((hq[order].tolist(), hr[order].tolist(), hc[order].tolist()))
    assert results[0] == results[1] == results[2]
    # need and capacity: the count says what was found, the arrays end at the capacity
    want = mc.expected_hits(counts, np.arange(1, 10) % 3 + 1)
    for cap in (0, 1, len(want[0]) - 1, len(want[0])):
        hits, (hq, hr, hc) = run_pass(emul, queries, rows, mc.U64_MAX, np.arange(1, 10) % 3 + 1, 4, capacity=cap)
        assert hits == len(want[0]) and len(hq) == min(cap, hits)


# ---- the (query, row) key ----------------------------------------------------------------------------------------------------------
def test_key_orders_by_query_then_row(emul):
    pairs = [(0, 0), (0, 1), (0, 2**32 - 2), (1, 0), (7, 5), (7, 6), (2**32 - 2, 0), (2**32 - 2, 2**32 - 2)]
    keys = [emul.emul_many_key(q, r) for q, r in pairs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert keys == [(q << 32) | r for q, r in pairs]
    assert [(emul.emul_many_key_query(k), emul.emul_many_key_row(k)) for k in keys] == pairs


# ---- the integer filter of a threshold -----------------------------------------------------------------------------------------------
THRESHOLDS = [0.0, 1e-9, 0.01, 0.05, 0.1, 0.2, 0.25, 0.3, 1 / 3, 0.4, 0.5, 0.6, 2 / 3, 0.7, 0.75, 0.8, 0.9, 0.95, 0.99, 1.0] + \
    [i / 64 for i in range(1, 64)] + [i / 7 for i in range(1, 7)]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_need_never_above_the_smallest_passing_count(emul, mode):
    """For every query size up to 64, every threshold of the grid, every row size and every common count the pair can have: a pair that
    passes the float test of the scoring (score >= threshold and score > 0) has a count of at least need."""
    from sourmash_amd.index import many_need, score_hits
    kw = dict(do_containment=mode == 1, do_max_containment=mode == 2)
    row_sizes = np.array(list(range(0, 130)) + [1000, 10**6], dtype=np.int64)
    for t in THRESHOLDS:
        needs = many_need(np.arange(65, dtype=np.uint64), t, **kw)
        for n_q in range(65):
            need = emul.emul_many_need(mode, t, n_q)
            assert need == needs[n_q] and need >= 1
            if n_q == 0:
                continue
            c = np.arange(1, n_q + 1, dtype=np.int64)[:, None] + 0 * row_sizes[None, :]
            sizes = row_sizes[None, :] + 0 * c
            score = score_hits(c, sizes, n_q, **kw)
            passing = ((score >= t) & (score > 0) & (sizes >= c)).any(axis=1)
            if passing.any():
                assert need <= 1 + int(np.argmax(passing)), (mode, t, n_q)          # the smallest count that passes for some row
    # the filter does filter: half of a 5,000-hash query's size at containment 0.5, a third at Jaccard 0.5
    assert emul.emul_many_need(1, 0.5, 5000) == 2499 and emul.emul_many_need(0, 0.5, 5000) == 1665 and emul.emul_many_need(2, 0.5, 5000) == 1
    for t in (-1.0, float("nan"), 0.0):
        assert emul.emul_many_need(0, t, 5000) == 1
    assert emul.emul_many_need(1, 1e30, 5000) == 2**32 - 1


# ---- compatibility -----------------------------------------------------------------------------------------------------------------
def test_compatibility_codes_in_the_references_order(emul):
    def code(a, b):
        a, b = np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64)
        return emul.emul_many_compat_code(a.ctypes.data, b.ctypes.data)
    ok = [31, 1, 42, mc.MAX_HASH_1000, 0]                               # ksize, hash function, seed, max_hash, num
    assert code(ok, ok) == 0
    assert code(ok, [31, 1, 42, mc.MAX_HASH_2000, 0]) == 0              # scaled may differ: the pair meets at the coarser one
    assert code(ok, [21, 2, 43, 0, 500]) == lib.SOURMASH_ERROR_CODE_MISMATCH_K_SIZES == 101
    assert code(ok, [31, 2, 43, 0, 500]) == lib.SOURMASH_ERROR_CODE_MISMATCH_DNA_PROT == 102
    assert code(ok, [31, 1, 43, 0, 500]) == lib.SOURMASH_ERROR_CODE_MISMATCH_SCALED == 103     # max_hash only when a side is num
    assert code(ok, [31, 1, 43, mc.MAX_HASH_2000, 0]) == lib.SOURMASH_ERROR_CODE_MISMATCH_SEED == 104
    num = [31, 1, 42, 0, 500]
    assert code(num, num) == lib.SOURMASH_ERROR_CODE_MISMATCH_NUM == 107                        # num sets are refused
    from sourmash_amd.exceptions import exceptions_by_code
    assert all(exceptions_by_code[c] is ValueError for c in (101, 102, 103, 104, 107))


# ---- without a device ----------------------------------------------------------------------------------------------------------------
def test_entry_points_raise_without_gpu():
    if sourmash_amd.gpu_available():
        pytest.skip("a GPU is present: the calls succeed (covered by tests/test_gpu_many.py)")
    from sourmash_amd import MinHash, SketchSet
    from sourmash_amd.exceptions import SourmashError
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    lib.sourmash_err_clear()
    ws = lib.smgpu_many_overlap_workspace_bytes(1, 1, 1)                 # (a size: no device needed)
    assert ws > 0 and lib.sourmash_err_get_last_code() == 0
    assert lib.smgpu_many_overlap_raw(p, p, 1, 1, p, p, 1, p, 2**64 - 1, 0, 0, p, p, p, 1, p, p, ws, None) == 2**64 - 1
    assert lib.sourmash_err_get_last_code() != 0
    from sourmash_amd._lowlevel import decode_str
    assert "no HIP device" in decode_str(lib.sourmash_err_get_last_message())
    lib.sourmash_err_clear()
    lib.smgpu_many_sizes_raw(p, p, 1, 5, p, None)
    assert lib.sourmash_err_get_last_code() != 0 and "no HIP device" in decode_str(lib.sourmash_err_get_last_message())
    lib.sourmash_err_clear()
    mh = MinHash(0, 21, scaled=1000)
    mh.add_many([5, 7])
    with pytest.raises(SourmashError, match="no HIP device"):            # the sets themselves live on the device
        SketchSet([mh]).overlaps_many(SketchSet([mh]))
    lib.sourmash_err_clear()


def test_raw_entry_refuses_bad_arguments_before_the_device():
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    for kwargs in (dict(q_block=2**20), dict(grid=2**21), dict(ws=16), dict(result=None)):
        lib.sourmash_err_clear()
        ws = kwargs.get("ws", lib.smgpu_many_overlap_workspace_bytes(1, 1, 1))
        got = lib.smgpu_many_overlap_raw(p, p, 1, 1, p, p, 1, p, 5, kwargs.get("q_block", 0), kwargs.get("grid", 0), p, p, p, 1,
                                         kwargs.get("result", p), p, ws, None)
        assert got == 2**64 - 1 and lib.sourmash_err_get_last_code() != 0, kwargs
        from sourmash_amd._lowlevel import decode_str
        assert "no HIP device" not in decode_str(lib.sourmash_err_get_last_message()), kwargs
    lib.sourmash_err_clear()
