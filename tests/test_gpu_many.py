"""GPU parity of the many-queries pass (csrc/overlap_many.hip; SketchSet.overlaps_many / search_many / prefetch_many and the
LinearIndex methods on top): against dense numpy counts, the oracle's downsampled sketches, and the loops of the one-query methods,
at the smallest shapes at which the pass can go wrong.  Run with -m gpu."""
import ctypes as C
import glob

import numpy as np
import pytest

import many_cases as mc
import oracle
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 8
MARK = 0x5a5a5a5a


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    assert sourmash_amd.gpu_available()
    return sourmash_amd


@pytest.fixture(scope="module")
def geometry(sm):
    from sourmash_amd._lowlevel import lib
    wg, qb, qmax = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib.smgpu_many_geometry(C.byref(wg), C.byref(qb), C.byref(qmax))
    return wg.value, qb.value, qmax.value


def sketchset(sm, rows, scaled=1000, ksize=21, **kw):
    mhs = []
    for r in rows:
        mh = sm.MinHash(0, ksize, scaled=scaled, **kw)
        mh.add_many([int(h) for h in r])
        assert len(mh) == len(r)
        mhs.append(mh)
    return sm.SketchSet(mhs), mhs


def dense_of(db, qs, need=1):
    q, r, c = db.overlaps_many(qs, need)
    assert q.dtype == r.dtype == c.dtype == np.uint32
    key = q.astype(np.uint64) << np.uint64(32) | r
    assert np.array_equal(key, np.unique(key))                          # ordered by (query, row), no pair twice
    return mc.scatter(len(qs), len(db), q, r, c)


# ---- the raw entry on torch tensors -------------------------------------------------------------------------------------------------
def raw_run(queries, rows, need=1, cutoff=mc.U64_MAX, q_block=0, grid=0, capacity=None):
    "-> (returned, result[4], queries, rows, common, guards untouched) of smgpu_many_overlap_raw"
    import torch
    from sourmash_amd._lowlevel import lib

    def dev(a, dtype):
        a = np.concatenate([np.ascontiguousarray(a, dtype=dtype), np.zeros(4, dtype=dtype)])
        return torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).cuda()
    qh, qoff = mc.csr(queries)
    h, off = mc.csr(rows)
    m, n = len(queries), len(rows)
    d_qh, d_qoff, d_h, d_off = dev(qh, np.uint64), dev(qoff, np.uint64), dev(h, np.uint64), dev(off, np.uint64)
    d_need = dev(np.broadcast_to(np.asarray(need, dtype=np.uint32), (m,)), np.uint32)
    cap = m * n if capacity is None else capacity
    outs = [torch.full((cap + GUARD,), MARK, dtype=torch.int32, device="cuda") for _ in range(3)]
    result = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    ws_bytes = int(lib.smgpu_many_overlap_workspace_bytes(m, len(qh), cap))
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    tail = torch.full((64,), 0x5a, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = tail
    torch.cuda.synchronize()
    lib.sourmash_err_clear()
    got = lib.smgpu_many_overlap_raw(d_qh.data_ptr(), d_qoff.data_ptr(), m, len(qh), d_h.data_ptr(), d_off.data_ptr(), n, d_need.data_ptr(),
                                     cutoff, q_block, grid, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), cap, result.data_ptr(),
                                     ws.data_ptr(), ws_bytes, None)
    assert lib.sourmash_err_get_last_code() == 0
    torch.cuda.synchronize()
    res = result.cpu().numpy().view(np.uint64)
    assert got == res[0]
    host = [o.cpu().numpy().view(np.uint32) for o in outs]
    guards_ok = all((o[cap:] == MARK).all() for o in host) and bool((ws[ws_bytes:] == tail).all())
    k = min(int(got), cap)
    return int(got), res, host[0][:k], host[1][:k], host[2][:k], guards_ok


def check_raw(queries, rows, counts, **kw):
    got, res, q, r, c, guards_ok = raw_run(queries, rows, **kw)
    assert guards_ok
    want = mc.expected_hits(counts, kw.get("need", 1))
    assert got == len(want[0])
    assert [a.tolist() for a in (q, r, c)] == [a.tolist() for a in want]
    return res


# 1 ---- m = 1 ---------------------------------------------------------------------------------------------------------------------
def test_one_query_equals_overlaps(sm):
    queries, rows = mc.random_case(m=6, n=70)
    rows[3] = queries[2].copy()
    db, _ = sketchset(sm, rows)
    for q in queries[:4] + [mc.u64([]), rows[5][:1]]:
        qs, mhs = sketchset(sm, [q])
        want = db.overlaps(mhs[0])
        assert np.array_equal(dense_of(db, qs)[0], want.astype(np.int64))
        assert np.array_equal(want.astype(np.int64), mc.dense_counts([q], rows)[0])


# 2 ---- written by hand -------------------------------------------------------------------------------------------------------------
def test_hand_case(sm):
    queries, rows, cutoff = mc.hand_case()
    counts = mc.dense_counts(queries, rows, cutoff)
    db, db_mhs = sketchset(sm, rows)
    qs, q_mhs = sketchset(sm, queries)
    assert np.array_equal(dense_of(db, qs), counts)
    for q, a in enumerate(queries):                                     # the oracle agrees with the numpy matrix
        for r, b in enumerate(rows):
            oa, ob = oracle.OracleMinHash(0, 21, scaled=1000), oracle.OracleMinHash(0, 21, scaled=1000)
            oa.add_many([int(v) for v in a])
            ob.add_many([int(v) for v in b])
            assert oa.count_common(ob, downsample=True) == counts[q, r]
    check_raw(queries, rows, counts, cutoff=cutoff)


def test_largest_u64_values(sm):
    queries, rows, cutoff = mc.largest_values_case()
    counts = mc.dense_counts(queries, rows)
    db, _ = sketchset(sm, rows, scaled=1)
    qs, _ = sketchset(sm, queries, scaled=1)
    assert np.array_equal(dense_of(db, qs), counts)
    check_raw(queries, rows, counts)
    check_raw(queries[:1], rows, counts[:1])                            # one distinct query hash, with the top bit set


# 3 ---- row lengths around the lane, wave and workgroup sizes --------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2, 0, 16])
def test_row_lengths(sm, geometry, grid):
    block = geometry[0]
    queries, rows, lengths = mc.row_length_case(block)
    assert lengths == [0, 1, 63, 64, 65, block - 1, block, block + 1, 4 * block + 1] and [len(r) for r in rows] == lengths
    counts = mc.dense_counts(queries, rows)
    assert np.array_equal(counts[1], lengths)                           # query 1 is the whole pool
    res = check_raw(queries, rows, counts, grid=grid)                   # 9 rows: more than 1 or 2 workgroups, as many as the default, fewer than 16
    assert res[2] == 1
    check_raw(queries, rows, counts, grid=grid, need=[60, 64, 1])


# 4 ---- query blocks ----------------------------------------------------------------------------------------------------------------
def test_query_blocks_of_four(sm):
    queries, rows = mc.block_edge_case()
    counts = mc.dense_counts(queries, rows)
    one = raw_run(queries, rows)
    four = raw_run(queries, rows, q_block=4)
    assert one[1][2] == 1 and four[1][2] == 3                           # passes: blocks of 4, 4, 1
    assert one[0] == four[0] == np.count_nonzero(counts)
    assert [a.tolist() for a in one[2:5]] == [a.tolist() for a in four[2:5]]
    assert np.array_equal(mc.scatter(9, len(rows), *four[2:5]), counts)
    for grid in (1, 2):
        check_raw(queries, rows, counts, q_block=4, grid=grid, need=np.arange(1, 10) % 3 + 1)
    check_raw(queries, rows, counts, q_block=1)


# 5 ---- capacity --------------------------------------------------------------------------------------------------------------------
def test_raw_capacity_too_small(sm):
    queries, rows = mc.block_edge_case()
    counts = mc.dense_counts(queries, rows)
    want = mc.expected_hits(counts, 1)
    hits = len(want[0])
    valid = set(zip(*(a.tolist() for a in want)))
    for cap in (0, 1, hits - 1):
        for q_block in (0, 4):
            got, res, q, r, c, guards_ok = raw_run(queries, rows, capacity=cap, q_block=q_block)
            assert got == hits and res[0] == hits                       # the cursor reports the true count
            assert guards_ok                                            # and nothing lies beyond the capacity
            found = list(zip(q.tolist(), r.tolist(), c.tolist()))
            assert len(found) == cap and len(set(found)) == cap and set(found) <= valid
    got, res, q, r, c, guards_ok = raw_run(queries, rows, capacity=hits)
    assert got == hits and guards_ok and [a.tolist() for a in (q, r, c)] == [a.tolist() for a in want]


def test_public_call_runs_again_when_the_first_capacity_is_too_small(sm):
    from sourmash_amd._lowlevel import lib
    queries, rows = mc.random_case(m=7, n=40)
    counts = mc.dense_counts(queries, rows)
    db, _ = sketchset(sm, rows)
    qs, _ = sketchset(sm, queries)
    assert db._many_hits(qs, 1).stats["reruns"] == 0
    lib.smgpu_many_set_first_capacity(3)
    try:
        hits = db._many_hits(qs, 1)
    finally:
        lib.smgpu_many_set_first_capacity(0)
    assert hits.stats["reruns"] == 1 and len(hits) == np.count_nonzero(counts) > 3
    assert np.array_equal(mc.scatter(len(queries), len(rows), hits.queries, hits.rows, hits.common), counts)


# 6 ---- need ------------------------------------------------------------------------------------------------------------------------
def test_need_per_query(sm):
    queries, rows, cutoff = mc.hand_case()
    counts = mc.dense_counts(queries, rows, cutoff)
    db, _ = sketchset(sm, rows)
    qs, _ = sketchset(sm, queries)
    c02 = int(counts[0, 2])
    assert c02 >= 2
    for need0, present in ((1, True), (c02, True), (c02 + 1, False)):
        need = [need0, 1, 1]
        got = dense_of(db, qs, need)
        want = mc.scatter(3, 5, *mc.expected_hits(counts, need))
        assert np.array_equal(got, want) and (got[0, 2] == c02) == present
        check_raw(queries, rows, counts, cutoff=cutoff, need=need)
    with pytest.raises(ValueError):
        db.overlaps_many(qs, 0)
    with pytest.raises(ValueError):
        db.overlaps_many(qs, [1, 0, 1])
    with pytest.raises(ValueError):
        db.overlaps_many(qs, [1, 1])


# 7 ---- different scaled ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled_q,scaled_db", [(1000, 2000), (2000, 1000)])
def test_coarser_scaled(sm, scaled_q, scaled_db):
    from sourmash_amd.minhash import _get_max_hash_for_scaled
    queries, rows, cutoff = mc.hand_case(_get_max_hash_for_scaled(scaled_q), _get_max_hash_for_scaled(scaled_db))
    assert cutoff == mc.MAX_HASH_2000
    db, _ = sketchset(sm, rows, scaled=scaled_db)
    qs, _ = sketchset(sm, queries, scaled=scaled_q)
    hits = db._many_hits(qs, 1)
    assert hits.scaled == 2000

    def down(hashes, scaled):
        mh = oracle.OracleMinHash(0, 21, scaled=scaled)
        mh.add_many([int(v) for v in hashes])
        assert len(mh) == len(hashes)
        return mh.downsample_scaled(2000) if scaled != 2000 else mh
    oq, orows = [down(a, scaled_q) for a in queries], [down(b, scaled_db) for b in rows]
    want = np.array([[a.count_common(b, downsample=True) for b in orows] for a in oq])
    assert np.array_equal(want, mc.dense_counts(queries, rows, cutoff))
    assert np.array_equal(mc.scatter(3, 5, hits.queries, hits.rows, hits.common), want)
    assert hits.query_sizes.tolist() == [len(a) for a in oq] and hits.row_sizes.tolist() == [len(b) for b in orows]
    finer = queries if scaled_q == 1000 else rows
    assert sum(len(a) for a in finer) > sum(len(a) for a in (oq if scaled_q == 1000 else orows))      # the cutoff did drop hashes
    check_raw(queries, rows, want, cutoff=cutoff)
    assert db._sizes_at(2000).tolist() == hits.row_sizes.tolist() and qs._sizes_at(2000).tolist() == hits.query_sizes.tolist()


# 8 ---- random, m = 40 x n = 300 ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_sets(sm):
    queries, rows = mc.random_case()
    assert len(queries) == 40 and len(rows) == 300 and len(rows[17]) == 0 and len(rows[203]) == 1
    db, _ = sketchset(sm, rows)
    qs, q_mhs = sketchset(sm, queries)
    return queries, rows, mc.dense_counts(queries, rows), db, qs, q_mhs


def test_random_dense_matrix_and_determinism(sm, random_sets):
    queries, rows, counts, db, qs, _ = random_sets
    assert np.count_nonzero(counts) > 0.9 * counts.size * (298 / 300)  # most pairs share something
    first = db.overlaps_many(qs)
    assert np.array_equal(mc.scatter(40, 300, *first), counts)
    second = db.overlaps_many(qs)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    check_raw(queries, rows, counts, q_block=16, grid=7)
    assert np.array_equal(dense_of(db, qs, 40), np.where(counts >= 40, counts, 0))


@pytest.mark.parametrize("mode", ["jaccard", "containment", "max_containment"])
def test_random_search_many_equals_search(sm, random_sets, mode):
    _, _, counts, db, qs, q_mhs = random_sets
    kw = dict(do_containment=mode == "containment", do_max_containment=mode == "max_containment")
    n_hits = 0
    for threshold, best_only in ((0.0, False), (0.05, False), (0.5, False), (0.05, True)):
        got = db.search_many(qs, threshold=threshold, best_only=best_only, **kw)
        assert len(got) == 40
        for q, mh in enumerate(q_mhs):
            want = db.search(mh, threshold=threshold, best_only=best_only, **kw)
            assert got[q] == want, (mode, threshold, best_only, q)
            n_hits += len(want)
    assert got[3] and got[3][0] == (1.0, 40)                            # the planted identical pair
    assert n_hits > 40


def test_random_prefetch_many_equals_prefetch(sm, random_sets):
    _, _, counts, db, qs, q_mhs = random_sets
    for threshold_bp in (0, 50_000):
        got = db.prefetch_many(qs, threshold_bp)
        want = [db.prefetch(mh, threshold_bp) for mh in q_mhs]
        assert got == want
        assert sum(len(w) for w in want) == np.count_nonzero(counts >= max(1, threshold_bp / 1000))
    assert 0 < sum(len(w) for w in want) < np.count_nonzero(counts)    # 50 hashes in common: some pairs pass, some do not


# 9 ---- LinearIndex -------------------------------------------------------------------------------------------------------------------
def test_linear_index_many_equals_the_loops(sm):
    from sourmash_amd.index import LinearIndex
    sigs = [sm.load_one_signature_from_json(f, ksize=21) for f in sorted(glob.glob(golden("gather", "GCF_*.sig")))]
    assert len(sigs) == 12
    db = LinearIndex(sigs)
    queries = [sigs[0], sigs[7]]

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.score == w.score and g.signature is w.signature and g.location == w.location
    for kw in (dict(threshold=0.0), dict(threshold=0.1), dict(threshold=0.0, do_containment=True), dict(threshold=0.0, do_max_containment=True),
               dict(threshold=0.0, best_only=True)):
        got = db.search_many(queries, **kw)
        assert len(got) == 2
        for q, g in zip(queries, got):
            want = db.search(q, **kw)
            same(g, want)
            assert want and want[0].signature is q
    for threshold_bp in (0, 100_000):
        got = db.prefetch_many(queries, threshold_bp)
        for q, g in zip(queries, got):
            same(g, list(db.prefetch(q, threshold_bp)))
    packed = db._packed
    db.search_many(queries, threshold=0.0)
    assert db._packed is packed                                         # the cached device CSR served again
    with pytest.raises(TypeError):
        db.search_many(queries)


# 10 ---- mismatches -------------------------------------------------------------------------------------------------------------------
def test_mismatches_raise_what_the_one_query_path_raises(sm):
    _, rows, _ = mc.hand_case()
    db, db_mhs = sketchset(sm, rows)
    for kw in (dict(ksize=31), dict(ksize=7, is_protein=True), dict(seed=43)):
        qs, q_mhs = sketchset(sm, [mc.u64([5, 7])], **{"ksize": 21, **kw})
        with pytest.raises(ValueError) as one:
            q_mhs[0].count_common(db_mhs[0])
        for call in (lambda: db.overlaps_many(qs), lambda: db.search_many(qs), lambda: db.prefetch_many(qs)):
            with pytest.raises(ValueError) as many:
                call()
            assert str(many.value) == str(one.value), kw
    num = sm.MinHash(500, 21)
    num.add_many([5, 7])
    nums = sm.SketchSet([num])
    for many, one in ((lambda: db.prefetch_many(nums), lambda: db.prefetch(num)),
                      (lambda: db.search_many(nums, do_containment=True), lambda: db.search(num, do_containment=True)),
                      (lambda: db.search_many(nums, do_containment=True, do_max_containment=True),
                       lambda: db.search(num, do_containment=True, do_max_containment=True))):
        with pytest.raises((ValueError, TypeError)) as e_one:
            one()
        with pytest.raises(type(e_one.value)) as e_many:
            many()
        assert str(e_many.value) == str(e_one.value)
    with pytest.raises(ValueError, match="scaled"):
        db.overlaps_many(nums)
    with pytest.raises(ValueError, match="scaled"):
        nums.overlaps_many(db)
    with pytest.raises(TypeError):
        db.overlaps_many([num])
