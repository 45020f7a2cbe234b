"""GPU parity of the many-queries gather (csrc/gather_many.hip; SketchSet.gather_many and LinearIndex.gather_many on top): against
oracle.gather per query and the loop of the one-query gather, at the smallest shapes at which the kernels can go wrong.  Run with -m gpu."""
import ctypes as C
import glob

import numpy as np
import pytest

import gather_many_cases as gc
import many_cases as mc
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


def sketchset(sm, rows, scaled=1000, ksize=21, **kw):
    mhs = []
    for r in rows:
        mh = sm.MinHash(0, ksize, scaled=scaled, **kw)
        mh.add_many([int(h) for h in r])
        assert len(mh) == len(r)
        mhs.append(mh)
    return sm.SketchSet(mhs), mhs


# ---- the raw entry on torch tensors -------------------------------------------------------------------------------------------------
def raw_run(queries, rows, hits, cutoff=mc.U64_MAX, thr=0, max_query_hashes=0, max_candidates=0, grid=0):
    "-> (returned, out_rows, out_isect, rounds, status, guards untouched) of smgpu_gather_many_raw on the given hits"
    import torch
    from sourmash_amd._lowlevel import lib

    def dev(a, dtype):
        a = np.concatenate([np.ascontiguousarray(a, dtype=dtype), np.zeros(4, dtype=dtype)])
        return torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).cuda()
    qh, qoff = mc.csr(queries)
    h, off = mc.csr(rows)
    m, n, n_hits = len(queries), len(rows), len(hits[0])
    d_qh, d_qoff, d_h, d_off = dev(qh, np.uint64), dev(qoff, np.uint64), dev(h, np.uint64), dev(off, np.uint64)
    d_hq, d_hr, d_hc = (dev(a, np.uint32) for a in hits)
    outs = [torch.full((size + GUARD,), MARK, dtype=torch.int32, device="cuda") for size in (n_hits, n_hits, m, m)]
    ws_bytes = int(lib.smgpu_gather_many_workspace_bytes(m, n_hits, int(hits[2].sum())))
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    tail = torch.full((64,), 0x5a, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = tail
    torch.cuda.synchronize()
    lib.sourmash_err_clear()
    got = lib.smgpu_gather_many_raw(d_qh.data_ptr(), d_qoff.data_ptr(), m, d_h.data_ptr(), d_off.data_ptr(), n, d_hq.data_ptr(), d_hr.data_ptr(),
                                    d_hc.data_ptr(), n_hits, cutoff, thr, max_query_hashes, max_candidates, grid, outs[0].data_ptr(),
                                    outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), ws.data_ptr(), ws_bytes, None)
    code = lib.sourmash_err_get_last_code()
    torch.cuda.synchronize()
    host = [o.cpu().numpy().view(np.uint32) for o in outs]
    sizes = (n_hits, n_hits, m, m)
    guards_ok = all((o[s:] == MARK).all() for o, s in zip(host, sizes)) and bool((ws[ws_bytes:] == tail).all())
    return (int(got) if code == 0 else None), host[0][:n_hits], host[1][:n_hits], host[2][:m], host[3][:m], guards_ok


def check_raw(queries, rows, want, hits, **kw):
    got, out_rows, out_isect, rounds, status, guards_ok = raw_run(queries, rows, hits, **kw)
    assert guards_ok and not status.any()
    assert gc.picks_from_slots(hits, out_rows, out_isect, rounds, len(queries)) == want
    assert got == sum(len(w) for w in want)
    first = np.searchsorted(hits[0], np.arange(len(queries) + 1))
    for q in range(len(queries)):                                          # the slots behind a query's rounds are untouched
        assert (out_rows[first[q] + rounds[q]:first[q + 1]] == MARK).all() and (out_isect[first[q] + rounds[q]:first[q + 1]] == MARK).all()
    return out_rows, out_isect, rounds


# 1 ---- written by hand -------------------------------------------------------------------------------------------------------------
def test_hand_case(sm):
    db, _ = sketchset(sm, gc.HAND_ROWS)
    qs, q_mhs = sketchset(sm, gc.HAND_QUERIES)
    for threshold_bp, picks in sorted(gc.HAND_PICKS.items()):
        want = [[], picks, []]
        assert gc.oracle_picks(gc.HAND_QUERIES, gc.HAND_ROWS, threshold_bp) == want
        assert db.gather_many(qs, threshold_bp) == want, threshold_bp
        assert [db.gather(mh, threshold_bp) for mh in q_mhs] == want
        thr = gc.threshold_hashes(threshold_bp, 1000)
        check_raw(gc.HAND_QUERIES, gc.HAND_ROWS, want, gc.hits_of(gc.HAND_QUERIES, gc.HAND_ROWS, need=thr), thr=thr)
    res = db._many_gather(qs, 0)
    assert res.scaled == 1000 and res.offsets.tolist() == [0, 0, 4, 4]
    assert res.stats["way_out_queries"] == 0 and res.stats["batches"] == 1


# 2 ---- random, m = 40 x n = 300 ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_sets(sm):
    queries, rows = gc.random_case()
    db, _ = sketchset(sm, rows)
    qs, q_mhs = sketchset(sm, queries)
    return queries, rows, mc.dense_counts(queries, rows), db, qs, q_mhs


@pytest.mark.parametrize("threshold_bp", [0, 20_000, 60_000])
def test_random_case_equals_oracle_and_the_loop(sm, random_sets, threshold_bp):
    queries, rows, counts, db, qs, q_mhs = random_sets
    want = gc.oracle_picks(queries, rows, threshold_bp)
    got = db.gather_many(qs, threshold_bp)
    assert got == want
    assert got == [db.gather(mh, threshold_bp) for mh in q_mhs]
    assert (np.count_nonzero(counts, axis=1) > 256).all()                   # more candidates than one stride of 256 lanes
    n = [len(w) for w in want]
    assert max(n) >= 1 and (threshold_bp != 60_000 or min(n) == 0)


# 3 ---- lane and word edges ---------------------------------------------------------------------------------------------------------
def test_lane_and_word_edges(sm):
    queries, rows, owner = gc.edge_case()
    counts = mc.dense_counts(queries, rows)
    assert np.count_nonzero(counts, axis=1).tolist() == gc.CANDIDATE_COUNTS + [5] * len(gc.QUERY_SIZES) + [2]
    assert [len(q) for q in queries] == [40] * len(gc.CANDIDATE_COUNTS) + gc.QUERY_SIZES + [70]
    want = gc.oracle_picks(queries, rows)
    db, _ = sketchset(sm, rows)
    qs, _ = sketchset(sm, queries)
    assert db.gather_many(qs) == want
    first_row = np.searchsorted(owner, np.arange(len(queries)))
    for q, picks in enumerate(want[:-1]):
        assert picks and picks[0][1] >= 1
        if counts[q].astype(bool).sum() >= 2:
            assert first_row[q] + 1 not in [r for r, _ in picks]            # the second of two identical rows is never picked
    assert want[-1] == [(len(rows) - 1, 70)]                                # a query identical to a row: one round
    check_raw(queries, rows, want, gc.hits_of(queries, rows, counts=counts))


def test_rows_around_the_fill_group_of_512(sm):
    queries, rows = gc.long_row_case()
    assert [len(r) for r in rows] == gc.LONG_ROWS
    db, _ = sketchset(sm, rows)
    qs, q_mhs = sketchset(sm, queries)
    for threshold_bp in (0, 300_000):
        want = gc.oracle_picks(queries, rows, threshold_bp)
        assert db.gather_many(qs, threshold_bp) == want == [db.gather(mh, threshold_bp) for mh in q_mhs]
        thr = gc.threshold_hashes(threshold_bp, 1000)
        check_raw(queries, rows, want, gc.hits_of(queries, rows, need=thr), thr=thr)
    assert len(want[0]) >= 2


# 4 ---- the raw entry: guards, grids, determinism -------------------------------------------------------------------------------------
def test_raw_entry_grids_and_determinism(sm, random_sets):
    queries, rows, counts, _, _, _ = random_sets
    queries, counts = queries[:12], counts[:12]
    thr = 20
    want = gc.oracle_picks(queries, rows, 20_000)
    hits = gc.hits_of(queries, rows, need=thr, counts=counts)
    runs = [check_raw(queries, rows, want, hits, thr=thr, grid=grid) for grid in (1, 2, 0, 0)]
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))    # grid = 1, grid = 2, and two calls alike: identical arrays
    # a hit whose common count is not what the row shares with the query is found, not believed
    bad = [a.copy() for a in hits]
    bad[2][5] = int(hits[2][5]) + 1
    got, _, _, _, _, guards_ok = raw_run(queries, rows, bad, thr=thr)
    assert got is None and guards_ok
    from sourmash_amd._lowlevel import lib
    lib.sourmash_err_clear()


# 5 ---- caps ------------------------------------------------------------------------------------------------------------------------
def test_caps_and_the_way_out(sm):
    from sourmash_amd._lowlevel import lib
    queries, rows, _ = gc.edge_case()
    counts = mc.dense_counts(queries, rows)
    hits = gc.hits_of(queries, rows, counts=counts)
    want = gc.oracle_picks(queries, rows)
    n_cand = np.count_nonzero(counts, axis=1)
    sizes = np.array([len(q) for q in queries])
    mqh, mcand = 64, 255
    beyond = (sizes > mqh) | (n_cand > mcand)
    assert np.flatnonzero(beyond).tolist() == [5, 6, 13, 14]                # 256 and 257 candidates, 65 and 70 hashes
    got, out_rows, out_isect, rounds, status, guards_ok = raw_run(queries, rows, hits, max_query_hashes=mqh, max_candidates=mcand)
    assert guards_ok and status.tolist() == beyond.astype(int).tolist()
    assert (rounds[beyond] == MARK).all()                                   # nothing is written for them
    first = np.searchsorted(hits[0], np.arange(len(queries) + 1))
    picks = gc.picks_from_slots(hits, out_rows, out_isect, np.where(beyond, 0, rounds), len(queries))
    for q in range(len(queries)):
        if beyond[q]:
            assert (out_rows[first[q]:first[q + 1]] == MARK).all() and (out_isect[first[q]:first[q + 1]] == MARK).all()
        else:
            assert picks[q] == want[q]
    assert got == sum(len(want[q]) for q in range(len(queries)) if not beyond[q])
    db, _ = sketchset(sm, rows)
    qs, _ = sketchset(sm, queries)
    assert db._many_gather(qs, 0).stats["way_out_queries"] == 0
    lib.smgpu_gather_many_set_limits(mqh, mcand, 0)
    try:
        res = db._many_gather(qs, 0)
        full = res.per_query()
        stats = res.stats
    finally:
        lib.smgpu_gather_many_set_limits(0, 0, 0)
    assert full == want                                                     # the answer is complete
    assert stats["way_out_queries"] == 4 and stats["way_out_ms"] > 0


# 6 ---- batches ---------------------------------------------------------------------------------------------------------------------
def test_batches(sm, random_sets):
    from sourmash_amd._lowlevel import lib
    queries, rows, counts, db, qs, _ = random_sets
    want = gc.oracle_picks(queries, rows)
    one = db._many_gather(qs, 0)
    assert one.stats["batches"] == 1 and one.per_query() == want
    per_query = counts.sum(axis=1)
    budget = int(per_query.max()) * 15                                      # at most 14 queries a batch: 3 batches or more for 40
    lib.smgpu_gather_many_set_limits(0, 0, budget)
    try:
        res = db._many_gather(qs, 0)
        got, stats = res.per_query(), res.stats
    finally:
        lib.smgpu_gather_many_set_limits(0, 0, 0)
    assert got == want
    # the batch count is the rule's: contiguous ranges whose entries stay under the budget
    n_batches, total = 1, 0
    for w in per_query.tolist():
        if total and total + w >= budget:
            n_batches, total = n_batches + 1, 0
        total += w
    assert stats["batches"] == n_batches >= 3


# 7 ---- different scaled ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled_q,scaled_db", [(1000, 2000), (2000, 1000)])
def test_coarser_scaled(sm, scaled_q, scaled_db):
    import oracle
    from sourmash_amd.minhash import _get_max_hash_for_scaled
    queries, rows, cutoff = gc.scaled_case(_get_max_hash_for_scaled(scaled_q), _get_max_hash_for_scaled(scaled_db))
    assert cutoff == mc.MAX_HASH_2000
    db, _ = sketchset(sm, rows, scaled=scaled_db)
    qs, _ = sketchset(sm, queries, scaled=scaled_q)

    def down(hashes, scaled):
        mh = oracle.OracleMinHash(0, 21, scaled=scaled)
        mh.add_many([int(v) for v in hashes])
        assert len(mh) == len(hashes)
        return np.array(sorted(int(v) for v in (mh.downsample_scaled(2000) if scaled != 2000 else mh).mins), dtype=np.uint64)
    dq, drows = [down(a, scaled_q) for a in queries], [down(b, scaled_db) for b in rows]
    assert [a.tolist() for a in dq] == [a.tolist() for a in gc.cut(queries, cutoff)] and [b.tolist() for b in drows] == [b.tolist() for b in gc.cut(rows, cutoff)]
    assert sum(len(a) for a in queries + rows) > sum(len(a) for a in dq + drows)      # the cutoff did drop hashes
    ddb, _ = sketchset(sm, drows, scaled=2000)
    _, dq_mhs = sketchset(sm, dq, scaled=2000)
    for threshold_bp in (0, 4000, 4001):
        want = gc.oracle_picks(dq, drows, threshold_bp, 2000)
        res = db._many_gather(qs, threshold_bp)
        assert res.scaled == 2000 and res.per_query() == want
        assert [ddb.gather(mh, threshold_bp) for mh in dq_mhs] == want      # SketchSet.gather on both sides downsampled
    assert want != gc.oracle_picks(dq, drows, 4000, 2000)                   # ceil(4001 / 2000) = 3 hashes: one more than 4000 asks for
    thr = 2
    check_raw(queries, rows, gc.oracle_picks(dq, drows, 4000, 2000), gc.hits_of(queries, rows, cutoff, thr), cutoff=cutoff, thr=thr)


# 8 ---- objects ---------------------------------------------------------------------------------------------------------------------
def test_linear_index_gather_many_equals_the_loop(sm):
    from sourmash_amd.index import LinearIndex
    sigs = [sm.load_one_signature_from_json(f, ksize=21) for f in sorted(glob.glob(golden("gather", "GCF_*.sig")))]
    assert len(sigs) == 12
    combined = sm.load_one_signature_from_json(golden("gather", "combined.sig"), ksize=21)
    db = LinearIndex(sigs)
    queries = [combined, sigs[0], sigs[7]]
    assert all(q.minhash.scaled == sigs[0].minhash.scaled and not q.minhash.track_abundance for q in queries)
    for threshold_bp in (0, 100_000):
        want = [db.counter_gather(q, threshold_bp).gather_all(threshold_bp) for q in queries]
        got = db.gather_many(queries, threshold_bp)
        assert got == want
        assert len(want[0]) > 2 and want[1][0] == (sigs[0].md5sum(), len(sigs[0].minhash))
    assert db.gather_many([], 0) == []


def _sig(sm, hashes, name, scaled=1000, **kw):
    mh = sm.MinHash(0, 21, scaled=scaled, **kw)
    mh.add_many([int(h) for h in hashes])
    return sm.SourmashSignature(mh, name=name)


def test_linear_index_mixed_scaled_takes_the_loop(sm, monkeypatch):
    from sourmash_amd.index import LinearIndex, SketchSet
    fine = _sig(sm, list(range(1, 40)) + [mc.MAX_HASH_2000 + 5], "fine")
    coarse = _sig(sm, range(20, 60), "coarse", scaled=2000)
    other = _sig(sm, range(50, 80), "other")
    db = LinearIndex([fine, coarse, other])
    queries = [_sig(sm, range(1, 70), "q0"), _sig(sm, range(30, 80), "q1")]
    want = [db.counter_gather(q, 0).gather_all(0) for q in queries]
    monkeypatch.setattr(SketchSet, "gather_many", lambda *a, **k: pytest.fail("a coarser subject must take the loop"))
    assert db.gather_many(queries, 0) == want and all(want)
    # queries of two scaled values take it as well
    mixed = [queries[0], _sig(sm, range(2, 70, 2), "q2", scaled=2000)]
    assert db.gather_many(mixed, 0) == [db.counter_gather(q, 0).gather_all(0) for q in mixed]


def test_linear_index_errors_are_the_loops(sm):
    from sourmash_amd.index import LinearIndex
    db = LinearIndex([_sig(sm, range(1, 40), "a"), _sig(sm, range(20, 60), "b")])
    good = _sig(sm, range(1, 70), "q")
    abund = _sig(sm, range(1, 70), "qa", track_abundance=True)
    cases = [(LinearIndex([]), [good], 0),                                  # an empty index
             (db, [good, _sig(sm, [], "empty")], 0),                        # an empty query, behind a good one
             (db, [good, _sig(sm, range(1, 4), "small")], 5000),            # threshold_bp unattainable for the second query
             (db, [good, abund], 0)]                                        # an abundance query: not flat, the loop itself
    for index, queries, threshold_bp in cases:
        try:
            want = [index.counter_gather(q, threshold_bp).gather_all(threshold_bp) for q in queries]
            raised = None
        except Exception as exc:                                             # noqa: BLE001
            raised = exc
        if raised is None:
            assert index.gather_many(queries, threshold_bp) == want
        else:
            with pytest.raises(type(raised)) as got:
                index.gather_many(queries, threshold_bp)
            assert str(got.value) == str(raised)
    with pytest.raises(ValueError, match="no signatures to search"):
        LinearIndex([]).gather_many([good], 0)
    with pytest.raises(ValueError, match="empty"):
        db.gather_many([good, _sig(sm, [], "empty")], 0)
    with pytest.raises(ValueError, match="unattainable"):
        db.gather_many([good, _sig(sm, range(1, 4), "small")], 5000)


# 9 ---- mismatches ------------------------------------------------------------------------------------------------------------------
def test_mismatches_raise_what_overlaps_many_raises(sm):
    _, rows, _ = mc.hand_case()
    db, _ = sketchset(sm, rows)
    for kw in (dict(ksize=31), dict(ksize=7, is_protein=True), dict(seed=43)):
        qs, _ = sketchset(sm, [mc.u64([5, 7])], **{"ksize": 21, **kw})
        with pytest.raises(ValueError) as one:
            db.overlaps_many(qs)
        with pytest.raises(ValueError) as many:
            db.gather_many(qs)
        assert str(many.value) == str(one.value), kw
    num = sm.MinHash(500, 21)
    num.add_many([5, 7])
    nums = sm.SketchSet([num])
    for a, b in ((db, nums), (nums, db)):
        with pytest.raises(ValueError, match="scaled") as one:
            a.overlaps_many(b)
        with pytest.raises(ValueError, match="scaled") as many:
            a.gather_many(b, 1000)
        assert str(many.value) == str(one.value)
    with pytest.raises(TypeError):
        db.gather_many([num])
