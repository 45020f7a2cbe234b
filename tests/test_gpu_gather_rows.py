"""GPU parity of the gather-rows pass (csrc/gather_rows.hip; SketchSet.gather_stats_many / gather_stats and LinearIndex.gather_results_many on
top): the raw entry against the numpy restatement of tests/gather_rows_cases.py on every case, the handle entries against gather_many, and
the rows against the gatherresultdicts of the GatherDatabases loop, every column, floats by ==.  Run with -m gpu."""
import numpy as np
import pytest

import gather_many_cases as gc
import gather_rows_cases as rc
import many_cases as mc
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 8
MARK = 0x5a


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    assert sourmash_amd.gpu_available()
    return sourmash_amd


def sketchset(sm, rows, scaled=1000, abunds=None, **kw):
    mhs = []
    for i, r in enumerate(rows):
        mh = sm.MinHash(0, 21, scaled=scaled, track_abundance=abunds is not None, **kw)
        if abunds is not None:
            mh.set_abundances({int(h): int(a) for h, a in zip(r, abunds[i])})
        else:
            mh.add_many([int(h) for h in r])
        assert len(mh) == len(r)
        mhs.append(mh)
    return sm.SketchSet([mh.flatten() for mh in mhs]), mhs


# ---- the raw entry on torch tensors -------------------------------------------------------------------------------------------------
def raw_run(queries, abunds, rows, pick_rows, cutoff=mc.U64_MAX, grid=0, pick_csr=None, n_rows=None, qoff=None):
    "-> (returned or None on an error, outputs by name, guards untouched) of smgpu_gather_rows_raw"
    import torch
    from sourmash_amd._lowlevel import lib

    def dev(a, dtype):
        a = np.concatenate([np.ascontiguousarray(a, dtype=dtype), np.zeros(4, dtype=dtype)])
        return torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).cuda()
    qh, qoff0 = mc.csr(queries)
    h, off = mc.csr(rows)
    poff, prow = rc.pick_csr(pick_rows) if pick_csr is None else pick_csr
    m, n, q_total, n_picks = len(queries), len(rows) if n_rows is None else n_rows, len(qh), len(prow)
    d_qh, d_qoff, d_h, d_off = dev(qh, np.uint64), dev(qoff0 if qoff is None else qoff, np.uint64), dev(h, np.uint64), dev(off, np.uint64)
    d_qa = dev(np.concatenate([np.asarray(a, dtype=np.uint64) for a in abunds]), np.uint64) if abunds is not None else None
    d_poff, d_prow = dev(poff, np.uint64), dev(prow, np.uint32)
    names = ("owner", "orig_common", "unique", "weighted", "abund_offsets", "abund_values", "query_sizes", "total_weighted")
    sizes = (q_total, n_picks, n_picks, n_picks, n_picks + 1, q_total, m, m)
    widths = (4, 4, 4, 8, 8, 8, 8, 8)
    outs = [torch.full(((size + GUARD) * w,), MARK, dtype=torch.uint8, device="cuda") for size, w in zip(sizes, widths)]
    ws_bytes = int(lib.smgpu_gather_rows_workspace_bytes(m, q_total, n_picks))
    ws = torch.full((ws_bytes + 64,), MARK, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib.sourmash_err_clear()
    got = lib.smgpu_gather_rows_raw(d_qh.data_ptr(), d_qa.data_ptr() if d_qa is not None else None, d_qoff.data_ptr(), m, q_total, d_h.data_ptr(),
                                    d_off.data_ptr(), n, d_poff.data_ptr(), d_prow.data_ptr(), n_picks, cutoff, grid, *[o.data_ptr() for o in outs],
                                    ws.data_ptr(), ws_bytes, None)
    code = lib.sourmash_err_get_last_code()
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    guards_ok = all((a[s * w:] == MARK).all() for a, s, w in zip(host, sizes, widths)) and bool((ws[ws_bytes:] == MARK).all())
    out = {k: a[:s * w].view(np.uint32 if w == 4 else np.uint64) for k, a, s, w in zip(names, host, sizes, widths)}
    if code == 0:
        out["abund_values"] = out["abund_values"][:int(got)]
    lib.sourmash_err_clear()
    return (int(got) if code == 0 else None), out, guards_ok


def same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


# 1 ---- the raw entry on every case --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_raw_entry_equals_the_restatement(sm, name):
    queries, abunds, rows, picks, pick_rows, cutoff = rc.cases()[name]
    want = rc.expected(name)
    got, out, guards_ok = raw_run(queries, abunds, rows, pick_rows, cutoff)
    assert guards_ok and got == int(want["unique"].sum())
    same(out, want)
    if name == "hand":
        e = rc.HAND_EXPECTED
        assert out["orig_common"].tolist() == e["orig_common"] and out["unique"].tolist() == e["unique"] and out["weighted"].tolist() == e["weighted"]
        assert out["abund_values"].tolist() == e["abund_values"] and out["total_weighted"].tolist() == e["total_weighted"]
    if name == "useless_picks":
        assert out["unique"].tolist() == [5, 0, 2, 0, 0, 4, 0]


def test_raw_entry_grids_determinism_and_refusals(sm):
    queries, abunds, rows, _, pick_rows, cutoff = rc.cases()["long_rows"]
    want = rc.expected("long_rows")
    for grid in (1, 2, 0):                                                  # one workgroup walks every pick and every position
        got, out, guards_ok = raw_run(queries, abunds, rows, pick_rows, cutoff, grid=grid)
        assert guards_ok and got == int(want["unique"].sum())
        same(out, want)
    # what the device finds wrong with its input is an error, and nothing is written past an array
    queries, abunds, rows, _, pick_rows, _ = rc.cases()["hand"]
    _, prow = rc.pick_csr(pick_rows)
    for kw in (dict(n_rows=6), dict(pick_csr=(np.array([0, 4, 0, 4], dtype=np.uint64), prow)), dict(pick_csr=(np.array([0, 0, 3, 3], dtype=np.uint64), prow)),
               dict(qoff=[0, 12, 0, 14]), dict(qoff=[0, 0, 12, 15])):
        got, _, guards_ok = raw_run(queries, abunds, rows, pick_rows, **kw)
        assert got is None and guards_ok, kw


# 2 ---- the handle entries --------------------------------------------------------------------------------------------------------------
def check_stats(stats, want, picks, row_sizes):
    assert stats.per_query() == picks
    assert stats.orig_common.tolist() == want["orig_common"].tolist() and stats.weighted.tolist() == want["weighted"].tolist()
    assert stats.abund_offsets.tolist() == want["abund_offsets"].tolist() and stats.abund_values.tolist() == want["abund_values"].tolist()
    assert stats.query_sizes.tolist() == want["query_sizes"].tolist() and stats.total_weighted.tolist() == want["total_weighted"].tolist()
    assert stats.row_sizes.tolist() == row_sizes.tolist()


@pytest.mark.parametrize("name", ["hand", "edge", "edge_flat", "long_rows"])
def test_gather_stats_many_equals_gather_many_and_the_restatement(sm, name):
    queries, abunds, rows, picks, _, cutoff = rc.cases()[name]
    want = rc.expected(name)
    db, _ = sketchset(sm, rows)
    qs, q_mhs = sketchset(sm, queries, abunds=abunds)
    stats = db.gather_stats_many(qs, 0, abunds=abunds)
    assert stats.per_query() == db.gather_many(qs, 0) == picks
    check_stats(stats, want, picks, mc.sizes_at(rows))
    assert stats.scaled == 1000 and stats.with_abundance == (abunds is not None)
    assert set(stats.stats) == {"gather_ms", "owner_ms", "tally_ms", "sort_ms", "call_ms"} and stats.stats["call_ms"] > 0
    if abunds is not None:                                                  # a flat array is the same as one array per query
        flat = db.gather_stats_many(qs, 0, abunds=np.concatenate(abunds))
        assert flat.abund_values.tolist() == stats.abund_values.tolist() and flat.weighted.tolist() == stats.weighted.tolist()
    # one query through the one-query gather == its part of the many-query call
    q = 1 if name in ("hand", "long_rows") else 3
    one = db.gather_stats(q_mhs[q], 0)
    lo, hi = int(stats.offsets[q]), int(stats.offsets[q + 1])
    assert one.per_query() == [picks[q]] and len(one) == 1 and hi > lo
    for field in ("pick_rows", "isect", "orig_common", "weighted"):
        assert getattr(one, field).tolist() == getattr(stats, field)[lo:hi].tolist(), field
    a, b = int(stats.abund_offsets[lo]), int(stats.abund_offsets[hi])
    assert one.abund_values.tolist() == stats.abund_values[a:b].tolist() and (one.abund_offsets + np.uint64(a)).tolist() == stats.abund_offsets[lo:hi + 1].tolist()
    assert one.query_sizes.tolist() == [stats.query_sizes[q]] and one.total_weighted.tolist() == [stats.total_weighted[q]]
    assert one.row_sizes.tolist() == stats.row_sizes.tolist() and one.with_abundance == (abunds is not None)
    if abunds is not None:
        ignored = db.gather_stats(q_mhs[q], 0, ignore_abundance=True)
        assert not ignored.with_abundance and ignored.weighted.tolist() == ignored.isect.tolist() and ignored.total_weighted.tolist() == ignored.query_sizes.tolist()


@pytest.mark.parametrize("scaled_q,scaled_db", [(1000, 2000), (2000, 1000)])
def test_gather_stats_at_the_coarser_scaled(sm, scaled_q, scaled_db):
    name = f"cutoff_{scaled_q}_{scaled_db}"
    queries, abunds, rows, picks, _, cutoff = rc.cases()[name]
    want = rc.expected(name)
    db, _ = sketchset(sm, rows, scaled=scaled_db)
    qs, q_mhs = sketchset(sm, queries, scaled=scaled_q, abunds=abunds)
    stats = db.gather_stats_many(qs, 0, abunds=abunds)
    assert stats.scaled == 2000 and stats.query_scaled == scaled_q
    check_stats(stats, want, picks, mc.sizes_at(rows, cutoff))
    one = db.gather_stats(q_mhs[0], 0)
    assert one.per_query() == [picks[0]] and one.scaled == 2000
    assert one.weighted.tolist() == stats.weighted[:len(picks[0])].tolist() and one.total_weighted.tolist() == [stats.total_weighted[0]]
    # a threshold in bp is taken at the common scaled: ceil(4001 / 2000) = 3 hashes
    assert db.gather_stats_many(qs, 4001, abunds=abunds).per_query() == gc.oracle_picks(queries, rows, 4001, 2000, cutoff)


def test_abundance_arguments_are_checked(sm):
    db, _ = sketchset(sm, gc.HAND_ROWS)
    qs, _ = sketchset(sm, gc.HAND_QUERIES)
    with pytest.raises(ValueError):
        db.gather_stats_many(qs, 0, abunds=np.ones(13, dtype=np.uint64))
    with pytest.raises(ValueError):
        db.gather_stats_many(qs, 0, abunds=[np.ones(12, dtype=np.uint64)])
    with pytest.raises(TypeError):
        db.gather_stats_many([qs], 0)
    other, _ = sketchset(sm, [mc.u64([5, 7])], seed=43)
    with pytest.raises(ValueError) as one:
        db.overlaps_many(other)
    with pytest.raises(ValueError) as many:
        db.gather_stats_many(other)
    assert str(many.value) == str(one.value)


# 3 ---- the rows against the loop of GatherDatabases ----------------------------------------------------------------------------------------
def loop_rows(index, queries, threshold_bp, ignore_abundance=False):
    from sourmash_amd.search import GatherDatabases
    return [[r.gatherresultdict for r in GatherDatabases(q, [index.counter_gather(q, threshold_bp)], threshold_bp=threshold_bp,
                                                         ignore_abundance=ignore_abundance)] for q in queries]


def same_rows(got, want):
    assert len(got) == len(want)
    for g_rows, w_rows in zip(got, want):
        assert len(g_rows) == len(w_rows)
        for g, w in zip(g_rows, w_rows):
            assert sorted(g) == sorted(w)
            for k in w:
                assert g[k] == w[k] and type(g[k]) is type(w[k]), (k, g[k], w[k])
    assert got == want


def test_set_level_rows_equal_the_loop(sm):
    "GatherStats.rows() of a SketchSet call: names, file names and md5s from the sets' manifests and md5sums"
    from sourmash_amd.index import LinearIndex
    queries, abunds, rows, picks, _, _ = rc.cases()["hand"]
    row_sigs = [_sig(sm, r, f"row{i}") for i, r in enumerate(rows)]
    q_sigs = [_sig(sm, q, f"query{i}", abunds=a) for i, (q, a) in enumerate(zip(queries, abunds))]
    db = sm.SketchSet([s.minhash for s in row_sigs])
    db.set_names([s.name for s in row_sigs], [s.filename for s in row_sigs])
    qs = sm.SketchSet([s.minhash.flatten() for s in q_sigs])
    qs.set_names([s.name for s in q_sigs], [s.filename for s in q_sigs])
    index = LinearIndex([s for s in row_sigs if len(s.minhash)])
    for threshold_bp in (0, 2000):
        want = loop_rows(index, [q_sigs[1]], threshold_bp)[0]
        got = db.gather_stats_many(qs, threshold_bp, abunds=abunds).rows()
        assert got[0] == [] and got[2] == []
        same_rows([got[1]], [want])
        one = db.gather_stats(q_sigs[1].minhash, threshold_bp)
        one.query_info = [dict(query_name="query1", query_filename="query1.sig", query_md5=q_sigs[1].md5sum()[:8])]
        same_rows(one.rows(), [want])
        flat = db.gather_stats_many(qs, threshold_bp).rows()
        same_rows([flat[1]], loop_rows(index, [q_sigs[1]], threshold_bp, ignore_abundance=True))
    assert len(want) == 3 and want[0]["name"] == "row1" and want[0]["filename"] == "row1.sig"


@pytest.fixture(scope="module")
def abund_golden(sm):
    from sourmash_amd.index import LinearIndex
    genomes = [sm.load_one_signature_from_json(golden("gather-abund", f"genome-s{i}.fa.gz.sig"), ksize=21) for i in (10, 11, 12)]
    queries = [sm.load_one_signature_from_json(golden("gather-abund", f"reads-{n}.sig"), ksize=21) for n in ("s10-s11", "s10x10-s11")]
    assert all(q.minhash.track_abundance for q in queries)
    return LinearIndex(genomes), queries


@pytest.mark.parametrize("ignore_abundance", [False, True])
def test_golden_abundance_rows_equal_the_loop(sm, abund_golden, monkeypatch, ignore_abundance):
    from sourmash_amd.search import GatherDatabases
    db, queries = abund_golden
    want = loop_rows(db, queries, 0, ignore_abundance)
    monkeypatch.setattr(GatherDatabases, "__next__", lambda self: pytest.fail("the native path builds no GatherResult"))
    got = db.gather_results_many(queries, 0, ignore_abundance=ignore_abundance)
    monkeypatch.undo()
    same_rows(got, want)
    assert [len(r) for r in got] == [2, 2]
    if not ignore_abundance:
        # the printed triples of tests/test_gpu_results.py: percent of the query (weighted), percent of the match, average abundance
        triples = [[(f"{r['f_unique_weighted'] * 100:.1f}%", f"{r['f_match'] * 100:.1f}%", f"{r['average_abund']:.1f}") for r in rows] for rows in got]
        assert triples[0] == [("49.6%", "78.5%", "1.8"), ("50.4%", "80.0%", "1.9")]
        assert triples[1] == [("91.0%", "100.0%", "14.5"), ("9.0%", "80.0%", "1.9")]
    else:
        assert all("average_abund" not in r and r["query_abundance"] is False and r["f_unique_weighted"] == r["f_unique_to_query"] for rows in got for r in rows)


def _sig(sm, hashes, name, scaled=1000, abunds=None, **kw):
    mh = sm.MinHash(0, 21, scaled=scaled, track_abundance=abunds is not None, **kw)
    if abunds is not None:
        mh.set_abundances({int(h): int(a) for h, a in zip(hashes, abunds)})
    else:
        mh.add_many([int(h) for h in hashes])
    return sm.SourmashSignature(mh, name=name, filename=name + ".sig")


def test_synthetic_abundance_queries_equal_the_loop(sm, monkeypatch):
    "300 rows x about 400 hashes, 40 abundance queries of about 670, threshold_bp = 30,000: several picks each"
    from sourmash_amd.index import LinearIndex
    from sourmash_amd.search import GatherDatabases
    queries, rows = mc.random_case(m=40, n=300, pool_size=4000)
    assert 350 < np.mean([len(r) for r in rows]) < 450
    abunds = rc.random_abunds(queries, 31)
    db = LinearIndex([_sig(sm, r, f"row{i}") for i, r in enumerate(rows) if len(r)], filename="db.sig")
    qsigs = [_sig(sm, q, f"query{i}", abunds=a) for i, (q, a) in enumerate(zip(queries, abunds))]
    qsigs[5] = _sig(sm, queries[5], "flat5")                                # a flat query among them
    want = loop_rows(db, qsigs, 30_000)
    monkeypatch.setattr(GatherDatabases, "__next__", lambda self: pytest.fail("the native path builds no GatherResult"))
    got = db.gather_results_many(qsigs, 30_000)
    monkeypatch.undo()
    same_rows(got, want)
    print("picks per query:", [len(r) for r in got])
    assert all(3 <= len(r) for i, r in enumerate(got) if i != 3) and len(got[3]) == 1
    assert got[0][0]["filename"] == "db.sig" and got[0][0]["query_filename"] == "query0.sig" and "average_abund" not in got[5][0]
    assert max(r["n_unique_weighted_found"] for r in got[0]) > 2**32


def test_subjects_of_one_md5_report_the_last_of_them(sm, monkeypatch):
    """The same sketch under two names, as a flat and an abundance copy, and at a finer scaled: one md5, so one entry of the loop's
    counter, which keeps the first one's place in the order and the LAST one's signature and location.  The native path picks the
    first of the equal rows and has to name the last."""
    from sourmash_amd.index import LinearIndex
    from sourmash_amd.search import GatherDatabases
    a, b, c = range(1, 60), range(40, 120), range(100, 130)
    subjects = [_sig(sm, a, "a-first"), _sig(sm, b, "b-first"), _sig(sm, a, "a-second"), _sig(sm, c, "c"), _sig(sm, b, "b-abund", abunds=range(1, 81)),
                _sig(sm, a, "a-finer", scaled=500)]
    assert len({s.md5sum() for s in subjects}) == 3 and subjects[0].md5sum() == subjects[5].md5sum() and subjects[1].md5sum() == subjects[4].md5sum()
    db = LinearIndex(subjects)                                              # no location of its own: every row reports its signature's file
    queries = [_sig(sm, range(1, 125), "q0", abunds=range(2, 126)), _sig(sm, range(30, 130), "q1")]
    want = loop_rows(db, queries, 0)
    monkeypatch.setattr(GatherDatabases, "__next__", lambda self: pytest.fail("the native path builds no GatherResult"))
    got = db.gather_results_many(queries, 0)
    monkeypatch.undo()
    same_rows(got, want)
    assert [(r["name"], r["filename"]) for r in got[0]] == [("b-abund", "b-abund.sig"), ("a-finer", "a-finer.sig"), ("c", "c.sig")]
    assert [r["name"] for r in got[1]] == ["b-abund", "a-finer", "c"] and got[0][1]["md5"] == subjects[0].md5sum()


def test_fallback_conditions_return_the_loops_result(sm, monkeypatch):
    from sourmash_amd.index import LinearIndex, SketchSet
    fine = _sig(sm, list(range(1, 40)) + [mc.MAX_HASH_2000 + 5], "fine")
    coarse = _sig(sm, range(20, 60), "coarse", scaled=2000)
    other = _sig(sm, range(50, 80), "other")
    queries = [_sig(sm, range(1, 70), "q0", abunds=range(1, 70)), _sig(sm, range(30, 80), "q1")]
    monkeypatch.setattr(SketchSet, "gather_stats_many", lambda *a, **k: pytest.fail("these conditions take the loop"))
    db = LinearIndex([fine, coarse, other])                                 # a subject coarser than the queries
    want = loop_rows(db, queries, 0)
    same_rows(db.gather_results_many(queries, 0), want)
    assert all(want)
    db = LinearIndex([fine, other])                                         # queries of two scaled values
    mixed = [queries[0], _sig(sm, range(2, 70, 2), "q2", scaled=2000)]
    same_rows(db.gather_results_many(mixed, 0), loop_rows(db, mixed, 0))
    assert db.gather_results_many([], 0) == []


def test_errors_are_the_loops(sm):
    from sourmash_amd.index import LinearIndex
    db = LinearIndex([_sig(sm, range(1, 40), "a"), _sig(sm, range(20, 60), "b")])
    good = _sig(sm, range(1, 70), "q", abunds=range(1, 70))
    cases = [(LinearIndex([]), [good], 0),                                  # an empty index
             (db, [good, _sig(sm, [], "empty")], 0),                        # an empty query, behind a good one
             (db, [good, _sig(sm, range(1, 4), "small", abunds=[1, 2, 3])], 5000)]   # threshold_bp unattainable for the second query
    for index, queries, threshold_bp in cases:
        with pytest.raises(Exception) as want:                             # noqa: PT011
            loop_rows(index, queries, threshold_bp)
        with pytest.raises(type(want.value)) as got:
            index.gather_results_many(queries, threshold_bp)
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError, match="no signatures to search"):
        LinearIndex([]).gather_results_many([good], 0)
