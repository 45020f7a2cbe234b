"""GPU parity of the set algebra on a SketchSet (csrc/setops.hip; SketchSet.merge / subtract / intersect / downsample and the raw
entries under them): against numpy set operations, the loop over MinHash objects, and the golden fixtures, at the smallest shapes at
which the kernels can go wrong.  Run with -m gpu."""
import ctypes as C
import os

import numpy as np
import pytest

import setops_cases as sc
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 8
MARK = 0x5a5a5a5a5a5a5a5a

GOLDEN_GATHER = [("NC_003198.1", 487), ("NC_000853.1", 192), ("NC_011978.1", 169), ("NC_002163.1", 157),
                 ("NC_003197.2", 152), ("NC_009486.1", 92), ("NC_006905.1", 76), ("NC_011080.1", 59),
                 ("NC_011274.1", 42), ("NC_006511.1", 31), ("NC_011294.1", 7), ("NC_004631.1", 2)]


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    assert sourmash_amd.gpu_available()
    return sourmash_amd


@pytest.fixture(scope="module")
def geometry(sm):
    from sourmash_amd._lowlevel import lib
    wg, lds, split = C.c_uint32(), C.c_uint32(), C.c_uint64()
    lib.smgpu_setops_geometry(C.byref(wg), C.byref(lds), C.byref(split))
    return wg.value, lds.value, split.value


def dev(a, dtype=np.uint64):
    import torch
    a = np.concatenate([np.ascontiguousarray(a, dtype=dtype), np.zeros(4, dtype=dtype)])
    return torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).cuda()


def make_set(sm, rows, scaled=1000, num=0, ksize=21, names=None):
    "a SketchSet of these rows, from device tensors (any hash value goes: 0 and 2^64 - 1 too)"
    import torch
    flat, off = sc.csr(rows)
    d_h = torch.from_numpy(np.ascontiguousarray(flat).view(np.int64).copy()).cuda() if len(flat) else torch.zeros(0, dtype=torch.int64, device="cuda")
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    return sm.SketchSet.from_csr(d_h, d_off, ksize=ksize, scaled=scaled, num=num, names=names)


def rows_of(s):
    "the rows of a set on the host, with the sizes, the total and the manifest checked against them"
    rows = [s.minhash(r)._mins_array() for r in range(len(s))]
    assert [int(x) for x in s.sizes] == [len(r) for r in rows]
    assert s.total_hashes == sum(len(r) for r in rows)
    assert [m["n_hashes"] for m in s.manifest] == [len(r) for r in rows]
    return rows


def assert_rows_equal(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for r, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.uint64 and np.array_equal(a, np.asarray(b, dtype=np.uint64)), (what, r, len(a), len(b))


def gcf_paths():
    return [golden("gather", f) for f in sorted(os.listdir(golden("gather"))) if f.startswith("GCF_")]


# ---- golden cases -------------------------------------------------------------------------------------------------------------------
def test_golden_merge_and_intersection_of_47_and_63(sm):
    pair = sm.SketchSet.load([golden("pairs", "47.fa.sig"), golden("pairs", "63.fa.sig")], ksize=31)
    assert len(pair) == 2
    merged = pair.merge(names=["47+63"])
    want = sm.load_one_signature_from_json(golden("pairs", "47+63.fa.sig"), ksize=31).minhash
    assert len(merged) == 1 and merged.total_hashes == 7886 == len(want)
    assert merged.md5sums()[0] == "491c0a81b2cfb0188c0d3b46837c2f42" == want.md5sum()
    assert np.array_equal(rows_of(merged)[0], want._mins_array())
    assert merged.params == pair.params and merged.manifest[0]["name"] == "47+63"
    both = pair.merge(min_rows="all")
    assert both.total_hashes == 2529
    a, b = rows_of(pair)
    assert np.array_equal(rows_of(both)[0], np.intersect1d(a, b))
    # the same intersection by the filter, in both forms of `other`
    assert np.array_equal(rows_of(pair.subset([0]).intersect(pair.subset([1])))[0], np.intersect1d(a, b))
    assert np.array_equal(rows_of(pair.subset([0]).intersect(pair.minhash(1)))[0], np.intersect1d(a, b))
    assert len(pair) == 2 and [int(x) for x in pair.sizes] == [len(a), len(b)]      # the receiver is unchanged


def test_golden_merge_of_2_and_63(sm):
    pair = sm.SketchSet.load([golden("pairs", "2.fa.sig"), golden("pairs", "63.fa.sig")], ksize=31)
    want = sm.load_one_signature_from_json(golden("pairs", "2+63.fa.sig"), ksize=31).minhash
    merged = pair.merge()
    assert merged.total_hashes == 7939 == len(want) and np.array_equal(rows_of(merged)[0], want._mins_array())
    assert merged.md5sums()[0] == want.md5sum()


def test_golden_gather_by_overlaps_and_subtract(sm):
    db = sm.SketchSet.load(gcf_paths(), ksize=21, moltype="DNA")
    query = sm.load_one_signature_from_json(golden("gather", "combined.sig"), ksize=21).minhash
    q = sm.SketchSet([query.flatten()]).downsample(db.params[3])        # (a result: a full set, whose rows come back as objects)
    got = []
    for step in range(len(db) + 1):
        ov = db.overlaps(q.minhash(0))
        best = int(np.argmax(ov))
        if ov[best] == 0:
            break
        got.append((db.manifest[best]["name"].split()[0], int(ov[best])))
        q = q.subtract(db.subset([best]) if step % 2 else db.minhash(best))       # both forms of one sketch
    assert got == GOLDEN_GATHER and got[0][0] == "NC_003198.1" and got[-1][0] == "NC_004631.1"
    assert [n for _, n in got] == [487, 192, 169, 157, 152, 92, 76, 59, 42, 31, 7, 2]


# ---- merge edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_rows", [1, 2, "all", 9])
def test_merge_cases_against_numpy(sm, min_rows):
    for name, rows, groups, n_groups, max_hash in sc.merge_cases():
        s = make_set(sm, rows, scaled=1 if max_hash == sc.U64_MAX else 1000)
        got = s.merge(groups, min_rows=min_rows)
        assert len(got) == n_groups and got.params == s.params, name
        assert_rows_equal(rows_of(got), sc.expected_merge(rows, groups, n_groups, min_rows), name)


def test_merge_of_one_row_is_that_row(sm):
    name, rows, groups, n_groups, _ = sc.merge_cases()[1]
    s = make_set(sm, rows)
    assert np.array_equal(rows_of(s.merge(groups))[4], rows[6])         # group 4 is row 6 alone
    one = make_set(sm, [rows[7]])
    for kw in (dict(), dict(min_rows="all")):
        got = one.merge(**kw)
        assert_rows_equal(rows_of(got), [rows[7]])
        assert got.md5sums() == one.md5sums()
    # names are the groups'
    named = s.merge(groups, names=["a", "b", "c", "d", "e"])
    assert [m["name"] for m in named.manifest] == ["a", "b", "c", "d", "e"]


def test_merge_on_both_sides_of_the_key_form_boundary(sm):
    from sourmash_amd._lowlevel import lib

    def packed(n_groups):
        p = C.c_uint32()
        lib.smgpu_setops_key_form(sc.MAX_HASH_1000, n_groups, None, None, C.byref(p))
        return bool(p.value)
    edge = max(g for g in range(2, 2000) if packed(g))
    assert packed(edge) and not packed(edge + 1)
    results = {}
    for n_groups in (edge, edge + 1):
        rows, groups, _ = sc.boundary_case(n_groups)
        assert max(groups) == edge - 1
        groups = groups + ([n_groups - 1] if n_groups > edge else [])    # (the wide side really has its last group: an empty row in it)
        s = make_set(sm, rows + ([sc.u64([])] if n_groups > edge else []))
        for min_rows in (1, "all"):
            got = s.merge(groups, min_rows=min_rows)
            assert len(got) == n_groups
            want = sc.expected_merge(rows, groups[:len(rows)], n_groups, min_rows)
            sizes = [int(x) for x in got.sizes]
            assert sizes == [len(w) for w in want]
            for g in (0, 1, edge - 1):
                assert np.array_equal(got.minhash(g)._mins_array(), want[g]), (n_groups, min_rows, g)
            results[(n_groups, min_rows)] = [got.minhash(g)._mins_array() for g in (0, 1, edge - 1)]
    for min_rows in (1, "all"):
        assert_rows_equal(results[(edge, min_rows)], results[(edge + 1, min_rows)])


def test_merge_of_num_sketches_against_the_minhash_loop(sm):
    paths = sorted(os.path.join(golden("demo"), f) for f in os.listdir(golden("demo")) if f.endswith(".sig"))
    mhs = [sm.load_one_signature_from_json(p, ksize=31).minhash for p in paths]
    assert all(mh.num == 500 and len(mh) == 500 for mh in mhs)

    def head(mh, k):
        out = sm.MinHash(500, 31)
        out.add_many(mh._mins_array()[:k])
        return out
    # unions longer than num (two full sketches), equal to it (one full sketch), shorter (two short ones), and an empty group
    members = [mhs[0], mhs[1], mhs[2], head(mhs[3], 120), head(mhs[4], 200), mhs[5], mhs[6], mhs[0]]
    groups = [0, 0, 1, 2, 2, 4, 4, 4]
    s = sm.SketchSet([m.flatten() for m in members])
    got = s.merge(groups)
    assert got.params[4] == 500 and len(got) == 5
    want = []
    for g in range(5):
        acc = sm.MinHash(500, 31)
        for m, gg in zip(members, groups):
            if gg == g:
                acc.merge(m)
        want.append(acc._mins_array())
    assert [len(w) for w in want][1:4] == [500, len(want[2]), 0] and len(want[2]) < 500 and len(want[0]) == 500
    assert_rows_equal(rows_of(got), want)
    for min_rows in (2, "all"):
        with pytest.raises(ValueError):
            s.merge(groups, min_rows=min_rows)


# ---- filter edges -----------------------------------------------------------------------------------------------------------------------
def check_filter(sm, rows, other, what, scaled=1000):
    "both operations, through the set-level methods; other: one array (as a MinHash and as a set of one row) or one array per row"
    s = make_set(sm, rows, scaled=scaled, names=[f"row {r}" for r in range(len(rows))])
    if isinstance(other, np.ndarray):
        mh = sm.MinHash(0, 21, scaled=scaled)
        mh.add_many(other)
        assert len(mh) == len(other)
        others = [mh, make_set(sm, [other], scaled=scaled)]
    else:
        others = [make_set(sm, other, scaled=scaled)]
    for o in others:
        for keep_present, method in ((0, s.subtract), (1, s.intersect)):
            got = method(o)
            assert_rows_equal(rows_of(got), sc.expected_filter(rows, other, keep_present), (what, keep_present))
            assert [m["name"] for m in got.manifest] == [f"row {r}" for r in range(len(rows))]
            assert got.params == s.params


@pytest.mark.parametrize("pattern", sc.pattern_names())
def test_filter_patterns_against_numpy(sm, geometry, pattern):
    rows, one, partners = sc.filter_pattern_case(pattern, geometry[2])
    assert max(len(r) for r in rows) > geometry[2]                      # one row above the split cap
    check_filter(sm, rows, one, pattern)
    check_filter(sm, rows, partners, pattern + ", row-wise")


def test_filter_one_sketch_edges(sm):
    for name, rows, other in sc.one_sketch_edge_cases():
        check_filter(sm, rows, other, name, scaled=1 if (len(other) and int(other[-1]) == sc.U64_MAX) else 1000)
    for k, rows, other in sc.bucket_cases():
        check_filter(sm, rows, other, f"bucket of {k}")


def test_filter_partner_rows(sm, geometry):
    rows, partners = sc.partner_cases(geometry[1])
    assert max(len(p) for p in partners) > geometry[1]
    check_filter(sm, rows, partners, "partners")
    empty = make_set(sm, [])
    assert len(empty.subtract(make_set(sm, [sc.u64([5])]))) == 0 and len(empty.intersect(make_set(sm, []))) == 0


def raw_filter(rows, other, keep_present, grid=0, capacity=None):
    "smgpu_setops_filter_raw on torch tensors -> (returned, rows or None, guards untouched)"
    import torch
    from sourmash_amd._lowlevel import lib
    flat, off = sc.csr(rows)
    n, total = len(rows), len(flat)
    if isinstance(other, np.ndarray):
        d_oh, d_ooff, o_len = dev(other), None, len(other)
    else:
        o_flat, o_off = sc.csr(other)
        d_oh, d_ooff, o_len = dev(o_flat), dev(o_off), 0
    d_h, d_off = dev(flat), dev(off)
    cap = total if capacity is None else capacity
    out = torch.from_numpy(np.full(cap + GUARD, MARK, dtype=np.uint64).view(np.int64)).cuda()
    out_off = torch.from_numpy(np.full(n + 1 + GUARD, MARK, dtype=np.uint64).view(np.int64)).cuda()
    result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    ws_bytes = int(lib.smgpu_setops_filter_workspace_bytes(n, total, o_len))
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    tail = torch.full((64,), 0x5a, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = tail
    torch.cuda.synchronize()
    lib.sourmash_err_clear()
    got = lib.smgpu_setops_filter_raw(d_h.data_ptr(), d_off.data_ptr(), n, total, d_oh.data_ptr(), d_ooff.data_ptr() if d_ooff is not None else None,
                                      o_len, keep_present, grid, out.data_ptr(), cap, out_off.data_ptr(), result.data_ptr(), ws.data_ptr(), ws_bytes, None)
    assert lib.sourmash_err_get_last_code() == 0
    torch.cuda.synchronize()
    res = result.cpu().numpy().view(np.uint64)
    assert got == res[0] and res[1] == 0
    h_out, h_off = out.cpu().numpy().view(np.uint64), out_off.cpu().numpy().view(np.uint64)
    guards_ok = bool((h_out[cap:] == MARK).all() and (h_off[n + 1:] == MARK).all() and (ws[ws_bytes:] == tail).all())
    assert h_off[n] == got
    if got > cap:
        return int(got), None, guards_ok and bool((h_out == MARK).all())
    return int(got), sc.uncsr(h_out[:got], h_off[:n + 1]), guards_ok and bool((h_out[got:] == MARK).all())


def test_filter_raw_entry_grids_and_capacity(sm, geometry):
    rows, one, partners = sc.filter_pattern_case("alternating", geometry[2])
    for other in (one, partners):
        for keep_present in (0, 1):
            want = sc.expected_filter(rows, other, keep_present)
            for grid in (0, 1, 3):                                      # one workgroup takes every item by ticket; three share them
                total, got, guards_ok = raw_filter(rows, other, keep_present, grid=grid)
                assert guards_ok and total == sum(len(w) for w in want)
                assert_rows_equal(got, want, (keep_present, grid))
            # a result that does not fit: the total and the offsets, nothing written
            total, got, guards_ok = raw_filter(rows, other, keep_present, capacity=sum(len(w) for w in want) - 1)
            assert guards_ok and got is None and total == sum(len(w) for w in want)


def test_merge_raw_entry(sm):
    import torch
    from sourmash_amd._lowlevel import lib
    name, rows, groups, n_groups, max_hash = sc.merge_cases()[1]
    flat, off = sc.csr(rows)
    n, total = len(rows), len(flat)
    # the CSR inside a longer buffer: the offsets do not start at 0
    lead = np.arange(7, dtype=np.uint64)
    d_h, d_off, d_g = dev(np.concatenate([lead, flat])), dev(off + np.uint64(7)), dev(groups, np.uint32)
    for need, need_all, min_rows in ((None, 0, 1), (np.full(n_groups, 2, dtype=np.uint32), 0, 2), (None, 1, "all")):
        d_need = dev(need, np.uint32) if need is not None else None
        out = torch.from_numpy(np.full(total + GUARD, MARK, dtype=np.uint64).view(np.int64)).cuda()
        out_off = torch.from_numpy(np.full(n_groups + 1 + GUARD, MARK, dtype=np.uint64).view(np.int64)).cuda()
        result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        ws_bytes = int(lib.smgpu_setops_merge_workspace_bytes(total, n_groups))
        ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
        tail = torch.full((64,), 0x5a, dtype=torch.uint8, device="cuda")
        ws[ws_bytes:] = tail
        torch.cuda.synchronize()
        lib.sourmash_err_clear()
        got = lib.smgpu_setops_merge_raw(d_h.data_ptr(), d_off.data_ptr(), n, total, d_g.data_ptr(), n_groups, d_need.data_ptr() if d_need is not None else None,
                                         need_all, max_hash, 0, out.data_ptr(), out_off.data_ptr(), result.data_ptr(), ws.data_ptr(), ws_bytes, None)
        assert lib.sourmash_err_get_last_code() == 0
        torch.cuda.synchronize()
        h_out, h_off = out.cpu().numpy().view(np.uint64), out_off.cpu().numpy().view(np.uint64)
        want = sc.expected_merge(rows, groups, n_groups, min_rows)
        assert got == sum(len(w) for w in want) == h_off[n_groups] == result.cpu().numpy().view(np.uint64)[0]
        assert (h_out[got:] == MARK).all() and (h_off[n_groups + 1:] == MARK).all() and bool((ws[ws_bytes:] == tail).all())
        assert_rows_equal(sc.uncsr(h_out[:got], h_off[:n_groups + 1]), want, min_rows)
    # a group number outside the groups is refused before anything runs
    bad = dev(np.array(groups[:-1] + [n_groups], dtype=np.uint32), np.uint32)
    assert lib.smgpu_setops_merge_raw(d_h.data_ptr(), d_off.data_ptr(), n, total, bad.data_ptr(), n_groups, None, 0, max_hash, 0, out.data_ptr(),
                                      out_off.data_ptr(), result.data_ptr(), ws.data_ptr(), ws_bytes, None) == 2**64 - 1
    assert lib.sourmash_err_get_last_code() != 0
    lib.sourmash_err_clear()


# ---- downsample -----------------------------------------------------------------------------------------------------------------------
def test_downsample(sm):
    rng = np.random.default_rng(51)
    p = sc.pool(3000, 52)
    rows = [np.sort(rng.choice(p, size=k, replace=False)) for k in (0, 1, 300, 1000)]
    rows.append(p[p > sc.MAX_HASH_10000][:50].copy())                   # a row that 10x the scaled empties
    rows.append(sc.u64([sc.MAX_HASH_10000, sc.MAX_HASH_10000 + 1, sc.MAX_HASH_1000]))
    s = make_set(sm, rows, names=[f"r{i}" for i in range(len(rows))])
    same = s.downsample(1000)
    assert same.params == s.params and same.md5sums() == s.md5sums()
    assert_rows_equal(rows_of(same), rows)
    for scaled in (10000, 500_000):
        got = s.downsample(scaled)
        assert got.params == (21, "DNA", 42, scaled, 0)
        want = [s.minhash(r).downsample(scaled=scaled)._mins_array() for r in range(len(s))]
        assert_rows_equal(rows_of(got), want, scaled)
        assert [m["name"] for m in got.manifest] == [f"r{i}" for i in range(len(rows))]
        assert [m["scaled"] for m in got.manifest] == [m["scaled"] for m in make_set(sm, want, scaled=scaled).manifest]      # what a set of that scaled says
    assert len(rows_of(s.downsample(10000))[4]) == 0 and len(rows_of(s.downsample(10000))[5]) == 1
    assert sum(len(r) == 0 for r in rows_of(s.downsample(500_000))) >= 3
    with pytest.raises(ValueError) as want_err:
        s.minhash(2).downsample(scaled=100)
    with pytest.raises(ValueError) as got_err:
        s.downsample(100)
    assert str(got_err.value) == str(want_err.value)
    num = sm.MinHash(500, 21)
    num.add_many([1, 2, 3])
    with pytest.raises(ValueError) as want_err:
        num.downsample(scaled=1000)
    with pytest.raises(ValueError) as got_err:
        sm.SketchSet([num]).downsample(1000)
    assert str(got_err.value) == str(want_err.value)


# ---- composition ----------------------------------------------------------------------------------------------------------------------
def test_composition(sm, tmp_path):
    rng = np.random.default_rng(61)
    p = sc.pool(2500, 62)
    rows = [np.sort(rng.choice(p, size=k, replace=False)) for k in (400, 900, 0, 650, 1200, 30)]
    partners = [np.sort(rng.choice(p, size=k, replace=False)) for k in (500, 0, 100, 650, 1000, 2000)]
    a = make_set(sm, rows, names=[f"a{i}" for i in range(6)])
    b = make_set(sm, partners)
    assert a.subtract(b).intersect(b).total_hashes == 0
    one = b.merge()
    assert a.subtract(one).intersect(one).total_hashes == 0
    groups = [1, 0, 1, 2, 0, 2]
    left, right = a.merge(groups).downsample(10000), a.downsample(10000).merge(groups)
    assert_rows_equal(rows_of(left), rows_of(right))
    assert left.params == right.params == (21, "DNA", 42, 10000, 0) and left.md5sums() == right.md5sums()
    # a result is a full set: saved, loaded, searched
    result = a.subtract(b)
    path = str(tmp_path / "result.zip")
    result.save(path)
    back = sm.SketchSet.load(path)
    assert back.params == result.params and back.md5sums() == result.md5sums()
    assert_rows_equal(rows_of(back), rows_of(result))
    assert [m["name"] for m in back.manifest] == [m["name"] for m in result.manifest] == [f"a{i}" for i in range(6)]
    assert result.to_json() == back.to_json() and len(result.subset([1, 3])) == 2
    q, r, c = result.overlaps_many(a)
    want = np.array([[len(np.intersect1d(x, y)) for y in rows_of(result)] for x in rows])
    got = np.zeros_like(want)
    got[q, r] = c
    assert np.array_equal(got, want)
    common, _ = result.compare()
    assert common.shape == (6, 6) and [int(common[i, i]) for i in range(6)] == [int(x) for x in result.sizes]


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_mismatch_errors_are_count_commons(sm):
    base = dict(ksize=21, scaled=1000, seed=42)

    def mh_of(**kw):
        p = dict(base, **kw)
        protein = p.pop("is_protein", False)
        mh = sm.MinHash(0, p["ksize"], scaled=p["scaled"], seed=p["seed"], is_protein=protein)
        mh.add_many([5, 7, 11])
        return mh
    ref = mh_of()
    s = sm.SketchSet([ref, mh_of()])
    # one difference at a time, and all at once: the first in check_compatible's order (ksize, moltype, scaled, seed) is the one raised
    variants = [dict(ksize=31), dict(is_protein=True, ksize=21), dict(scaled=2000), dict(seed=43), dict(ksize=31, scaled=2000, seed=43),
                dict(scaled=2000, seed=43), dict(is_protein=True, ksize=21, scaled=2000, seed=43)]
    for kw in variants:
        other = mh_of(**kw)
        with pytest.raises(ValueError) as want:
            ref.count_common(other)
        for o in (other, sm.SketchSet([other]), sm.SketchSet([other, other])):
            for method in (s.subtract, s.intersect):
                with pytest.raises(ValueError) as got:
                    method(o)
                assert str(got.value) == str(want.value), kw
    with pytest.raises(ValueError):
        s.subtract(sm.SketchSet([ref, ref, ref]))                       # neither one row nor len(self)
    with pytest.raises(TypeError):
        s.subtract([5, 7])
    with pytest.raises(ValueError):
        s.merge([0])
    with pytest.raises(ValueError):
        s.merge([0, -1])
    # abundances of `other` are dropped
    ab = sm.MinHash(0, 21, scaled=1000, track_abundance=True)
    ab.set_abundances({5: 3, 11: 2})
    assert [r.tolist() for r in rows_of(s.subtract(ab))] == [[7], [7]] and [r.tolist() for r in rows_of(s.intersect(ab))] == [[5, 11], [5, 11]]
