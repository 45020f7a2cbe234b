"""GPU parity of abundance sets (SketchSet with an abundance column; csrc/setops.hip's value-moving filter and summing merge,
csrc/abund_set.hip, csrc/capi_abund_set.cpp): against the numpy / dict expectations of abund_set_cases.py, the loop over MinHash
objects, and the golden fixtures, at the smallest shapes at which the kernels can go wrong.  Everything is integer-exact.  Run with
-m gpu."""
import ctypes as C

import numpy as np
import pytest

import abund_set_cases as ac
import setops_cases as sc
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 8
MARK = 0x5a5a5a5a5a5a5a5a


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


def marked(n):
    import torch
    return torch.from_numpy(np.full(n, MARK, dtype=np.uint64).view(np.int64)).cuda()


def make_set(sm, rows, abunds=None, scaled=1000, num=0, ksize=21, names=None):
    "a SketchSet of these rows (and abundances), from device tensors: any hash value goes, 0 and 2^64 - 1 too"
    import torch
    flat, off = sc.csr(rows)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda() if len(a) else torch.zeros(0, dtype=torch.int64, device="cuda")
    return sm.SketchSet.from_csr(t(flat), torch.from_numpy(off.view(np.int64).copy()).cuda(), ksize=ksize, scaled=scaled, num=num, names=names,
                                 abunds=t(ac.flat(abunds)) if abunds is not None else None)


def columns_of(s):
    "the rows of an abundance set on the host, both columns, with sizes, total and manifest checked against them"
    assert s.track_abundance
    mhs = [s.minhash(r) for r in range(len(s))]
    assert all(mh.track_abundance for mh in mhs)
    rows = [mh._mins_array() for mh in mhs]
    abunds = [np.fromiter(mh.hashes.values(), dtype=np.uint64, count=len(mh)) for mh in mhs]
    assert [int(x) for x in s.sizes] == [len(r) for r in rows] and s.total_hashes == sum(len(r) for r in rows)
    assert [m["n_hashes"] for m in s.manifest] == [len(r) for r in rows] and all(m["with_abundance"] for m in s.manifest)
    return rows, abunds


def assert_rows_equal(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for r, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.uint64 and np.array_equal(a, np.asarray(b, dtype=np.uint64)), (what, r, len(a), len(b))


def assert_columns(got, want, what=""):
    assert_rows_equal(got[0], want[0], (what, "hashes"))
    assert_rows_equal(got[1], want[1], (what, "abundances"))


def abund_mh(sm, hashes, abunds, scaled=1000, ksize=21):
    mh = sm.MinHash(0, ksize, scaled=scaled, track_abundance=True)
    mh.set_abundances(dict(zip([int(h) for h in hashes], [int(a) for a in abunds])))
    return mh


# ---- the filter through the set: carry, take, range -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ac.KEPT_PATTERNS)
def test_filter_patterns_against_numpy(sm, geometry, pattern):
    rows = ac.filter_rows(geometry[2])
    assert [len(r) for r in rows[-2:]] == [65537, 131075]
    abunds = [ac.abund_of(r) for r in rows]
    for k, v in enumerate(ac.EDGE_ABUNDS):
        abunds[5][3 * k] = np.uint64(v)                                 # the carry is 64-bit
    one, partners = ac.pattern_other(rows, pattern)
    aset, fset = make_set(sm, rows, abunds), make_set(sm, rows)
    one_ab, partner_ab = ac.abund_of(one, salt=3), [ac.abund_of(q, salt=3) for q in partners]
    one_set, partner_set = make_set(sm, [one], [one_ab]), make_set(sm, partners, partner_ab)
    for other, other_set in ((one, one_set), (partners, partner_set)):
        for keep_present, op in ((0, aset.subtract), (1, aset.intersect)):
            assert_columns(columns_of(op(other_set)), ac.expected_carry(rows, abunds, other, keep_present), (pattern, keep_present))
    assert_columns(columns_of(fset.inflate(one_set)), ac.expected_take(rows, one, one_ab), "take, one row")
    assert_columns(columns_of(fset.inflate(abund_mh(sm, one, one_ab))), ac.expected_take(rows, one, one_ab), "take, one sketch")
    assert_columns(columns_of(fset.inflate(partner_set)), ac.expected_take(rows, partners, partner_ab), "take, row-wise")
    assert aset.track_abundance and not fset.track_abundance and not aset.subtract(one_set).flatten().track_abundance


def test_take_edges(sm, geometry):
    for k, rows, other, o_ab in ac.take_bucket_cases():
        got = make_set(sm, rows).inflate(make_set(sm, [other], [o_ab]))
        assert_columns(columns_of(got), ac.expected_take(rows, other, o_ab), f"bucket of {k}")
    for name, rows, other, o_ab in ac.take_edge_cases():               # scaled = 1: hash 0 and 2^64 - 1 are members
        got = make_set(sm, rows, scaled=1).inflate(make_set(sm, [other], [o_ab], scaled=1))
        assert_columns(columns_of(got), ac.expected_take(rows, other, o_ab), name)
    rows, partners, p_ab = ac.partner_take_case(geometry[1])          # a staged partner, and one read from global memory
    assert [len(q) for q in partners[:2]] == [geometry[1], geometry[1] + 1]
    got = make_set(sm, rows).inflate(make_set(sm, partners, p_ab))
    assert_columns(columns_of(got), ac.expected_take(rows, partners, p_ab), "partners")


def test_range_filter(sm):
    rows = sc.disjoint_rows(ac.ROW_LENGTHS + [1300], 57)
    abunds = ac.seeded_abunds(rows, 58)
    aset = make_set(sm, rows, abunds)
    for lo, hi in ((2, None), (2, 5), (5, 5), (6, 5), (2**32, None), (2**32 - 1, 2**32), (2**64 - 1, None), (1, 1)):
        assert_columns(columns_of(aset.filter_abund(lo, hi)), ac.expected_range(rows, abunds, lo, hi), (lo, hi))
    assert aset.filter_abund(6, 5).total_hashes == 0                    # min > max keeps nothing
    assert_columns(columns_of(aset.filter_abund()), (rows, abunds), "min=1")
    assert_columns(columns_of(aset.filter_abund(min_abundance=1, max_abundance=None)), (rows, abunds), "min=1, no max")
    with pytest.raises(ValueError, match="abundance"):
        make_set(sm, rows).filter_abund(2)


def raw_filter(rows, abunds, other, other_abunds, keep_present, mode, lo=0, hi=2**64 - 1, grid=0, capacity=None):
    "-> (total, (hash rows, abundance rows) or None, guards untouched) of smgpu_setops_filter_values_raw"
    import torch
    from sourmash_amd._lowlevel import lib
    flat, off = sc.csr(rows)
    n, total = len(rows), len(flat)
    d_h, d_off = dev(flat), dev(off)
    d_a = dev(ac.flat(abunds)) if abunds is not None else None
    d_oh = d_oa = d_ooff = None
    o_len = 0
    if isinstance(other, np.ndarray):
        d_oh, o_len = dev(other), len(other)
        d_oa = dev(other_abunds) if other_abunds is not None else None
    elif other is not None:
        o_flat, o_off = sc.csr(other)
        d_oh, d_ooff = dev(o_flat), dev(o_off)
        d_oa = dev(ac.flat(other_abunds)) if other_abunds is not None else None
    cap = total if capacity is None else capacity
    out, out_a, out_off = marked(cap + GUARD), marked(cap + GUARD), marked(n + 1 + GUARD)
    result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    ws_bytes = int(lib.smgpu_setops_filter_workspace_bytes(n, total, o_len))
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    tail = torch.full((64,), 0x5a, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = tail
    torch.cuda.synchronize()

    def ptr(t):
        return t.data_ptr() if t is not None else None
    lib.sourmash_err_clear()
    got = lib.smgpu_setops_filter_values_raw(ptr(d_h), ptr(d_a), ptr(d_off), n, total, ptr(d_oh), ptr(d_oa), ptr(d_ooff), o_len, keep_present, mode, lo, hi,
                                             grid, ptr(out), ptr(out_a), cap, ptr(out_off), ptr(result), ptr(ws), ws_bytes, None)
    assert lib.sourmash_err_get_last_code() == 0
    torch.cuda.synchronize()
    h_out, h_a, h_off = (x.cpu().numpy().view(np.uint64) for x in (out, out_a, out_off))
    guards_ok = bool((h_off[n + 1:] == MARK).all()) and bool((ws[ws_bytes:] == tail).all())
    assert h_off[n] == got
    if got > cap:
        return int(got), None, guards_ok and bool((h_out == MARK).all()) and bool((h_a == MARK).all())
    cols = sc.uncsr(h_out[:got], h_off[:n + 1]), sc.uncsr(h_a[:got], h_off[:n + 1])
    return int(got), cols, guards_ok and bool((h_out[got:] == MARK).all()) and bool((h_a[got:] == MARK).all())


def test_filter_raw_entry_grids_guards_and_capacity(sm, geometry):
    rows = ac.filter_rows(geometry[2])
    abunds = [ac.abund_of(r) for r in rows]
    one, partners = ac.pattern_other(rows, "alternating")
    one_ab, partner_ab = ac.abund_of(one, salt=3), [ac.abund_of(q, salt=3) for q in partners]
    runs = [("carry, one", (rows, abunds, one, None, 0, ac.VALUES_CARRY), ac.expected_carry(rows, abunds, one, 0)),
            ("carry, row-wise", (rows, abunds, partners, None, 1, ac.VALUES_CARRY), ac.expected_carry(rows, abunds, partners, 1)),
            ("take, one", (rows, None, one, one_ab, 1, ac.VALUES_TAKE), ac.expected_take(rows, one, one_ab)),
            ("take, row-wise", (rows, None, partners, partner_ab, 1, ac.VALUES_TAKE), ac.expected_take(rows, partners, partner_ab)),
            ("range", (rows, abunds, None, None, 1, ac.VALUES_RANGE, 2**18, 2**19), ac.expected_range(rows, abunds, 2**18, 2**19))]
    for name, args, want in runs:
        n_want = sum(len(w) for w in want[0])
        assert n_want > 0, name
        for grid in (0, 1, 3):                                          # one workgroup takes every item by ticket; three share them
            total, got, guards_ok = raw_filter(*args, grid=grid)
            assert guards_ok and total == n_want, (name, grid)
            assert_columns(got, want, (name, grid))
        total, got, guards_ok = raw_filter(*args, capacity=n_want - 1)  # a result that does not fit: the total and the offsets, nothing written
        assert guards_ok and got is None and total == n_want, name


# ---- the merge ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_rows", [1, 2, "all", 9])
def test_merge_sums_and_counts_against_numpy(sm, min_rows):
    for name, rows, groups, n_groups, max_hash in sc.merge_cases():
        scaled = 1 if max_hash == sc.U64_MAX else 1000
        abunds = ac.seeded_abunds(rows, 61)
        aset, fset = make_set(sm, rows, abunds, scaled=scaled), make_set(sm, rows, scaled=scaled)
        got = aset.merge(groups, min_rows=min_rows)
        assert len(got) == n_groups
        assert_columns(columns_of(got), ac.expected_merge_values(rows, abunds, groups, n_groups, min_rows), name)
        got = fset.merge(groups, min_rows=min_rows, count_rows=True)
        assert_columns(columns_of(got), ac.expected_merge_values(rows, None, groups, n_groups, min_rows, count_rows=True), name)
        with pytest.raises(ValueError, match="count_rows"):
            aset.merge(groups, min_rows=min_rows, count_rows=True)
    # a group of one row is that row, bit for bit, in both columns
    name, rows, groups, n_groups, max_hash = sc.merge_cases()[1]
    abunds = ac.seeded_abunds(rows, 61)
    h, a = columns_of(make_set(sm, rows, abunds).merge(groups))
    assert np.array_equal(h[4], rows[6]) and np.array_equal(a[4], abunds[6])


def test_merge_edges(sm):
    # the two sides of the key form at scaled = 1000: 512 groups pack into one key, 513 (an empty row in group 512) do not
    rows, groups, _ = sc.boundary_case(512)
    abunds = ac.seeded_abunds(rows, 62)
    rows513, abunds513, groups513 = rows + [sc.u64([])], abunds + [np.zeros(0, dtype=np.uint64)], groups + [512]
    for min_rows in (1, "all"):
        packed = make_set(sm, rows, abunds).merge(groups, min_rows=min_rows)
        wide = make_set(sm, rows513, abunds513).merge(groups513, min_rows=min_rows)
        assert (len(packed), len(wide)) == (512, 513)
        assert_columns(columns_of(packed), ac.expected_merge_values(rows, abunds, groups, 512, min_rows), ("packed", min_rows))
        assert_columns(columns_of(wide), ac.expected_merge_values(rows513, abunds513, groups513, 513, min_rows), ("wide", min_rows))
    rows, abunds = ac.run_length_case()                                 # runs that end on and cross the chunk borders of the run pass
    aset = make_set(sm, rows, abunds)
    for min_rows in (1, 2, 65, 257):
        assert_columns(columns_of(aset.merge(min_rows=min_rows)), ac.expected_merge_values(rows, abunds, None, 1, min_rows), min_rows)
    assert_columns(columns_of(make_set(sm, rows).merge(count_rows=True)), ac.expected_merge_values(rows, None, None, 1, 1, count_rows=True), "counts")
    assert columns_of(make_set(sm, rows).merge(count_rows=True))[1][0].tolist() == [1, 2, 64, 65, 256, 257]
    rows, abunds, groups, n_groups = ac.wrap_case()                     # addends on both sides of 2^32, a sum of exactly 2^64 - 1
    got = columns_of(make_set(sm, rows, abunds).merge(groups))
    assert_columns(got, ac.expected_merge_values(rows, abunds, groups, n_groups))
    assert got[1][0].tolist() == [2**32, 2**64 - 1, 2**64 - 1, 4]
    # count_rows against np.unique per group
    name, rows, groups, n_groups, _ = sc.merge_cases()[1]
    h, c = columns_of(make_set(sm, rows).merge(groups, count_rows=True))
    for g in range(n_groups):
        members = [rows[r] for r in range(len(rows)) if groups[r] == g]
        values, counts = np.unique(np.concatenate(members), return_counts=True) if members else (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64))
        assert np.array_equal(h[g], values.astype(np.uint64)) and np.array_equal(c[g], counts.astype(np.uint64))


def test_merge_of_an_abundance_num_set_against_the_object_loop(sm):
    pool = sc.pool(900, 41, sc.U64_MAX)
    rng = np.random.default_rng(42)
    rows = [np.sort(rng.choice(pool, size=k, replace=False))[:500] for k in (500, 500, 300, 100, 500, 20)]
    abunds = ac.seeded_abunds(rows, 63, edges=False)
    groups = [0, 0, 1, 1, 2, 3]
    mhs = []
    for row, ab in zip(rows, abunds):
        mh = sm.MinHash(500, 21, track_abundance=True)
        mh.set_abundances(dict(zip(row.tolist(), ab.tolist())))
        mhs.append(mh)
    aset = sm.SketchSet(mhs, track_abundance=True)
    assert aset.params[4] == 500
    got = columns_of(aset.merge(groups))
    assert_columns(got, ac.expected_merge_values(rows, abunds, groups, 4, 1, num=500), "num cut")
    for g in range(4):                                                  # MinHash.merge, one object at a time
        acc = None
        for r in range(len(rows)):
            if groups[r] == g:
                if acc is None:
                    acc = mhs[r].copy()
                else:
                    acc.merge(mhs[r])
        assert np.array_equal(got[0][g], acc._mins_array()) and got[1][g].tolist() == list(acc.hashes.values())


def test_merge_raw_entry(sm):
    import torch
    from sourmash_amd._lowlevel import lib
    name, rows, groups, n_groups, max_hash = sc.merge_cases()[1]
    abunds = ac.seeded_abunds(rows, 61)
    flat, off = sc.csr(rows)
    n, total = len(rows), len(flat)
    lead = np.arange(7, dtype=np.uint64)                                # the CSR inside a longer buffer: the offsets do not start at 0
    d_h, d_a, d_off, d_g = dev(np.concatenate([lead, flat])), dev(np.concatenate([lead, ac.flat(abunds)])), dev(off + np.uint64(7)), dev(groups, np.uint32)
    for mode, count_rows in ((ac.MERGE_SUM, False), (ac.MERGE_COUNT, True)):
        for need_all, min_rows in ((0, 1), (1, "all")):
            out, out_a, out_off = marked(total + GUARD), marked(total + GUARD), marked(n_groups + 1 + GUARD)
            result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
            ws_bytes = int(lib.smgpu_setops_merge_values_workspace_bytes(total, n_groups))
            ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
            tail = torch.full((64,), 0x5a, dtype=torch.uint8, device="cuda")
            ws[ws_bytes:] = tail
            torch.cuda.synchronize()
            lib.sourmash_err_clear()
            got = lib.smgpu_setops_merge_values_raw(d_h.data_ptr(), d_a.data_ptr(), d_off.data_ptr(), n, total, d_g.data_ptr(), n_groups, None, need_all, max_hash, 0,
                                                    mode, out.data_ptr(), out_a.data_ptr(), out_off.data_ptr(), result.data_ptr(), ws.data_ptr(), ws_bytes, None)
            assert lib.sourmash_err_get_last_code() == 0
            torch.cuda.synchronize()
            h_out, h_a, h_off = (x.cpu().numpy().view(np.uint64) for x in (out, out_a, out_off))
            want = ac.expected_merge_values(rows, None if count_rows else abunds, groups, n_groups, min_rows, count_rows=count_rows)
            assert got == sum(len(w) for w in want[0]) == h_off[n_groups]
            assert (h_out[got:] == MARK).all() and (h_a[got:] == MARK).all() and (h_off[n_groups + 1:] == MARK).all() and bool((ws[ws_bytes:] == tail).all())
            assert_columns((sc.uncsr(h_out[:got], h_off[:n_groups + 1]), sc.uncsr(h_a[:got], h_off[:n_groups + 1])), want, (mode, min_rows))


# ---- against the object loop and the golden pair ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_pair(sm):
    return [sm.load_one_signature_from_json(golden("pairs", f"track_abund_{n}.fa.sig")) for n in (47, 63)]


def test_golden_pair_merge_inflate_and_angular(sm, golden_pair):
    from sourmash_amd.compare import compare_all_pairs
    a, b = (s.minhash for s in golden_pair)
    assert a.track_abundance and b.track_abundance
    aset = sm.SketchSet([a, b], track_abundance=True)
    assert aset.track_abundance and all(m["with_abundance"] for m in aset.manifest)
    merged = aset.merge()
    want = a.to_mutable()
    want.merge(b)
    got = merged.minhash(0)
    assert got.track_abundance and got.hashes == want.hashes and len(got) > 0
    # inflate of the flat 47 by the abundance 63
    flat47 = sm.load_one_signature_from_json(golden("pairs", "47.fa.sig"), ksize=31).minhash
    assert not flat47.track_abundance and (b.ksize, b.scaled) == (flat47.ksize, flat47.scaled)
    want = flat47.inflate(b)
    for other in (b, sm.SketchSet([b], track_abundance=True)):
        got = sm.SketchSet([flat47]).inflate(other).minhash(0)
        assert got.hashes == want.hashes and len(got) > 0
    with pytest.raises(ValueError) as ref:
        a.inflate(b)
    with pytest.raises(ValueError) as ours:
        aset.inflate(b)
    assert str(ours.value) == str(ref.value)
    # the angular matrix: the same integer sums, the same host function
    assert np.array_equal(aset.compare_angular(), compare_all_pairs(golden_pair, ignore_abundance=False))
    with pytest.raises(ValueError, match="abundance"):
        aset.flatten().compare_angular()


def test_small_sets_against_the_object_loop(sm):
    rng = np.random.default_rng(71)
    pool = sc.pool(600, 72)
    rows = [np.sort(rng.choice(pool, size=k, replace=False)) for k in (0, 1, 40, 200, 257)]
    abunds = ac.seeded_abunds(rows, 73, edges=False)
    mhs = [abund_mh(sm, r, a) for r, a in zip(rows, abunds)]
    aset = sm.SketchSet(mhs, track_abundance=True)
    assert_columns(columns_of(aset), (rows, abunds))
    assert aset.abund_sums.tolist() == [mh.sum_abundances for mh in mhs]
    # sig filter's dictionary rule
    for lo, hi in ((2, None), (3, 20)):
        got = aset.filter_abund(lo, hi)
        for r, mh in enumerate(mhs):
            keep = {h: v for h, v in mh.hashes.items() if v >= lo and (hi is None or v <= hi)}
            assert got.minhash(r).hashes == keep
    # flat.inflate(ab), row by row and against one sketch
    fset = sm.SketchSet([mh.flatten() for mh in mhs])
    got = fset.inflate(aset.subset([4, 3, 2, 1, 0]))
    for r, mh in enumerate(mhs):
        assert got.minhash(r).hashes == mh.flatten().inflate(mhs[4 - r]).hashes
    got = fset.inflate(mhs[4])
    for r, mh in enumerate(mhs):
        assert got.minhash(r).hashes == mh.flatten().inflate(mhs[4]).hashes
    # the angular matrix of the set equals the object path's
    from sourmash_amd.compare import angular_matrix
    assert np.array_equal(aset.compare_angular(), angular_matrix(mhs))


# ---- records: one abundance sketch per record of a buffer or a file ------------------------------------------------------------------------
def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _records_buffer(records):
    import torch
    starts = np.zeros(len(records) + 1, dtype=np.int64)
    starts[1:] = np.cumsum([len(r) for r in records])
    buf = np.frombuffer("".join(records).encode(), dtype=np.uint8).copy()
    return torch.from_numpy(buf).cuda(), torch.from_numpy(starts).cuda()


def _dna_records(k):
    rng = np.random.default_rng(101)

    def dna(n):
        return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))
    x, y = dna(40), dna(40)
    return [x + "T" + x,                   # k-mers repeated on one strand
            y + _revcomp(y),               # k-mers beside their reverse complements: one canonical k-mer, counted twice
            "",                            # an empty record
            dna(k - 1),                    # a record shorter than k
            dna(80)]


def _assert_rows_are_the_objects(ss, want, what):
    assert ss.track_abundance and len(ss) == len(want) and all(m["with_abundance"] for m in ss.manifest), what
    for r, mh in enumerate(want):
        got = ss.minhash(r)
        assert got.track_abundance and got.hashes == mh.hashes, (what, r)
    assert ss.abund_sums.tolist() == [mh.sum_abundances for mh in want], what


def test_sketch_records_with_abundance_against_add_sequence(sm):
    k = 21
    records = _dna_records(k)
    assert sum(len(r) for r in records) < 400
    seq, starts = _records_buffer(records)
    want = []
    for rec in records:
        mh = sm.MinHash(0, k, scaled=1, track_abundance=True)
        if rec:
            mh.add_sequence(rec)
        want.append(mh)
    assert max(want[0].hashes.values()) == 2 and set(want[1].hashes.values()) == {2} and len(want[2]) == 0 == len(want[3]) and len(want[4]) == 60
    ss = sm.SketchSet.sketch_records(seq, starts, ksize=k, scaled=1, track_abundance=True)
    _assert_rows_are_the_objects(ss, want, "DNA")
    assert ss.params == (k, "DNA", 42, 1, 0)
    flat = sm.SketchSet.sketch_records(seq, starts, ksize=k, scaled=1)      # the default stays flat, with the same hashes
    assert not flat.track_abundance and not any(m["with_abundance"] for m in flat.manifest)
    assert [flat.minhash(r)._mins_array().tolist() for r in range(len(flat))] == [sorted(mh.hashes) for mh in want]


def test_sketch_records_with_abundance_protein_and_translated(sm):
    rng = np.random.default_rng(102)
    k = 7

    def protein(n):
        return "".join("ACDEFGHIKLMNPQRSTVWY"[i] for i in rng.integers(0, 20, size=n))
    p = protein(25)
    records = [p + "A" + p, "", protein(k - 1), protein(60)]                # a repeat, an empty record, one shorter than k
    seq, starts = _records_buffer(records)
    want = []
    for rec in records:
        mh = sm.MinHash(0, k, scaled=1, is_protein=True, track_abundance=True)
        if rec:
            mh.add_protein(rec)
        want.append(mh)
    assert max(want[0].hashes.values()) == 2 and len(want[1]) == 0 == len(want[2])
    ss = sm.SketchSet.sketch_records(seq, starts, ksize=k, scaled=1, moltype="protein", is_protein=True, track_abundance=True)
    _assert_rows_are_the_objects(ss, want, "protein")
    # translated: DNA records read in six frames
    x = "".join("ACGT"[i] for i in rng.integers(0, 4, size=45))
    records = [x + x, "", "ACGTAC", "".join("ACGT"[i] for i in rng.integers(0, 4, size=90))]
    seq, starts = _records_buffer(records)
    want = []
    for rec in records:
        mh = sm.MinHash(0, k, scaled=1, is_protein=True, track_abundance=True)
        if rec:
            mh.add_sequence(rec, True)
        want.append(mh)
    assert max(want[0].hashes.values()) >= 2 and len(want[1]) == 0 == len(want[2])
    ss = sm.SketchSet.sketch_records(seq, starts, ksize=k, scaled=1, moltype="protein", track_abundance=True)
    _assert_rows_are_the_objects(ss, want, "translated")


def test_sketch_file_with_abundance(sm, tmp_path):
    rng = np.random.default_rng(103)
    z = "".join("ACGT"[i] for i in rng.integers(0, 4, size=95))
    records = [r for r in _dna_records(21) if r] + [z + z]                  # (the last one repeats 90-mers too)
    path = str(tmp_path / "reads.fa")
    with open(path, "w") as f:
        for i, rec in enumerate(records):
            f.write(f">read{i} x\n{rec}\n")
    for k in (21, 90):                                                      # the one-pass path, and record by record (k > 88)
        want = []
        for rec in records:
            mh = sm.MinHash(0, k, scaled=1, track_abundance=True)
            mh.add_sequence(rec, True)
            want.append(mh)
        ss = sm.SketchSet.sketch_file(path, ksize=k, scaled=1, track_abundance=True)
        _assert_rows_are_the_objects(ss, want, k)
        assert max(want[-1].hashes.values()) == 2
        flat = sm.SketchSet.sketch_file(path, ksize=k, scaled=1)
        assert not flat.track_abundance and not any(m["with_abundance"] for m in flat.manifest)
        assert [m["name"] for m in ss.manifest] == [m["name"] for m in flat.manifest] and all(m["name"].startswith("read") for m in ss.manifest)
        assert all(m["filename"] == path for m in ss.manifest)


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def test_plumbing(sm, tmp_path):
    import torch
    out_path = str(tmp_path / "refused.sig")
    rng = np.random.default_rng(81)
    pool = sc.pool(3000, 82)
    rows = [np.sort(rng.choice(pool, size=k, replace=False)) for k in (0, 1, 300, 1000, 65)]
    abunds = ac.seeded_abunds(rows, 83)
    names = [f"r{i}" for i in range(len(rows))]
    aset = make_set(sm, rows, abunds, names=names)
    assert aset.track_abundance and [m["name"] for m in aset.manifest] == names and all(m["with_abundance"] for m in aset.manifest)
    assert_columns(columns_of(aset), (rows, abunds))
    with np.errstate(over="ignore"):
        assert aset.abund_sums.tolist() == [int(a.sum(dtype=np.uint64)) for a in abunds]
    sig = aset.signature(2)
    assert sig.name == "r2" and sig.minhash.track_abundance and sig.minhash.hashes == dict(zip(rows[2].tolist(), abunds[2].tolist()))
    pick = [3, 0, 3, 4]
    assert_columns(columns_of(aset.subset(pick)), ([rows[i] for i in pick], [abunds[i] for i in pick]), "subset")
    cut = aset.downsample(10000)
    keep = [r <= np.uint64(sc.MAX_HASH_10000) for r in rows]
    assert_columns(columns_of(cut), ([r[k] for r, k in zip(rows, keep)], [a[k] for a, k in zip(abunds, keep)]), "downsample")
    flat = aset.flatten()
    assert not flat.track_abundance and not any(m["with_abundance"] for m in flat.manifest) and [m["name"] for m in flat.manifest] == names
    assert [flat.minhash(r)._mins_array().tolist() for r in range(len(rows))] == [r.tolist() for r in rows]
    assert not flat.minhash(2).track_abundance and flat.md5sums() == aset.md5sums()
    # the borrowed pointer is the column
    from sourmash_amd._lowlevel import lib
    d_ab = C.c_void_p()
    lib.smgpu_sketchset_device_abunds(aset._get_objptr(), C.byref(d_ab))
    assert d_ab.value and lib.smgpu_sketchset_abund_max(aset._get_objptr()) == 2**64 - 1
    d_none = C.c_void_p()
    lib.smgpu_sketchset_device_abunds(flat._get_objptr(), C.byref(d_none))
    assert not d_none.value
    # a zero abundance is refused, with its first position
    bad = [a.copy() for a in abunds]
    bad[3][7] = 0
    bad[4][1] = 0
    with pytest.raises(Exception, match="abundance 0 at position 308 "):      # (row 3 starts at 0 + 1 + 300)
        make_set(sm, rows, bad)
    with pytest.raises(ValueError, match="as many as the hashes"):
        sm.SketchSet.from_csr(torch.zeros(3, dtype=torch.int64, device="cuda"), torch.tensor([0, 3], device="cuda"), ksize=21, scaled=1000,
                              abunds=torch.ones(2, dtype=torch.int64, device="cuda"))
    # the writers refuse, and name the ways out
    for write in (lambda: aset.to_json(), lambda: aset.save(out_path), lambda: sm.SketchSetWriter(out_path).add(aset)):
        with pytest.raises(Exception, match="abundance") as err:
            write()
        assert "flatten()" in str(err.value) and "signature(row)" in str(err.value)
    # the default keeps a flat set, of abundance sketches too; a flat sketch is refused by track_abundance=True
    mhs = [abund_mh(sm, rows[2], abunds[2]), abund_mh(sm, rows[4], abunds[4])]
    assert not sm.SketchSet(mhs).track_abundance
    with pytest.raises(Exception, match="abundance"):
        sm.SketchSet([mhs[0], mhs[1].flatten()], track_abundance=True)
    with pytest.raises(ValueError):
        sm.SketchSet([mhs[0], abund_mh(sm, rows[4], abunds[4], ksize=31)], track_abundance=True)


def test_hash_only_readers_see_the_flattened_set(sm):
    rng = np.random.default_rng(91)
    pool = sc.pool(1500, 92)
    rows = [np.sort(rng.choice(pool, size=k, replace=False)) for k in (200, 400, 300, 1, 0)]
    aset = make_set(sm, rows, ac.seeded_abunds(rows, 93))
    flat = aset.flatten()
    query = sm.MinHash(0, 21, scaled=1000)
    query.add_many(np.sort(rng.choice(pool, size=500, replace=False)).tolist())
    assert np.array_equal(aset.overlaps(query), flat.overlaps(query))
    (c1, j1), (c2, j2) = aset.compare(), flat.compare()
    assert np.array_equal(c1, c2) and np.array_equal(j1, j2)
    queries = make_set(sm, [np.sort(rng.choice(pool, size=k, replace=False)) for k in (600, 50)])
    assert aset.gather_many(queries) == flat.gather_many(queries)
    assert any(len(p) for p in aset.gather_many(queries))


def test_gather_stats_many_reads_the_resident_column(sm):
    from sourmash_amd.index import SketchSet
    genomes = [sm.load_one_signature_from_json(golden("gather-abund", f"genome-s{i}.fa.gz.sig"), ksize=21) for i in (10, 11, 12)]
    queries = [sm.load_one_signature_from_json(golden("gather-abund", f"reads-{n}.sig"), ksize=21) for n in ("s10-s11", "s10x10-s11")]
    mhs = [q.minhash for q in queries]
    assert all(mh.track_abundance for mh in mhs)
    assert genomes[0].minhash.scaled <= mhs[0].scaled
    db = SketchSet.load([golden("gather-abund", f"genome-s{i}.fa.gz.sig") for i in (10, 11, 12)], ksize=21).downsample(mhs[0].scaled)
    arrays = [np.fromiter(mh.hashes.values(), dtype=np.uint64, count=len(mh)) for mh in mhs]
    aq, fq = SketchSet(mhs, track_abundance=True), SketchSet([mh.flatten() for mh in mhs])
    for qs in (aq, fq):
        qs.set_names(["reads-a", "reads-b"], ["a.sig", "b.sig"])
    resident, by_array = db.gather_stats_many(aq), db.gather_stats_many(fq, abunds=arrays)
    assert resident.with_abundance and resident.rows() == by_array.rows() and [len(r) for r in resident.rows()] == [2, 2]
    for name in ("pick_rows", "isect", "weighted", "abund_offsets", "abund_values", "total_weighted"):
        assert np.array_equal(getattr(resident, name), getattr(by_array, name)), name
    assert db.gather_stats_many(aq, ignore_abundance=True).rows() == db.gather_stats_many(fq).rows()
    # LinearIndex.gather_results_many on the same signatures: the same rows, every column (the query set carries the queries' names)
    from sourmash_amd.index import LinearIndex
    want = LinearIndex(genomes).gather_results_many(queries, 0)
    named = SketchSet(mhs, track_abundance=True)
    named.set_names([q.name for q in queries], [q.filename for q in queries])
    got = db.gather_stats_many(named).rows()
    assert [len(q) for q in got] == [len(q) for q in want] == [2, 2]
    for q_got, q_want in zip(got, want):
        for r_got, r_want in zip(q_got, q_want):
            assert set(r_got) == set(r_want)
            assert r_got == r_want, {c: (r_got[c], r_want[c]) for c in r_want if r_got[c] != r_want[c]}
