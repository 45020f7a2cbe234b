"""CPU checks of the abundance forms of the set algebra on a SketchSet (csrc/setops.hip): the value rules of csrc/setops_core.hpp
compiled for the host and walked as the kernels walk them, against the expectations of abund_set_cases.py; the C interface; and the
argument errors, which need no device.  None of this needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abund_set_cases as ac
import setops_cases as sc
import sourmash_amd
from sourmash_amd._lowlevel import lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "native", "abund_set_core_emul.cpp")

PROTOTYPES = [
    "SmgpuSketchSet *smgpu_sketchset_new_abund(const SourmashKmerMinHash *const *mhs, uintptr_t n);",
    "SmgpuSketchSet *smgpu_sketchset_from_csr_abund(const uint64_t *d_hashes, const uint64_t *d_abunds, const uint64_t *d_offsets, uint64_t n, "
    "uint32_t ksize, uint32_t hash_function, uint64_t seed, uint64_t max_hash, uint64_t num, "
    "const char *const *names, const char *const *filenames);",
    "SmgpuSketchSet *smgpu_sketchset_sketch_records_abund(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, uint64_t n_records, "
    "uint32_t ksize, uint64_t seed, uint64_t scaled, uint32_t track_abundance);",
    "SmgpuSketchSet *smgpu_sketchset_sketch_file_abund(const char *path, uint32_t ksize, uint64_t seed, uint64_t scaled, uint32_t track_abundance);",
    "SmgpuSketchSet *smgpu_sketchset_sketch_residue_records_abund(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, const uint64_t *d_ends, "
    "uint64_t n_records, uint32_t ksize, uint32_t hash_function, int32_t translate, "
    "uint64_t seed, uint64_t scaled, uint32_t track_abundance);",
    "SmgpuSketchSet *smgpu_sketchset_sketch_residue_file_abund(const char *path, uint32_t ksize, uint32_t hash_function, int32_t translate, "
    "uint64_t seed, uint64_t scaled, uint32_t track_abundance);",
    "uint32_t smgpu_sketchset_track_abundance(const SmgpuSketchSet *set);",
    "uint64_t smgpu_sketchset_abund_max(const SmgpuSketchSet *set);",
    "void smgpu_sketchset_device_abunds(const SmgpuSketchSet *set, const uint64_t **d_abunds);",
    "void smgpu_sketchset_abund_sums(const SmgpuSketchSet *set, uint64_t *out);",
    "SmgpuSketchSet *smgpu_sketchset_flatten(const SmgpuSketchSet *set);",
    "SmgpuSketchSet *smgpu_sketchset_inflate(const SmgpuSketchSet *set, const SmgpuSketchSet *other);",
    "SmgpuSketchSet *smgpu_sketchset_inflate_sketch(const SmgpuSketchSet *set, const SourmashKmerMinHash *mh);",
    "SmgpuSketchSet *smgpu_sketchset_filter_abund(const SmgpuSketchSet *set, uint64_t min_abundance, uint64_t max_abundance);",
    "SmgpuSketchSet *smgpu_sketchset_merge_groups_values(const SmgpuSketchSet *set, const uint32_t *groups, uint64_t n_groups, const uint32_t *need, "
    "uint32_t need_all, const char *const *names, uint32_t count_rows);",
    "void smgpu_sketchset_compare_angular(const SmgpuSketchSet *set, double *sims_out);",
    "SmgpuGatherRows *smgpu_sketchset_gather_rows_many_resident(const SmgpuSketchSet *db, const SmgpuSketchSet *queries, const uint64_t *abunds, "
    "uint64_t threshold_hashes, uint32_t use_resident);",
    "uint64_t smgpu_setops_filter_values_raw(const uint64_t *d_hashes, const uint64_t *d_abunds, const uint64_t *d_offsets, uint64_t n, uint64_t total, "
    "const uint64_t *d_other_hashes, const uint64_t *d_other_abunds, const uint64_t *d_other_offsets, "
    "uint64_t other_len, uint32_t keep_present, uint32_t values, uint64_t range_lo, uint64_t range_hi, "
    "uint32_t grid, uint64_t *d_out_hashes, uint64_t *d_out_abunds, uint64_t capacity, "
    "uint64_t *d_out_offsets, uint64_t *d_result, void *d_workspace, uint64_t workspace_bytes, void *stream);",
    "uint64_t smgpu_setops_merge_values_workspace_bytes(uint64_t total, uint64_t n_groups);",
    "uint64_t smgpu_setops_merge_values_raw(const uint64_t *d_hashes, const uint64_t *d_abunds, const uint64_t *d_offsets, uint64_t n, uint64_t total, "
    "const uint32_t *d_groups, uint64_t n_groups, const uint32_t *d_need, uint32_t need_all, "
    "uint64_t max_hash, uint64_t num, uint32_t values, uint64_t *d_out_hashes, uint64_t *d_out_abunds, "
    "uint64_t *d_out_offsets, uint64_t *d_result, void *d_workspace, uint64_t workspace_bytes, void *stream);",
]


def _norm(s):
    return " ".join(s.replace("( ", "(").replace(" )", ")").split())


def test_prototypes_declared_and_exported():
    with open(os.path.join(ROOT, "include", "sourmash_amd.h")) as f:
        header = _norm(f.read())
    so = C.CDLL(os.path.join(ROOT, "sourmash_amd", "libsourmash_amd.so"))
    assert len(PROTOTYPES) == 20
    for p in PROTOTYPES:
        assert _norm(p) in header, p
        name = p.split("(")[0].split()[-1].lstrip("*")
        assert hasattr(so, name), name
        assert name in lib.functions, name                     # the binding parsed it
    for name in ("flatten", "inflate", "filter_abund", "compare_angular", "track_abundance", "abund_sums"):
        assert hasattr(sourmash_amd.SketchSet, name), name


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("abund_set_core") / "libabund_set_core_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so_path, SRC])
    so = C.CDLL(so_path)
    u64, u32, ptr = C.c_uint64, C.c_uint32, C.c_void_p
    so.emul_abund_not_found.restype = u64
    so.emul_abund_find.argtypes, so.emul_abund_find.restype = [ptr, u64, u64], u64
    so.emul_abund_in_range.argtypes, so.emul_abund_in_range.restype = [u64, u64, u64], u32
    so.emul_abund_payload.argtypes, so.emul_abund_payload.restype = [u64, u64], u64
    so.emul_abund_payload_group.argtypes, so.emul_abund_payload_group.restype = [u64], u64
    so.emul_abund_payload_pos.argtypes, so.emul_abund_payload_pos.restype = [u64], u64
    so.emul_abund_run_sum.argtypes, so.emul_abund_run_sum.restype = [ptr, u64, u64], u64
    so.emul_abund_modes.argtypes = [ptr]
    so.emul_abund_filter.argtypes = [ptr, ptr, ptr, u64, ptr, ptr, ptr, u64, u32, u32, u64, u64, ptr, ptr, ptr, ptr]
    so.emul_abund_filter.restype = u64
    so.emul_abund_merge.argtypes = [ptr, ptr, ptr, u64, ptr, u64, ptr, u32, u64, u64, u32, u32, ptr, ptr, ptr]
    so.emul_abund_merge.restype = u64
    return so


def p(a):
    return a.ctypes.data if a is not None else None


def assert_rows_equal(got, want, what=""):
    assert len(got) == len(want), what
    for r, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (what, r, len(a), len(b))
    return True


# ---- the small rules ------------------------------------------------------------------------------------------------------------------
def test_small_rules(emul):
    modes = np.zeros(7, dtype=np.uint32)
    emul.emul_abund_modes(modes.ctypes.data)
    assert modes.tolist() == [0, ac.VALUES_CARRY, ac.VALUES_TAKE, ac.VALUES_RANGE, 0, ac.MERGE_SUM, ac.MERGE_COUNT]
    none = emul.emul_abund_not_found()
    assert none == 2**64 - 1
    row = sc.u64([0, 5, 9, 2**64 - 1])
    assert [emul.emul_abund_find(row.ctypes.data, 4, x) for x in (0, 5, 9, 2**64 - 1)] == [0, 1, 2, 3]
    assert [emul.emul_abund_find(row.ctypes.data, 4, x) for x in (1, 6, 2**64 - 2)] == [none] * 3
    assert emul.emul_abund_find(row.ctypes.data, 0, 5) == none
    # the range: inclusive at both ends, lo > hi keeps nothing, no upper bound is 2^64 - 1
    assert [emul.emul_abund_in_range(a, 2, 4) for a in (1, 2, 3, 4, 5)] == [0, 1, 1, 1, 0]
    assert [emul.emul_abund_in_range(a, 4, 2) for a in (1, 2, 3, 4, 5)] == [0] * 5
    assert emul.emul_abund_in_range(2**64 - 1, 1, 2**64 - 1) == 1
    # the payload: both fields whole at their 32-bit limits
    for g, j in ((0, 0), (1, 0), (0, 1), (0xfffffffd, 0xfffffffd), (513, 123456)):
        pl = emul.emul_abund_payload(g, j)
        assert (emul.emul_abund_payload_group(pl), emul.emul_abund_payload_pos(pl)) == (g, j)
    # a run's sum from the inclusive scan: modulo 2^64, whatever wrapped in front of the run
    vals = [2**64 - 1, 5, 2**63, 2**63, 7, 1]
    scan = np.array([sum(vals[:i + 1]) % 2**64 for i in range(len(vals))], dtype=np.uint64)
    for start in range(len(vals)):
        for count in range(1, len(vals) - start + 1):
            assert emul.emul_abund_run_sum(scan.ctypes.data, start, count) == sum(vals[start:start + count]) % 2**64


# ---- the filter -----------------------------------------------------------------------------------------------------------------------
def run_filter(emul, rows, abunds, other, other_abunds, keep_present, mode, lo=0, hi=2**64 - 1):
    flat, off = sc.csr(rows)
    flat = np.append(flat, np.uint64(0))
    ab = np.append(ac.flat(abunds), np.uint64(0)) if abunds is not None else None
    o_flat = o_ab = o_off = None
    o_len = 0
    if isinstance(other, np.ndarray):
        o_flat, o_len = np.append(other, np.uint64(0)), len(other)
        o_ab = np.append(other_abunds, np.uint64(0)) if other_abunds is not None else None
    elif other is not None:
        o_flat, o_off = sc.csr(other)
        o_flat = np.append(o_flat, np.uint64(0))
        o_ab = np.append(ac.flat(other_abunds), np.uint64(0)) if other_abunds is not None else None
    out = np.full(len(flat) + 2, 0xdeadbeef, dtype=np.uint64)
    out_ab = np.full(len(flat) + 2, 0xdeadbeef, dtype=np.uint64)
    out_off = np.full(len(rows) + 2, 0xdeadbeef, dtype=np.uint64)
    stats = np.zeros(6, dtype=np.uint64)
    total = emul.emul_abund_filter(p(flat), p(ab), p(off), len(rows), p(o_flat), p(o_ab), p(o_off), o_len, int(keep_present), mode, lo, hi,
                                   p(out), p(out_ab), p(out_off), p(stats))
    assert out_off[len(rows)] == total and out_off[len(rows) + 1] == 0xdeadbeef
    assert (out[total:] == 0xdeadbeef).all() and (out_ab[total:] == 0xdeadbeef).all()
    assert stats[1] == 0, "a lookup was made for a hash above the other sketch's largest, or in an empty sketch"
    assert stats[2] == 0 and stats[3] == 0
    if mode == ac.VALUES_TAKE:
        assert stats[5] == total                                        # one read of the other's abundances per kept hash
    return sc.uncsr(out[:total], out_off[:len(rows) + 1]), sc.uncsr(out_ab[:total], out_off[:len(rows) + 1]), stats


@pytest.mark.parametrize("pattern", ac.KEPT_PATTERNS)
def test_emulated_filter_patterns(emul, pattern):
    split = 65536
    rows = ac.filter_rows(split)
    abunds = [ac.abund_of(r) for r in rows]
    for k, v in enumerate(ac.EDGE_ABUNDS):
        abunds[5][3 * k] = np.uint64(v)
    one, partners = ac.pattern_other(rows, pattern)
    for other in (one, partners):
        for keep_present in (0, 1):
            got_h, got_a, stats = run_filter(emul, rows, abunds, other, None, keep_present, ac.VALUES_CARRY)
            want_h, want_a = ac.expected_carry(rows, abunds, other, keep_present)
            assert_rows_equal(got_h, want_h, "carry hashes")
            assert_rows_equal(got_a, want_a, "carry abundances")
            assert stats[4] == len(rows) + 1 + 2                          # two and three work items for the long rows
        o_ab = ac.abund_of(other, salt=3) if isinstance(other, np.ndarray) else [ac.abund_of(q, salt=3) for q in other]
        got_h, got_a, _ = run_filter(emul, rows, None, other, o_ab, 1, ac.VALUES_TAKE)
        want_h, want_a = ac.expected_take(rows, other, o_ab)
        assert_rows_equal(got_h, want_h, "take hashes")
        assert_rows_equal(got_a, want_a, "take abundances")


def test_emulated_take_edges(emul):
    for k, rows, other, o_ab in ac.take_bucket_cases():
        got_h, got_a, _ = run_filter(emul, rows, None, other, o_ab, 1, ac.VALUES_TAKE)
        want_h, want_a = ac.expected_take(rows, other, o_ab)
        assert_rows_equal(got_h, want_h, f"bucket of {k}")
        assert_rows_equal(got_a, want_a, f"bucket of {k}")
    for name, rows, other, o_ab in ac.take_edge_cases():
        got_h, got_a, stats = run_filter(emul, rows, None, other, o_ab, 1, ac.VALUES_TAKE)
        want_h, want_a = ac.expected_take(rows, other, o_ab)
        assert_rows_equal(got_h, want_h, name)
        assert_rows_equal(got_a, want_a, name)
        if name == "empty other":
            assert stats[0] == 0 and sum(len(r) for r in got_h) == 0
    rows, partners, p_ab = ac.partner_take_case(6144)
    got_h, got_a, _ = run_filter(emul, rows, None, partners, p_ab, 1, ac.VALUES_TAKE)
    want_h, want_a = ac.expected_take(rows, partners, p_ab)
    assert_rows_equal(got_h, want_h, "partners")
    assert_rows_equal(got_a, want_a, "partners")


def test_emulated_range_filter(emul):
    rows = sc.disjoint_rows(ac.ROW_LENGTHS + [1300], 57)
    abunds = ac.seeded_abunds(rows, 58)
    for lo, hi in ((1, None), (2, None), (2, 5), (5, 5), (6, 5), (2**32, None), (2**32 - 1, 2**32), (2**64 - 1, None), (1, 1)):
        got_h, got_a, stats = run_filter(emul, rows, abunds, None, None, 1, ac.VALUES_RANGE, lo, 2**64 - 1 if hi is None else hi)
        want_h, want_a = ac.expected_range(rows, abunds, lo, hi)
        assert_rows_equal(got_h, want_h, (lo, hi))
        assert_rows_equal(got_a, want_a, (lo, hi))
        assert stats[0] == 0                                            # no other sketch, no lookup
        if (lo, hi) == (1, None):
            assert_rows_equal(got_h, rows) and assert_rows_equal(got_a, abunds)
        if (lo, hi) == (6, 5):
            assert sum(len(r) for r in got_h) == 0


# ---- the merge ------------------------------------------------------------------------------------------------------------------------
def run_merge(emul, rows, abunds, groups, n_groups, max_hash, min_rows=1, num=0, mode=ac.MERGE_SUM, force_form=0):
    flat, off = sc.csr(rows)
    flat = np.append(flat, np.uint64(0))
    ab = np.append(ac.flat(abunds), np.uint64(0)) if abunds is not None else None
    g = np.ascontiguousarray(groups, dtype=np.uint32) if groups is not None else None
    if min_rows == "all":
        need, need_all = None, 1
    else:
        need, need_all = (None if min_rows == 1 else np.full(max(n_groups, 1), min_rows, dtype=np.uint32)), 0
    out = np.full(len(flat) + 2, 0xdeadbeef, dtype=np.uint64)
    out_ab = np.full(len(flat) + 2, 0xdeadbeef, dtype=np.uint64)
    out_off = np.full(n_groups + 2, 0xdeadbeef, dtype=np.uint64)
    total = emul.emul_abund_merge(p(flat), p(ab), p(off), len(rows), p(g) if g is not None and len(g) else None, n_groups, p(need), need_all, max_hash, num,
                                  mode, force_form, p(out), p(out_ab), p(out_off))
    assert out_off[n_groups] == total and out_off[n_groups + 1] == 0xdeadbeef
    return sc.uncsr(out[:total], out_off[:n_groups + 1]), sc.uncsr(out_ab[:total], out_off[:n_groups + 1])


@pytest.mark.parametrize("min_rows", [1, 2, "all", 9])
def test_emulated_merge_sums_and_counts(emul, min_rows):
    for name, rows, groups, n_groups, max_hash in sc.merge_cases():
        abunds = ac.seeded_abunds(rows, 61)
        want_h, want_a = ac.expected_merge_values(rows, abunds, groups, n_groups, min_rows)
        assert_rows_equal(want_h, sc.expected_merge(rows, groups, n_groups, min_rows), name)
        for force in (0, 2):
            got_h, got_a = run_merge(emul, rows, abunds, groups, n_groups, max_hash, min_rows, force_form=force)
            assert_rows_equal(got_h, want_h, (name, force))
            assert_rows_equal(got_a, want_a, (name, force))
        want_h, want_c = ac.expected_merge_values(rows, None, groups, n_groups, min_rows, count_rows=True)
        got_h, got_c = run_merge(emul, rows, None, groups, n_groups, max_hash, min_rows, mode=ac.MERGE_COUNT)
        assert_rows_equal(got_h, want_h, name)
        assert_rows_equal(got_c, want_c, name)
    # a group of one row is that row, in both columns
    name, rows, groups, n_groups, max_hash = sc.merge_cases()[1]
    abunds = ac.seeded_abunds(rows, 61)
    got_h, got_a = run_merge(emul, rows, abunds, groups, n_groups, max_hash)
    assert np.array_equal(got_h[4], rows[6]) and np.array_equal(got_a[4], abunds[6])


def test_emulated_merge_edges(emul):
    for n_groups in (512, 513):                                         # the two sides of the key form at scaled = 1000
        rows, groups, _ = sc.boundary_case(n_groups)
        abunds = ac.seeded_abunds(rows, 62)
        for min_rows in (1, "all"):
            got = run_merge(emul, rows, abunds, groups, n_groups, sc.MAX_HASH_1000, min_rows)
            want = ac.expected_merge_values(rows, abunds, groups, n_groups, min_rows)
            assert_rows_equal(got[0], want[0], n_groups)
            assert_rows_equal(got[1], want[1], n_groups)
    rows, abunds = ac.run_length_case()
    for min_rows in (1, 2, 65, 257):
        for force in (0, 2):
            got = run_merge(emul, rows, abunds, None, 1, sc.MAX_HASH_1000, min_rows, force_form=force)
            want = ac.expected_merge_values(rows, abunds, None, 1, min_rows)
            assert_rows_equal(got[0], want[0]) and assert_rows_equal(got[1], want[1])
    rows, abunds, groups, n_groups = ac.wrap_case()
    got = run_merge(emul, rows, abunds, groups, n_groups, sc.MAX_HASH_1000)
    want = ac.expected_merge_values(rows, abunds, groups, n_groups)
    assert_rows_equal(got[0], want[0]) and assert_rows_equal(got[1], want[1])
    assert want[1][0].tolist() == [2**32, 2**64 - 1, 2**64 - 1, 4]        # a sum of exactly 2^64 - 1, and one that wraps
    # the num cut in both columns
    pool = sc.pool(900, 41, sc.U64_MAX)
    rng = np.random.default_rng(42)
    rows = [np.sort(rng.choice(pool, size=k, replace=False))[:500] for k in (500, 500, 300, 100, 500, 20)]
    abunds = ac.seeded_abunds(rows, 63)
    got = run_merge(emul, rows, abunds, [0, 0, 1, 1, 2, 3], 4, 0, 1, num=500)
    want = ac.expected_merge_values(rows, abunds, [0, 0, 1, 1, 2, 3], 4, 1, num=500)
    assert_rows_equal(got[0], want[0]) and assert_rows_equal(got[1], want[1])


# ---- argument errors: raised without a device ------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    import torch
    from sourmash_amd.index import _abund_range, _check_count_rows, _check_csr_abunds, _check_inflate, _need_abundance_set
    with pytest.raises(ValueError, match="abundance"):
        _need_abundance_set(False, "filter_abund")                      # flat receiver for filter_abund
    _need_abundance_set(True, "filter_abund")
    mh = sourmash_amd.MinHash(0, 21, scaled=1000, track_abundance=True)
    flat_mh = sourmash_amd.MinHash(0, 21, scaled=1000)
    with pytest.raises(ValueError) as want:
        mh.inflate(mh)
    for receiver, other in ((True, True), (True, False), (False, False)):  # abundance receiver for inflate: the reference's words
        with pytest.raises(ValueError) as got:
            _check_inflate(receiver, other)
        assert str(got.value) == str(want.value)
    _check_inflate(False, True)
    with pytest.raises(ValueError, match="count_rows"):
        _check_count_rows(True, True)                                   # count_rows on an abundance set
    _check_count_rows(True, False)
    _check_count_rows(False, True)
    hashes = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="as many as the hashes"):
        _check_csr_abunds(torch.ones(4, dtype=torch.int64), hashes)     # wrong length
    for bad in (torch.ones(5, dtype=torch.float64), torch.ones(5, dtype=torch.int32)):
        with pytest.raises(ValueError, match="64-bit integers"):
            _check_csr_abunds(bad, hashes)                              # wrong dtype
    _check_csr_abunds(None, hashes)
    assert _abund_range(1, None) == (1, 2**64 - 1) and _abund_range(3, 2) == (3, 2)
    with pytest.raises(ValueError):
        _abund_range(-1, None)
    assert flat_mh.track_abundance is False


def test_raw_entries_refuse_bad_arguments_before_the_device():
    from sourmash_amd._lowlevel import decode_str
    buf = np.zeros(64, dtype=np.uint64)
    q = buf.ctypes.data
    ws = lib.smgpu_setops_merge_values_workspace_bytes(1, 1)
    assert ws > lib.smgpu_setops_merge_workspace_bytes(1, 1)
    fws = lib.smgpu_setops_filter_workspace_bytes(1, 1, 1)
    calls = [
        lambda: lib.smgpu_setops_merge_values_raw(q, q, q, 1, 1, None, 1, None, 0, 0, 0, 3, q, q, q, q, q, ws, None),         # unknown mode
        lambda: lib.smgpu_setops_merge_values_raw(q, None, q, 1, 1, None, 1, None, 0, 0, 0, 1, q, q, q, q, q, ws, None),      # sum without abundances
        lambda: lib.smgpu_setops_merge_values_raw(q, q, q, 1, 1, None, 1, None, 0, 0, 0, 1, q, None, q, q, q, ws, None),      # no room for values
        lambda: lib.smgpu_setops_merge_values_raw(q, q, q, 1, 1, None, 1, None, 0, 0, 0, 1, q, q, q, q, q, ws - 256, None),   # the flat workspace
        lambda: lib.smgpu_setops_filter_values_raw(q, q, q, 1, 1, q, q, None, 1, 1, 4, 0, 0, 0, q, q, 1, q, q, q, fws, None),  # unknown mode
        lambda: lib.smgpu_setops_filter_values_raw(q, None, q, 1, 1, q, None, None, 1, 1, 1, 0, 0, 0, q, q, 1, q, q, q, fws, None),  # carry without abundances
        lambda: lib.smgpu_setops_filter_values_raw(q, None, q, 1, 1, q, None, None, 1, 1, 2, 0, 0, 0, q, q, 1, q, q, q, fws, None),  # take without the other's
        lambda: lib.smgpu_setops_filter_values_raw(q, None, q, 1, 1, q, q, None, 1, 0, 2, 0, 0, 0, q, q, 1, q, q, q, fws, None),     # take that subtracts
        lambda: lib.smgpu_setops_filter_values_raw(q, q, q, 1, 1, q, None, None, 1, 1, 3, 1, 2, 0, q, q, 1, q, q, q, fws, None),     # range with another sketch
        lambda: lib.smgpu_setops_filter_values_raw(q, q, q, 1, 1, None, None, None, 0, 1, 3, 1, 2, 0, q, None, 1, q, q, q, fws, None),  # no room for values
    ]
    for i, call in enumerate(calls):
        lib.sourmash_err_clear()
        assert call() == 2**64 - 1 and lib.sourmash_err_get_last_code() != 0, i
        assert "no HIP device" not in decode_str(lib.sourmash_err_get_last_message()), i
    lib.sourmash_err_clear()
