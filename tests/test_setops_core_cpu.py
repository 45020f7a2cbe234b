"""CPU checks of the set algebra on a SketchSet (csrc/setops.hip): its rules (csrc/setops_core.hpp) compiled for the host and walked as
the kernels walk them, against numpy on every case of setops_cases.py; the C interface; and the argument errors, which need no device.
None of this needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import setops_cases as sc
import sourmash_amd
from sourmash_amd._lowlevel import lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "native", "setops_core_emul.cpp")

PROTOTYPES = [
    "void smgpu_setops_geometry(uint32_t *workgroup, uint32_t *lds_partner, uint64_t *split);",
    "void smgpu_setops_key_form(uint64_t max_hash, uint64_t n_groups, uint32_t *hbits, uint32_t *gbits, uint32_t *packed);",
    "uint64_t smgpu_setops_merge_workspace_bytes(uint64_t total, uint64_t n_groups);",
    "uint64_t smgpu_setops_merge_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n, uint64_t total, const uint32_t *d_groups, "
    "uint64_t n_groups, const uint32_t *d_need, uint32_t need_all, uint64_t max_hash, uint64_t num, "
    "uint64_t *d_out_hashes, uint64_t *d_out_offsets, uint64_t *d_result, void *d_workspace, "
    "uint64_t workspace_bytes, void *stream);",
    "uint64_t smgpu_setops_filter_workspace_bytes(uint64_t n, uint64_t total, uint64_t other_len);",
    "uint64_t smgpu_setops_filter_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n, uint64_t total, "
    "const uint64_t *d_other_hashes, const uint64_t *d_other_offsets, uint64_t other_len, "
    "uint32_t keep_present, uint32_t grid, uint64_t *d_out_hashes, uint64_t capacity, "
    "uint64_t *d_out_offsets, uint64_t *d_result, void *d_workspace, uint64_t workspace_bytes, void *stream);",
    "SmgpuSketchSet *smgpu_sketchset_merge_groups(const SmgpuSketchSet *set, const uint32_t *groups, uint64_t n_groups, const uint32_t *need, "
    "uint32_t need_all, const char *const *names);",
    "SmgpuSketchSet *smgpu_sketchset_filter(const SmgpuSketchSet *set, const SmgpuSketchSet *other, uint32_t keep_present);",
    "SmgpuSketchSet *smgpu_sketchset_filter_sketch(const SmgpuSketchSet *set, const SourmashKmerMinHash *mh, uint32_t keep_present);",
    "SmgpuSketchSet *smgpu_sketchset_downsample(const SmgpuSketchSet *set, uint64_t max_hash);",
]


def _norm(s):
    return " ".join(s.replace("( ", "(").replace(" )", ")").split())


def test_prototypes_declared_and_exported():
    with open(os.path.join(ROOT, "include", "sourmash_amd.h")) as f:
        header = _norm(f.read())
    so = C.CDLL(os.path.join(ROOT, "sourmash_amd", "libsourmash_amd.so"))
    assert len(PROTOTYPES) == 10
    for p in PROTOTYPES:
        assert _norm(p) in header, p
        name = p.split("(")[0].split()[-1].lstrip("*")
        assert hasattr(so, name), name
        assert name in lib.functions, name                     # the binding parsed it
    for name in ("merge", "subtract", "intersect", "downsample"):
        assert callable(getattr(sourmash_amd.SketchSet, name))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("setops_core") / "libsetops_core_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so_path, SRC])
    so = C.CDLL(so_path)
    so.emul_setops_split.restype = C.c_uint64
    so.emul_setops_bits.argtypes = [C.c_uint64]
    so.emul_setops_bits.restype = C.c_uint32
    so.emul_setops_pieces.argtypes = [C.c_uint64]
    so.emul_setops_pieces.restype = C.c_uint64
    so.emul_setops_num_cut.argtypes = [C.c_uint64, C.c_uint64]
    so.emul_setops_num_cut.restype = C.c_uint64
    so.emul_setops_row_of.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    so.emul_setops_row_of.restype = C.c_uint64
    so.emul_setops_key_form.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    so.emul_setops_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32,
                                     C.c_void_p, C.c_void_p]
    so.emul_setops_merge.restype = C.c_uint64
    so.emul_setops_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    so.emul_setops_filter.restype = C.c_uint64
    return so


def key_form(emul, max_hash, n_groups):
    out = np.zeros(3, dtype=np.uint32)
    emul.emul_setops_key_form(max_hash, n_groups, out.ctypes.data)
    return int(out[0]), int(out[1]), bool(out[2])


def test_geometry_is_the_headers(emul):
    wg, lds, split = C.c_uint32(), C.c_uint32(), C.c_uint64()
    lib.smgpu_setops_geometry(C.byref(wg), C.byref(lds), C.byref(split))
    assert (wg.value, lds.value, split.value) == (emul.emul_setops_block(), emul.emul_setops_lds_partner(), emul.emul_setops_split())
    assert wg.value == 256 and wg.value % 64 == 0
    assert split.value % wg.value == 0 and split.value > 1300          # the filter's length cases stay whole rows
    # three workgroups' staged partners fit a CU's 160 KiB of LDS; one fits the 64 KiB a workgroup can have
    assert 8 * lds.value + 64 <= 64 * 1024 and 3 * (8 * lds.value + 64) <= 160 * 1024


# ---- the key form -----------------------------------------------------------------------------------------------------------------
def test_bits(emul):
    for x, want in ((0, 0), (1, 1), (2, 2), (3, 2), (255, 8), (256, 9), (2**63 - 1, 63), (2**63, 64), (sc.U64_MAX, 64), (sc.MAX_HASH_1000, 55)):
        assert emul.emul_setops_bits(x) == want == int(x).bit_length()


def test_key_form_on_both_sides_of_64_bits(emul):
    # scaled = 1000: 55 hash bits, so 9 group bits pack and 10 do not: 512 groups against 513
    assert key_form(emul, sc.MAX_HASH_1000, 1) == (55, 1, True)          # at least one group bit
    assert key_form(emul, sc.MAX_HASH_1000, 2) == (55, 1, True)
    assert key_form(emul, sc.MAX_HASH_1000, 3) == (55, 2, True)
    assert key_form(emul, sc.MAX_HASH_1000, 512) == (55, 9, True)
    assert key_form(emul, sc.MAX_HASH_1000, 513) == (55, 10, False)
    # every max_hash: packed exactly when the bits of max_hash and of G - 1 fit 64
    for hbits in range(1, 65):
        max_hash = (1 << hbits) - 1
        for gbits in range(1, 33):
            for n_groups in ((1 << (gbits - 1)) + 1, 1 << gbits):
                if gbits == 1 and n_groups > 2:
                    continue
                h, g, packed = key_form(emul, max_hash, n_groups)
                assert (h, g) == (hbits, max(1, (n_groups - 1).bit_length())), (hbits, n_groups)
                assert packed == (h + g <= 64), (hbits, n_groups)
    # scaled = 1 (max_hash = 2^64 - 1) and num sets (max_hash = 0) have 64 hash bits: wide for any G, G = 1 included
    for max_hash in (sc.U64_MAX, 0):
        for n_groups in (1, 2, 3, 1000):
            h, g, packed = key_form(emul, max_hash, n_groups)
            assert h == 64 and not packed
    # the library says the same
    for max_hash, n_groups in ((sc.MAX_HASH_1000, 512), (sc.MAX_HASH_1000, 513), (0, 2), (sc.U64_MAX, 1), (sc.MAX_HASH_10000, 4096)):
        h, g, p = C.c_uint32(), C.c_uint32(), C.c_uint32()
        lib.smgpu_setops_key_form(max_hash, n_groups, C.byref(h), C.byref(g), C.byref(p))
        assert (h.value, g.value, bool(p.value)) == key_form(emul, max_hash, n_groups)


def test_small_rules(emul):
    split = emul.emul_setops_split()
    for length, want in ((0, 1), (1, 1), (split, 1), (split + 1, 2), (2 * split, 2), (2 * split + 1, 3), (10**7, -(-10**7 // split))):
        assert emul.emul_setops_pieces(length) == want
        assert want <= 1 + length // split                         # the bound the workspace is sized by
    assert [emul.emul_setops_num_cut(n, 500) for n in (0, 499, 500, 501)] == [0, 499, 500, 500]
    assert emul.emul_setops_num_cut(10**6, 0) == 10**6
    off = np.array([0, 0, 3, 3, 3, 7, 8], dtype=np.uint64)              # rows 0, 2, 3 are empty
    assert [emul.emul_setops_row_of(off.ctypes.data, 6, i) for i in range(8)] == [1, 1, 1, 4, 4, 4, 4, 5]
    off = off + np.uint64(100)                                          # a CSR that starts inside a larger buffer
    assert [emul.emul_setops_row_of(off.ctypes.data, 6, 100 + i) for i in range(8)] == [1, 1, 1, 4, 4, 4, 4, 5]


# ---- the merge ----------------------------------------------------------------------------------------------------------------------
def run_merge(emul, rows, groups, n_groups, max_hash, min_rows=1, num=0, force_form=0):
    flat, off = sc.csr(rows)
    flat = np.append(flat, np.uint64(0))
    g = np.ascontiguousarray(groups, dtype=np.uint32) if groups is not None else None
    if min_rows == "all":
        need, need_all = None, 1
    else:
        need, need_all = (None if min_rows == 1 else np.full(max(n_groups, 1), min_rows, dtype=np.uint32)), 0
    out = np.full(len(flat) + 2, 0xdeadbeef, dtype=np.uint64)
    out_off = np.full(n_groups + 2, 0xdeadbeef, dtype=np.uint64)
    total = emul.emul_setops_merge(flat.ctypes.data, off.ctypes.data, len(rows), g.ctypes.data if g is not None and len(g) else None, n_groups,
                                   need.ctypes.data if need is not None else None, need_all, max_hash, num, force_form, out.ctypes.data, out_off.ctypes.data)
    assert out_off[n_groups] == total and out_off[n_groups + 1] == 0xdeadbeef
    return sc.uncsr(out[:total], out_off[:n_groups + 1])


def assert_rows_equal(got, want, what=""):
    assert len(got) == len(want), what
    for r, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (what, r, len(a), len(b))


@pytest.mark.parametrize("min_rows", [1, 2, "all", 9])
def test_emulated_merge_against_numpy(emul, min_rows):
    for name, rows, groups, n_groups, max_hash in sc.merge_cases():
        want = sc.expected_merge(rows, groups, n_groups, min_rows)
        assert_rows_equal(run_merge(emul, rows, groups, n_groups, max_hash, min_rows), want, name)
        assert_rows_equal(run_merge(emul, rows, groups, n_groups, max_hash, min_rows, force_form=2), want, name + " (wide)")
    # a group of one row is that row; one group of one row is the set
    name, rows, groups, n_groups, max_hash = sc.merge_cases()[1]
    assert np.array_equal(run_merge(emul, rows, groups, n_groups, max_hash)[4], rows[6])


def test_emulated_merge_on_both_sides_of_the_form_boundary(emul):
    packed_g = max(g for g in range(2, 2000) if key_form(emul, sc.MAX_HASH_1000, g)[2])
    assert packed_g == 512 and not key_form(emul, sc.MAX_HASH_1000, packed_g + 1)[2]
    results = []
    for n_groups in (packed_g, packed_g + 1):
        rows, groups, _ = sc.boundary_case(n_groups)
        for min_rows in (1, "all"):
            got = run_merge(emul, rows, groups, n_groups, sc.MAX_HASH_1000, min_rows)
            assert_rows_equal(got, sc.expected_merge(rows, groups, n_groups, min_rows), str(n_groups))
            results.append(got[:packed_g])
    assert_rows_equal(results[0], results[2])
    assert_rows_equal(results[1], results[3])


def test_emulated_num_cut(emul):
    p = sc.pool(900, 41, sc.U64_MAX)
    rng = np.random.default_rng(42)
    rows = [np.sort(rng.choice(p, size=k, replace=False))[:500] for k in (500, 500, 300, 100, 500, 20)]
    groups = [0, 0, 1, 1, 2, 3]                                          # unions longer than, shorter than and equal to num; one short row
    want = sc.expected_merge(rows, groups, 4, 1, num=500)
    assert [len(w) for w in want] == [500, len(np.union1d(rows[2], rows[3])), 500, 20] and len(np.union1d(rows[0], rows[1])) > 500
    assert_rows_equal(run_merge(emul, rows, groups, 4, 0, 1, num=500), want)


# ---- the filter ---------------------------------------------------------------------------------------------------------------------
def run_filter(emul, rows, other, keep_present):
    flat, off = sc.csr(rows)
    flat = np.append(flat, np.uint64(0))
    if isinstance(other, np.ndarray):
        o_flat, o_off, o_len = np.append(other, np.uint64(0)), None, len(other)
    else:
        o_flat, o_off = sc.csr(other)
        o_flat, o_len = np.append(o_flat, np.uint64(0)), 0
    out = np.full(len(flat) + 2, 0xdeadbeef, dtype=np.uint64)
    out_off = np.full(len(rows) + 2, 0xdeadbeef, dtype=np.uint64)
    stats = np.zeros(5, dtype=np.uint64)
    total = emul.emul_setops_filter(flat.ctypes.data, off.ctypes.data, len(rows), o_flat.ctypes.data, o_off.ctypes.data if o_off is not None else None, o_len,
                                    int(keep_present), out.ctypes.data, out_off.ctypes.data, stats.ctypes.data)
    assert out_off[len(rows)] == total and out_off[len(rows) + 1] == 0xdeadbeef and (out[total:] == 0xdeadbeef).all()
    assert stats[1] == 0, "a lookup was made for a hash above the other sketch's largest, or in an empty sketch"
    assert stats[2] == 0 and stats[3] == 0
    return sc.uncsr(out[:total], out_off[:len(rows) + 1]), stats


@pytest.mark.parametrize("keep_present", [0, 1])
@pytest.mark.parametrize("pattern", sc.pattern_names())
def test_emulated_filter_patterns_against_numpy(emul, pattern, keep_present):
    rows, one, partners = sc.filter_pattern_case(pattern, emul.emul_setops_split())
    got, stats = run_filter(emul, rows, one, keep_present)
    assert_rows_equal(got, sc.expected_filter(rows, one, keep_present), "one sketch")
    assert stats[4] == len(rows) + 1                                    # the long row is two work items
    got, _ = run_filter(emul, rows, partners, keep_present)
    assert_rows_equal(got, sc.expected_filter(rows, partners, keep_present), "row-wise")


@pytest.mark.parametrize("keep_present", [0, 1])
def test_emulated_filter_edges_against_numpy(emul, keep_present):
    for name, rows, other in sc.one_sketch_edge_cases():
        got, stats = run_filter(emul, rows, other, keep_present)
        assert_rows_equal(got, sc.expected_filter(rows, other, keep_present), name)
        if name in ("empty", "wholly below the smallest"):
            assert stats[0] == 0, name                                  # nothing is looked up at all
        if name == "wholly below the largest":
            assert 0 < stats[0] < 2 * sum(len(r) for r in rows)
    for k, rows, other in sc.bucket_cases():
        got, _ = run_filter(emul, rows, other, keep_present)
        assert_rows_equal(got, sc.expected_filter(rows, other, keep_present), f"bucket of {k}")
    rows, partners = sc.partner_cases(emul.emul_setops_lds_partner())
    got, _ = run_filter(emul, rows, partners, keep_present)
    assert_rows_equal(got, sc.expected_filter(rows, partners, keep_present), "partners")
    got, _ = run_filter(emul, [], sc.u64([5]), keep_present)
    assert got == []


# ---- argument errors: raised without a device ------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    from sourmash_amd.index import _check_downsample, _check_other_rows, _merge_plan
    with pytest.raises(ValueError, match="one group number per row"):
        _merge_plan(3, 0, [0, 1], 1, None)                              # wrong groups length
    with pytest.raises(ValueError, match="not negative"):
        _merge_plan(3, 0, [0, -1, 1], 1, None)
    with pytest.raises(ValueError, match="integers"):
        _merge_plan(2, 0, [0.5, 1.0], 1, None)
    with pytest.raises(ValueError, match="min_rows"):
        _merge_plan(2, 0, [0, 1], 0, None)
    with pytest.raises(ValueError, match="min_rows"):
        _merge_plan(2, 0, [0, 1], "most", None)
    with pytest.raises(ValueError, match="one name per group"):
        _merge_plan(2, 0, [0, 1], 1, ["a"])
    for min_rows in (2, "all"):                                          # min_rows on a num set
        with pytest.raises(ValueError, match="num set"):
            _merge_plan(2, 500, [0, 1], min_rows, None)
    g, n_groups, need, need_all, names = _merge_plan(4, 0, [3, 0, 0, 1], "all", ["a", "b", "c", "d"])
    assert g.dtype == np.uint32 and g.tolist() == [3, 0, 0, 1] and n_groups == 4 and need is None and need_all == 1 and len(names) == 4
    g, n_groups, need, need_all, names = _merge_plan(4, 500, None, 1, None)
    assert g is None and n_groups == 1 and need is None and need_all == 0 and names is None
    assert _merge_plan(2, 0, [0, 1], 3, None)[2].tolist() == [3, 3]
    assert _merge_plan(0, 0, [], 1, None)[1] == 0
    with pytest.raises(ValueError, match="3 rows"):
        _check_other_rows(5, 3)                                         # `other` of a wrong length
    _check_other_rows(5, 1)
    _check_other_rows(5, 5)
    # downsample: the errors of MinHash.downsample
    mh = sourmash_amd.MinHash(0, 21, scaled=1000)
    with pytest.raises(ValueError) as want:
        mh.downsample(scaled=100)
    with pytest.raises(ValueError) as got:
        _check_downsample((21, "DNA", 42, 1000, 0), 100)
    assert str(got.value) == str(want.value)
    num = sourmash_amd.MinHash(500, 21)
    with pytest.raises(ValueError) as want:
        num.downsample(scaled=100)
    with pytest.raises(ValueError) as got:
        _check_downsample((21, "DNA", 42, 0, 500), 100)
    assert str(got.value) == str(want.value)
    _check_downsample((21, "DNA", 42, 1000, 0), 1000)
    _check_downsample((21, "DNA", 42, 1000, 0), 10000)


def test_entry_points_raise_without_gpu():
    if sourmash_amd.gpu_available():
        pytest.skip("a GPU is present: the calls succeed (covered by tests/test_gpu_setops.py)")
    from sourmash_amd._lowlevel import decode_str
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    lib.sourmash_err_clear()
    ws = lib.smgpu_setops_merge_workspace_bytes(1, 1)
    assert ws > 0 and lib.sourmash_err_get_last_code() == 0
    assert lib.smgpu_setops_merge_raw(p, p, 1, 1, None, 1, None, 0, sc.MAX_HASH_1000, 0, p, p, p, p, ws, None) == 2**64 - 1
    assert lib.sourmash_err_get_last_code() != 0 and "no HIP device" in decode_str(lib.sourmash_err_get_last_message())
    lib.sourmash_err_clear()
    ws = lib.smgpu_setops_filter_workspace_bytes(1, 1, 1)
    assert lib.smgpu_setops_filter_raw(p, p, 1, 1, p, None, 1, 1, 0, p, 1, p, p, p, ws, None) == 2**64 - 1
    assert lib.sourmash_err_get_last_code() != 0 and "no HIP device" in decode_str(lib.sourmash_err_get_last_message())
    lib.sourmash_err_clear()


def test_raw_entries_refuse_bad_arguments_before_the_device():
    from sourmash_amd._lowlevel import decode_str
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    ws = lib.smgpu_setops_merge_workspace_bytes(1, 1)
    calls = [
        lambda: lib.smgpu_setops_merge_raw(p, p, 1, 1, None, 1, None, 0, 0, 0, p, p, p, p, 16, None),              # workspace too small
        lambda: lib.smgpu_setops_merge_raw(p, p, 1, 1, None, 1, None, 0, 0, 0, p, p, None, p, ws, None),           # no result
        lambda: lib.smgpu_setops_merge_raw(p, p, 1, 1, None, 0, None, 0, 0, 0, p, p, p, p, ws, None),              # rows without a group
        lambda: lib.smgpu_setops_merge_raw(p, p, 1, 1, None, 1, None, 1, 0, 500, p, p, p, p, ws, None),            # a num cut of an intersection
        lambda: lib.smgpu_setops_merge_raw(p, p, 1, 2**32, None, 1, None, 0, 0, 0, p, p, p, p, 2**40, None),       # 2^32 hashes
        lambda: lib.smgpu_setops_filter_raw(p, p, 1, 1, p, None, 1, 1, 0, p, 1, p, p, p, 16, None),
        lambda: lib.smgpu_setops_filter_raw(p, p, 1, 1, p, None, 1, 1, 2**21, p, 1, p, p, p, 2**30, None),         # grid
        lambda: lib.smgpu_setops_filter_raw(p, p, 1, 1, None, None, 1, 1, 0, p, 1, p, p, p, 2**30, None),          # no other sketch
        lambda: lib.smgpu_setops_filter_raw(p, p, 1, 1, p, None, 2**32, 1, 0, p, 1, p, p, p, 2**40, None),         # 2^32 other hashes
    ]
    for i, call in enumerate(calls):
        lib.sourmash_err_clear()
        assert call() == 2**64 - 1 and lib.sourmash_err_get_last_code() != 0, i
        assert "no HIP device" not in decode_str(lib.sourmash_err_get_last_message()), i
    lib.sourmash_err_clear()
