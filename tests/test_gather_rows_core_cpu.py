"""CPU checks of the gather-rows pass (csrc/gather_rows.hip): its rules (csrc/gather_rows_core.hpp) compiled for the host -- the owner by
lowest rank, the pair key, the segment search, the workspace -- against the numpy restatement of tests/gather_rows_cases.py on every
case, the C interface, the entry points without a device, and GatherStats.rows on hand-made arrays.  None of this needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gather_many_cases as gc
import gather_rows_cases as rc
import many_cases as mc
import sourmash_amd
from sourmash_amd._lowlevel import decode_str, lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "native", "gather_rows_core_emul.cpp")
MARK32, MARK64 = 0xdeadbeef, 0xdeadbeefdeadbeef

PROTOTYPES = [
    "uint64_t smgpu_gather_rows_workspace_bytes(uint64_t m, uint64_t q_total, uint64_t n_picks);",
    "uint64_t smgpu_gather_rows_raw(const uint64_t *d_qhashes, const uint64_t *d_qabunds, const uint64_t *d_qoffsets, uint64_t m, uint64_t q_total, "
    "const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n_rows, "
    "const uint64_t *d_pick_offsets, const uint32_t *d_pick_rows, uint64_t n_picks, "
    "uint64_t cutoff, uint32_t grid, "
    "uint32_t *d_owner, uint32_t *d_orig_common, uint32_t *d_unique, uint64_t *d_weighted, "
    "uint64_t *d_abund_offsets, uint64_t *d_abund_values, uint64_t *d_query_sizes, uint64_t *d_total_weighted, "
    "void *d_workspace, uint64_t workspace_bytes, void *stream);",
    "typedef struct SmgpuGatherRows SmgpuGatherRows;",
    "SmgpuGatherRows *smgpu_sketchset_gather_rows_many(const SmgpuSketchSet *db, const SmgpuSketchSet *queries, const uint64_t *abunds, "
    "uint64_t threshold_hashes);",
    "SmgpuGatherRows *smgpu_sketchset_gather_rows(const SmgpuSketchSet *db, const SourmashKmerMinHash *query, uint64_t threshold_hashes);",
    "void smgpu_gatherrows_free(SmgpuGatherRows *ptr);",
    "uint64_t smgpu_gatherrows_queries(const SmgpuGatherRows *ptr);",
    "uint64_t smgpu_gatherrows_n_rows(const SmgpuGatherRows *ptr);",
    "const uint64_t *smgpu_gatherrows_offsets(const SmgpuGatherRows *ptr);",
    "const uint32_t *smgpu_gatherrows_rows(const SmgpuGatherRows *ptr);",
    "const uint32_t *smgpu_gatherrows_isect(const SmgpuGatherRows *ptr);",
    "const uint32_t *smgpu_gatherrows_orig_common(const SmgpuGatherRows *ptr);",
    "const uint64_t *smgpu_gatherrows_weighted(const SmgpuGatherRows *ptr);",
    "const uint64_t *smgpu_gatherrows_abund_offsets(const SmgpuGatherRows *ptr);",
    "const uint64_t *smgpu_gatherrows_abund_values(const SmgpuGatherRows *ptr);",
    "const uint64_t *smgpu_gatherrows_query_sizes(const SmgpuGatherRows *ptr);",
    "const uint64_t *smgpu_gatherrows_row_sizes(const SmgpuGatherRows *ptr);",
    "const uint64_t *smgpu_gatherrows_total_weighted(const SmgpuGatherRows *ptr);",
    "uint64_t smgpu_gatherrows_scaled(const SmgpuGatherRows *ptr);",
    "void smgpu_gatherrows_stats(const SmgpuGatherRows *ptr, double *out5);",
]


def _norm(s):
    return " ".join(s.replace("( ", "(").replace(" )", ")").split())


def test_prototypes_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "sourmash_amd.h")) as f:
        header = _norm(f.read())
    so = C.CDLL(os.path.join(ROOT, "sourmash_amd", "libsourmash_amd.so"))
    assert len(PROTOTYPES) == 20
    for p in PROTOTYPES:
        assert _norm(p) in header, p
        if p.startswith("typedef"):
            continue
        name = p.split("(")[0].split()[-1].lstrip("*")
        assert hasattr(so, name), name
        assert name in lib.functions, name                     # the binding parsed it
    from sourmash_amd.index import LinearIndex
    assert callable(sourmash_amd.SketchSet.gather_stats_many) and callable(sourmash_amd.SketchSet.gather_stats)
    assert callable(LinearIndex.gather_results_many) and callable(sourmash_amd.GatherStats.rows)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("gather_rows_core") / "libgather_rows_core_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so_path, SRC])
    so = C.CDLL(so_path)
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    so.emul_gr_owner_merge.argtypes, so.emul_gr_owner_merge.restype = [u32, u32], u32
    so.emul_gr_owned.argtypes = [u32]
    so.emul_gr_none.restype = so.emul_gr_block.restype = so.emul_gr_owned.restype = so.emul_gr_sizes_fit.restype = u32
    so.emul_gr_segment_of.argtypes, so.emul_gr_segment_of.restype = [vp, u64, u64], u32
    so.emul_gr_pair_key.argtypes, so.emul_gr_pair_key.restype = [u32, u32], u64
    so.emul_gr_key_pick.argtypes = so.emul_gr_key_pos.argtypes = [u64]
    so.emul_gr_key_pick.restype = so.emul_gr_key_pos.restype = u32
    so.emul_gr_key_bits.argtypes = [u64]
    so.emul_gr_sizes_fit.argtypes = [u64, u64, u64, u64]
    so.emul_gr_layout.argtypes = [u64, u64, u64, u64, u64, vp]
    so.emul_gr_rows.argtypes = [vp, vp, vp, u64, u64, vp, vp, u64, vp, vp, u64, u64] + [vp] * 8
    so.emul_gr_rows.restype = u64
    return so


# ---- the rules one by one --------------------------------------------------------------------------------------------------------------
def test_owner_is_the_lowest_rank(emul):
    none = emul.emul_gr_none()
    assert none == rc.NONE and emul.emul_gr_block() == 256
    assert emul.emul_gr_owner_merge(none, 5) == 5 and emul.emul_gr_owner_merge(5, 3) == 3 and emul.emul_gr_owner_merge(3, 5) == 3
    assert emul.emul_gr_owner_merge(0, 0) == 0 and emul.emul_gr_owner_merge(none, none - 1) == none - 1
    assert not emul.emul_gr_owned(none) and emul.emul_gr_owned(0) and emul.emul_gr_owned(none - 1)


def test_segment_of_steps_over_empty_segments(emul):
    off = np.array([0, 0, 4, 4, 4, 9, 10, 10], dtype=np.uint64)                  # segments 0, 2, 3 and 6 are empty
    m = len(off) - 1
    for i in range(10):
        want = int(np.searchsorted(off, i, side="right")) - 1
        assert emul.emul_gr_segment_of(off.ctypes.data, m, i) == want and off[want] <= i < off[want + 1]
    off = np.array([3, 5], dtype=np.uint64)                                        # offsets that do not start at 0
    assert [emul.emul_gr_segment_of(off.ctypes.data, 1, i) for i in (3, 4)] == [0, 0]
    rng = np.random.default_rng(2)
    for m in (1, 2, 63, 64, 65, 1000):
        off = np.concatenate([[0], np.cumsum(rng.integers(0, 4, size=m))]).astype(np.uint64)
        for i in range(0, int(off[-1]), max(1, int(off[-1]) // 97)):
            assert emul.emul_gr_segment_of(off.ctypes.data, m, i) == int(np.searchsorted(off, i, side="right")) - 1
    # offsets that are no offsets at all: the answer still lies in [0, m)
    junk = rng.integers(0, 2**63, size=41, dtype=np.uint64)
    assert all(emul.emul_gr_segment_of(junk.ctypes.data, 40, int(i)) < 40 for i in rng.integers(0, 2**63, size=50, dtype=np.uint64))


def test_pair_key_orders_by_pick_then_position(emul):
    key = emul.emul_gr_pair_key
    assert key(0, 5) < key(1, 0) and key(3, 7) < key(3, 8) and key(2, 2**32 - 1) < key(3, 0)
    for pick, pos in ((0, 0), (1, 2**32 - 1), (2**32 - 2, 17)):
        k = key(pick, pos)
        assert k == (pick << 32) | pos and emul.emul_gr_key_pick(k) == pick and emul.emul_gr_key_pos(k) == pos
    assert [emul.emul_gr_key_bits(n) for n in (0, 1, 2, 3, 4, 1500, 2**32 - 2)] == [33, 33, 34, 34, 35, 43, 64]
    for n in (1, 2, 5, 1000, 2**31):
        assert key(n - 1, 2**32 - 1) >> emul.emul_gr_key_bits(n) == 0                 # every key of a call fits the bits it is sorted by


def test_sizes_and_workspace(emul):
    fit = emul.emul_gr_sizes_fit
    assert fit(1, 1, 1, 1) and fit(0, 0, 0, 0) and fit(2**32 - 2, 2**32 - 2, 2**32 - 2, 2**32 - 2)
    assert not fit(2**32 - 1, 1, 1, 1) and not fit(1, 2**32 - 1, 1, 1) and not fit(1, 1, 2**32, 1) and not fit(1, 1, 1, 2**32 - 1)
    out = np.zeros(9, dtype=np.uint64)
    for m, q_total, n_picks, scan, sort in ((3, 100, 10, 700, 5000), (0, 0, 0, 0, 0), (1000, 5_000_000, 30_000, 4096, 1 << 20)):
        emul.emul_gr_layout(m, q_total, n_picks, scan, sort, out.ctypes.data)
        qn, scal, wide, scan_at, keys_a, vals_a, keys_b, sort_at, end = out.tolist()
        assert all(v % 256 == 0 for v in out.tolist()) and qn == 0
        assert scal - qn >= 4 * (m + 1) and wide - scal >= 256 and scan_at - wide >= 8 * (n_picks + 1) and keys_a - scan_at >= scan
        assert vals_a - keys_a >= 8 * q_total and keys_b - vals_a >= 8 * q_total and sort_at - keys_b >= 8 * q_total and end - sort_at >= sort
    # the library's own size is this layout with the device library's two scratch sizes: it grows with every argument
    base = lib.smgpu_gather_rows_workspace_bytes(3, 100, 10)
    assert 0 < base < lib.smgpu_gather_rows_workspace_bytes(3, 100_000, 10) and base < lib.smgpu_gather_rows_workspace_bytes(3, 100, 10_000)
    assert base <= lib.smgpu_gather_rows_workspace_bytes(3000, 100, 10)


# ---- the whole pass on the host ------------------------------------------------------------------------------------------------------------
def run_emul(emul, queries, abunds, rows, pick_rows, cutoff=mc.U64_MAX, pick_csr=None, n_rows=None, qoff=None):
    qh, off0 = mc.csr(queries)
    h, off = mc.csr(rows)
    q_total = len(qh)
    qa = np.append(np.concatenate([np.asarray(a, dtype=np.uint64) for a in abunds]) if abunds is not None and q_total else np.zeros(0, dtype=np.uint64),
                   np.uint64(0)) if abunds is not None else None
    qh, h = np.append(qh, np.uint64(0)), np.append(h, np.uint64(0))
    qoff = off0.astype(np.uint64) if qoff is None else np.asarray(qoff, dtype=np.uint64)
    off = off.astype(np.uint64)
    poff, prow = rc.pick_csr(pick_rows) if pick_csr is None else pick_csr
    m, n_picks = len(queries), len(prow)
    prow = np.append(prow, np.uint32(0))
    o32 = [np.full(size + 2, MARK32, dtype=np.uint32) for size in (q_total, n_picks, n_picks)]
    o64 = [np.full(size + 2, MARK64, dtype=np.uint64) for size in (n_picks, n_picks + 1, q_total, m, m)]
    got = emul.emul_gr_rows(qh.ctypes.data, qa.ctypes.data if qa is not None else None, qoff.ctypes.data, m, q_total, h.ctypes.data, off.ctypes.data,
                            len(rows) if n_rows is None else n_rows, poff.ctypes.data, prow.ctypes.data, n_picks, cutoff,
                            *[a.ctypes.data for a in o32], *[a.ctypes.data for a in o64])
    sizes32, sizes64 = (q_total, n_picks, n_picks), (n_picks, n_picks + 1, q_total, m, m)
    assert all((a[s:] == MARK32).all() for a, s in zip(o32, sizes32)) and all((a[s:] == MARK64).all() for a, s in zip(o64, sizes64))
    names = ("owner", "orig_common", "unique", "weighted", "abund_offsets", "abund_values", "query_sizes", "total_weighted")
    out = dict(zip(names, [a[:s] for a, s in zip(o32, sizes32)] + [a[:s] for a, s in zip(o64, sizes64)]))
    if got < 2**63:
        out["abund_values"] = out["abund_values"][:got]
    return got, out


def same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_hand_case_is_the_table(emul):
    "the hand case with abundance[h] = h: the restatement AND the core's rules on the host give the table, figure by figure"
    queries, abunds, rows, _, pick_rows, cutoff = rc.cases()["hand"]
    got, out = run_emul(emul, queries, abunds, rows, pick_rows, cutoff)
    e = rc.HAND_EXPECTED
    assert got == sum(e["unique"]) == 12
    for want in (rc.expected("hand"), out):
        assert want["orig_common"].tolist() == e["orig_common"] and want["unique"].tolist() == e["unique"] and want["weighted"].tolist() == e["weighted"]
        assert np.cumsum(want["weighted"]).tolist() == e["running"] and want["total_weighted"].tolist() == e["total_weighted"]
        assert want["abund_values"].tolist() == e["abund_values"] and want["query_sizes"].tolist() == e["query_sizes"]
        assert want["abund_offsets"].tolist() == [0, 5, 9, 11, 12]
        # hash 3 is held by rows 1, 2 and 0: it goes to rank 0; hashes 900 and 901 have no owner
        assert want["owner"].tolist() == [2, 2, 0, 0, 0, 0, 0, 1, 1, 1, 1, 3, rc.NONE, rc.NONE]


@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_emulation_equals_the_restatement(emul, name):
    queries, abunds, rows, picks, pick_rows, cutoff = rc.cases()[name]
    want = rc.expected(name)
    got, out = run_emul(emul, queries, abunds, rows, pick_rows, cutoff)
    assert got == int(want["unique"].sum()) == len(want["abund_values"])
    same(out, want)
    if name == "useless_picks":
        assert want["unique"].tolist() == [5, 0, 2, 0, 0, 4, 0] and want["orig_common"].tolist() == [5, 5, 2, 4, 0, 5, 0]
    if name.startswith("cutoff"):
        assert sum(len(q) for q in queries) > int(want["query_sizes"].sum()) or sum(len(r) for r in rows) > sum(len(r) for r in gc.cut(rows, cutoff))
        assert (want["owner"] != rc.NONE).any()
    if name == "edge":
        seen = set(np.concatenate(abunds).tolist())
        assert set(rc.BIG_ABUNDS) <= seen and int(want["weighted"].max()) > 2**62


def test_emulation_refuses_bad_offsets_and_rows(emul):
    queries, abunds, rows, _, pick_rows, _ = rc.cases()["hand"]
    poff, prow = rc.pick_csr(pick_rows)
    bad = lambda bits: 2**64 - 1 - bits                                                        # noqa: E731
    assert run_emul(emul, queries, abunds, rows, pick_rows, n_rows=6)[0] == bad(4)              # row 6 is picked
    assert run_emul(emul, queries, abunds, rows, pick_rows, pick_csr=(np.array([0, 4, 0, 4], dtype=np.uint64), prow))[0] == bad(2)
    assert run_emul(emul, queries, abunds, rows, pick_rows, pick_csr=(np.array([0, 0, 3, 3], dtype=np.uint64), prow))[0] == bad(2)
    assert run_emul(emul, queries, abunds, rows, pick_rows, qoff=[0, 12, 0, 14])[0] == bad(1)
    assert run_emul(emul, queries, abunds, rows, pick_rows, qoff=[0, 0, 12, 15])[0] == bad(1)


def test_emulation_under_sanitizers_as_a_program_of_its_own(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + probe.stderr.strip().splitlines()[-1])
    exe = str(tmp_path / "gather_rows_core_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DGR_EMUL_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok: 12 owned"), out.stdout + out.stderr


# ---- GatherStats.rows on hand-made arrays ----------------------------------------------------------------------------------------------------
def hand_stats(with_abundance, sizes_times=1):
    "sizes_times: the sketch sizes multiplied, for sizes large enough that an ANI is given (rows() is arithmetic on what it is handed)"
    want = rc.expected("hand")
    poff, prow = rc.pick_csr(rc.HAND_PICK_ROWS)
    flat = rc.restate(gc.HAND_QUERIES, None, gc.HAND_ROWS, rc.HAND_PICK_ROWS)
    src = want if with_abundance else flat
    return sourmash_amd.GatherStats(
        offsets=poff, pick_rows=prow, isect=want["unique"], orig_common=want["orig_common"], weighted=src["weighted"], abund_offsets=src["abund_offsets"],
        abund_values=src["abund_values"], query_sizes=want["query_sizes"] * np.uint64(sizes_times), row_sizes=mc.sizes_at(gc.HAND_ROWS) * np.uint64(sizes_times),
        total_weighted=src["total_weighted"],
        scaled=1000, with_abundance=with_abundance, ksize=21, moltype="DNA",
        match_info={r: dict(name=f"row{r}", filename=f"row{r}.sig", md5=f"{r:032x}") for r in range(7)},
        query_info=[dict(query_name=f"q{q}", query_filename=None, query_md5=f"{q:08x}") for q in range(3)])


def test_rows_from_hand_made_arrays():
    from sourmash_amd.distance_utils import containment_to_distance
    from sourmash_amd.minhash import MinHash
    from sourmash_amd.search import GatherResult
    stats = hand_stats(True)
    assert len(stats) == 3 and stats.per_query() == [[], gc.HAND_PICKS[0], []]
    rows = stats.rows()
    assert rows[0] == [] and rows[2] == [] and len(rows[1]) == 4
    cols = set(GatherResult.gather_write_cols)
    ani_cols = {"query_containment_ani", "match_containment_ani", "average_containment_ani", "max_containment_ani"}
    for r in rows[1]:
        # a None is not written: no query file name, and no ANI from sketches of 12 and 5 hashes (MinHash.size_is_accurate)
        assert set(r) == cols - {"query_filename"} - ani_cols and r["potential_false_negative"] in (False, True)
    first, third = rows[1][0], rows[1][2]
    assert first["intersect_bp"] == 5000 and first["unique_intersect_bp"] == 5000 and first["remaining_bp"] == 7000 and first["query_bp"] == 12000
    assert first["f_orig_query"] == 5 / 12 and first["f_unique_to_query"] == 5 / 12 and first["f_unique_weighted"] == 25 / 78
    assert first["f_match"] == first["f_match_orig"] == MinHash._debias(5, 5, 1000)
    assert (first["average_abund"], first["median_abund"], first["std_abund"]) == (5.0, 5.0, float(np.std([3, 4, 5, 6, 7])))
    assert (first["n_unique_weighted_found"], first["sum_weighted_found"], first["total_weighted_hashes"]) == (25, 25, 78)
    assert (first["name"], first["filename"], first["md5"], first["query_name"], first["query_md5"]) == ("row1", "row1.sig", f"{1:032x}", "q1", "00000001")
    assert (first["gather_result_rank"], first["ksize"], first["moltype"], first["scaled"], first["query_n_hashes"], first["query_abundance"]) == \
        (0, 21, "DNA", 1000, 12, True)
    # rank 2 is row 0: 4 of its 5 hashes are in the query, 2 of them were still uncovered
    assert third["intersect_bp"] == 4000 and third["unique_intersect_bp"] == 2000 and third["remaining_bp"] == (12 - 5 - 4 - 2) * 1000
    assert third["f_match"] == MinHash._debias(2, 5, 1000) and third["f_match_orig"] == MinHash._debias(4, 5, 1000)
    assert (third["average_abund"], third["median_abund"], third["std_abund"]) == (1.5, 1.5, 0.5) and third["sum_weighted_found"] == 66
    assert [r["sum_weighted_found"] for r in rows[1]] == rc.HAND_EXPECTED["running"]
    # sketches a thousand times the size: the ANI columns are distance_utils' on the containments of (original query, match)
    big = hand_stats(True, 1000).rows()[1][2]
    assert set(big) == cols - {"query_filename"} and big["query_n_hashes"] == 12000
    q_ani = containment_to_distance(MinHash._debias(4, 12000, 1000), 21, 1000, n_unique_kmers=12_000_000, confidence=0.95, estimate_ci=False, prob_threshold=1e-3)
    m_ani = containment_to_distance(MinHash._debias(4, 5000, 1000), 21, 1000, n_unique_kmers=5_000_000, confidence=0.95, estimate_ci=False, prob_threshold=1e-3)
    assert big["query_containment_ani"] == q_ani.ani and big["match_containment_ani"] == m_ani.ani and q_ani.ani is not None
    assert big["average_containment_ani"] == (q_ani.ani + m_ani.ani) / 2 and big["max_containment_ani"] == max(q_ani.ani, m_ani.ani)
    assert big["potential_false_negative"] == bool(q_ani.p_exceeds_threshold or m_ani.p_exceeds_threshold)
    # without abundances: the columns of the reference's ignore-abundance row
    flat = hand_stats(False).rows()[1]
    for r, a in zip(flat, rows[1]):
        assert set(r) == cols - {"query_filename", "average_abund", "median_abund", "std_abund", "n_unique_weighted_found"} - ani_cols
        assert r["f_unique_weighted"] == r["f_unique_to_query"] and r["query_abundance"] is False and r["total_weighted_hashes"] == 12
        assert {k: v for k, v in r.items() if k not in ("f_unique_weighted", "query_abundance", "sum_weighted_found", "total_weighted_hashes")} == \
            {k: a[k] for k in r if k not in ("f_unique_weighted", "query_abundance", "sum_weighted_found", "total_weighted_hashes")}
    assert [r["sum_weighted_found"] for r in flat] == [5, 9, 11, 12]


# ---- without a device ----------------------------------------------------------------------------------------------------------------
def raw_call(p, **kw):
    ws = kw.get("ws", lib.smgpu_gather_rows_workspace_bytes(1, 8, 1))
    return lib.smgpu_gather_rows_raw(p, kw.get("abunds", p), p, kw.get("m", 1), kw.get("q_total", 8), p, p, kw.get("n_rows", 1), kw.get("pick_offsets", p), p,
                                     kw.get("n_picks", 1), 2**64 - 1, kw.get("grid", 0), kw.get("owner", p), p, p, kw.get("weighted", p),
                                     kw.get("abund_offsets", p), p, p, kw.get("total_weighted", p), kw.get("workspace", p), ws, None)


def test_entry_points_raise_without_gpu():
    if sourmash_amd.gpu_available():
        pytest.skip("a GPU is present: the calls succeed (covered by tests/test_gpu_gather_rows.py)")
    from sourmash_amd import MinHash, SketchSet
    from sourmash_amd.exceptions import SourmashError
    buf = np.zeros(64, dtype=np.uint64)
    lib.sourmash_err_clear()
    assert lib.smgpu_gather_rows_workspace_bytes(1, 8, 1) > 0 and lib.sourmash_err_get_last_code() == 0     # (a size: no device needed)
    assert raw_call(buf.ctypes.data) == 2**64 - 1
    assert lib.sourmash_err_get_last_code() != 0 and "no HIP device" in decode_str(lib.sourmash_err_get_last_message())
    lib.sourmash_err_clear()
    assert raw_call(buf.ctypes.data, abunds=None) == 2**64 - 1                                  # no abundances is no refusal
    assert "no HIP device" in decode_str(lib.sourmash_err_get_last_message())
    lib.sourmash_err_clear()
    mh = MinHash(0, 21, scaled=1000)
    mh.add_many([5, 7])
    with pytest.raises(SourmashError, match="no HIP device"):              # the sets themselves live on the device
        SketchSet([mh]).gather_stats_many(SketchSet([mh]))
    lib.sourmash_err_clear()


def test_entries_refuse_bad_arguments_before_the_device():
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    for kwargs in (dict(grid=2**21), dict(ws=16), dict(workspace=None), dict(owner=None), dict(weighted=None), dict(abund_offsets=None),
                   dict(total_weighted=None), dict(pick_offsets=None), dict(n_picks=2**32 - 1), dict(q_total=2**32 - 1), dict(n_rows=2**32), dict(m=2**32),
                   dict(m=0, q_total=0)):
        lib.sourmash_err_clear()
        assert raw_call(p, **kwargs) == 2**64 - 1 and lib.sourmash_err_get_last_code() != 0, kwargs
        assert "no HIP device" not in decode_str(lib.sourmash_err_get_last_message()), kwargs
    for args in ((2**32 - 1, 1, 1), (1, 2**32 - 1, 1), (1, 1, 2**32 - 1)):
        lib.sourmash_err_clear()
        assert lib.smgpu_gather_rows_workspace_bytes(*args) == 2**64 - 1 and lib.sourmash_err_get_last_code() != 0
    # the handle entries: null handles are refused, with no device asked for
    for call in (lambda: lib.smgpu_sketchset_gather_rows_many(None, None, None, 0), lambda: lib.smgpu_sketchset_gather_rows(None, None, 0)):
        lib.sourmash_err_clear()
        assert not call() and lib.sourmash_err_get_last_code() != 0
        assert "null pointer" in decode_str(lib.sourmash_err_get_last_message())
    lib.sourmash_err_clear()
