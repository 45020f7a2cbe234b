"""CPU checks of the many-queries gather (csrc/gather_many.hip): its rules (csrc/gather_many_core.hpp) compiled for the host -- the fill
order, the inverted lists, the round rule with the packed key and the test-and-clear -- against oracle.gather, the C interface, and the
entry points without a device.  None of this needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gather_many_cases as gc
import many_cases as mc
import sourmash_amd
from sourmash_amd._lowlevel import decode_str, lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "native", "gather_many_core_emul.cpp")
MARK = 0xdeadbeef

PROTOTYPES = [
    "void smgpu_gather_many_geometry(uint32_t *workgroup, uint32_t *max_query_hashes, uint32_t *max_candidates);",
    "uint64_t smgpu_gather_many_workspace_bytes(uint64_t m, uint64_t n_hits, uint64_t total_common);",
    "uint64_t smgpu_gather_many_raw(const uint64_t *d_qhashes, const uint64_t *d_qoffsets, uint64_t m, "
    "const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n_rows, "
    "const uint32_t *d_hit_queries, const uint32_t *d_hit_rows, const uint32_t *d_hit_common, "
    "uint64_t n_hits, uint64_t cutoff, uint64_t threshold_hashes, "
    "uint32_t max_query_hashes, uint32_t max_candidates, uint32_t grid, "
    "uint32_t *d_out_rows, uint32_t *d_out_isect, uint32_t *d_out_rounds, uint32_t *d_status, "
    "void *d_workspace, uint64_t workspace_bytes, void *stream);",
    "typedef struct SmgpuManyGather SmgpuManyGather;",
    "SmgpuManyGather *smgpu_sketchset_gather_many(const SmgpuSketchSet *db, const SmgpuSketchSet *queries, uint64_t threshold_hashes);",
    "void smgpu_manygather_free(SmgpuManyGather *ptr);",
    "const uint64_t *smgpu_manygather_offsets(const SmgpuManyGather *ptr);",
    "const uint32_t *smgpu_manygather_rows(const SmgpuManyGather *ptr);",
    "const uint32_t *smgpu_manygather_isect(const SmgpuManyGather *ptr);",
    "uint64_t smgpu_manygather_scaled(const SmgpuManyGather *ptr);",
    "void smgpu_manygather_stats(const SmgpuManyGather *ptr, double *out8);",
    "void smgpu_gather_many_set_limits(uint32_t max_query_hashes, uint32_t max_candidates, uint64_t batch_common);",
]


def _norm(s):
    return " ".join(s.replace("( ", "(").replace(" )", ")").split())


def test_prototypes_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "sourmash_amd.h")) as f:
        header = _norm(f.read())
    so = C.CDLL(os.path.join(ROOT, "sourmash_amd", "libsourmash_amd.so"))
    assert len(PROTOTYPES) == 12
    for p in PROTOTYPES:
        assert _norm(p) in header, p
        if p.startswith("typedef"):
            continue
        name = p.split("(")[0].split()[-1].lstrip("*")
        assert hasattr(so, name), name
        assert name in lib.functions, name                     # the binding parsed it
    assert callable(sourmash_amd.SketchSet.gather_many)
    from sourmash_amd.index import LinearIndex
    assert callable(LinearIndex.gather_many)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("gather_many_core") / "libgather_many_core_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so_path, SRC])
    so = C.CDLL(so_path)
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    so.emul_gm_batch_common.restype = u64
    so.emul_gm_lds_bytes.argtypes, so.emul_gm_lds_bytes.restype = [u32, u32], u64
    so.emul_gm_caps_fit.argtypes = [u32, u32]
    so.emul_gm_status.argtypes, so.emul_gm_status.restype = [u64, u64, u32, u32], u32
    so.emul_gm_find.argtypes, so.emul_gm_find.restype = [vp, u32, u64], u32
    so.emul_gm_pick_key.argtypes, so.emul_gm_pick_key.restype = [u32, u32], u64
    so.emul_gm_key_count.argtypes = so.emul_gm_key_candidate.argtypes = [u64]
    so.emul_gm_key_count.restype = so.emul_gm_key_candidate.restype = u32
    so.emul_gm_stop.argtypes = [u64, u64]
    so.emul_gm_bitmap_init_word.argtypes, so.emul_gm_bitmap_init_word.restype = [u32, u32], u32
    so.emul_gm_test_and_clear.argtypes = [vp, u32]
    so.emul_gm_inv_start.argtypes, so.emul_gm_inv_start.restype = [vp, u32, u32, u64], u32
    so.emul_gm_key_bits.argtypes = [u64]
    so.emul_gm_batch_end.argtypes, so.emul_gm_batch_end.restype = [vp, u64, u64, u64], u64
    so.emul_gm_gather.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, u64, u64, u64, u32, u32, vp, vp, vp, vp, vp, vp]
    so.emul_gm_gather.restype = u64
    return so


def test_geometry_is_the_headers(emul):
    wg, mqh, mc_ = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib.smgpu_gather_many_geometry(C.byref(wg), C.byref(mqh), C.byref(mc_))
    assert (wg.value, mqh.value, mc_.value) == (emul.emul_gm_block(), emul.emul_gm_max_query_hashes(), emul.emul_gm_max_candidates())
    assert wg.value == 256
    # a bit per query hash and a u32 per candidate; with the static words at most 64 KiB, so two workgroups fit a CU's 160 KiB
    assert emul.emul_gm_lds_bytes(mqh.value, mc_.value) == mqh.value // 8 + 4 * mc_.value
    assert emul.emul_gm_lds_bytes(mqh.value, mc_.value) + emul.emul_gm_lds_static() <= emul.emul_gm_lds_limit() == 64 * 1024
    assert emul.emul_gm_caps_fit(mqh.value, mc_.value) and emul.emul_gm_caps_fit(1, 1) and emul.emul_gm_caps_fit(33, 3)
    assert not emul.emul_gm_caps_fit(mqh.value, 2 * mc_.value) and not emul.emul_gm_caps_fit(8 * mqh.value, 1)
    assert emul.emul_gm_lds_bytes(1, 0) == 4 and emul.emul_gm_lds_bytes(32, 0) == 4 and emul.emul_gm_lds_bytes(33, 1) == 12
    # the caps are inclusive
    assert [emul.emul_gm_status(nq, nc, 12, 4) for nq, nc in ((12, 4), (13, 4), (12, 5), (0, 0), (2**40, 1))] == [0, 1, 1, 0, 1]


# ---- the rules one by one --------------------------------------------------------------------------------------------------------------
def test_pick_key_larger_count_then_lower_candidate(emul):
    key = emul.emul_gm_pick_key
    assert key(5, 1) > key(4, 0) and key(5, 1) > key(5, 2) and key(5, 0) > key(5, 1)            # ties go to the lowest candidate
    assert key(1, 2**32 - 2) > key(0, 0)                                                        # a count always beats none
    for c, i in ((0, 0), (1, 0), (7, 300), (2**32 - 1, 8191)):
        k = key(c, i)
        assert k == (c << 32) | (~i & 0xffffffff) and emul.emul_gm_key_count(k) == c and emul.emul_gm_key_candidate(k) == i
    # the loop ends at a best count of 0, or below the threshold in hashes
    assert emul.emul_gm_stop(key(0, 3), 0) and not emul.emul_gm_stop(key(1, 3), 0) and not emul.emul_gm_stop(key(1, 3), 1)
    assert emul.emul_gm_stop(key(4, 0), 5) and not emul.emul_gm_stop(key(5, 0), 5) and emul.emul_gm_stop(key(2**32 - 1, 0), 2**32)


def test_bitmap_words_and_test_and_clear(emul):
    for n in (0, 1, 31, 32, 33, 63, 64, 65, 100):
        words = [emul.emul_gm_bitmap_init_word(w, n) for w in range(5)]
        bits = np.array(words, dtype=np.uint32)
        assert [bool(words[p >> 5] >> (p & 31) & 1) for p in range(160)] == [p < n for p in range(160)], n
        for p in list(range(n))[::-1]:
            assert emul.emul_gm_test_and_clear(bits.ctypes.data, p) == 1                        # set: cleared, and said so
            assert emul.emul_gm_test_and_clear(bits.ctypes.data, p) == 0                        # the second taker sees it gone
        assert not bits.any()


def test_find_and_list_starts(emul):
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 63, 64, 65, 1000):
        Q = np.unique(rng.integers(1, 2**64 - 1, size=n, dtype=np.uint64))
        Qp = np.append(Q, np.uint64(0))
        for i, h in enumerate(Q.tolist()):
            assert emul.emul_gm_find(Qp.ctypes.data, len(Q), h) == i
        for h in (0, 2**64 - 1, int(Q[0]) + 1 if len(Q) else 5):
            if h not in set(Q.tolist()):
                assert emul.emul_gm_find(Qp.ctypes.data, len(Q), h) == 2**32 - 1
    keys = np.array([3, 3, 3, 7, 9, 9, 20, 0], dtype=np.uint64)                                 # (the last entry lies behind the range)
    for lo, hi in ((0, 7), (1, 7), (2, 5), (4, 4)):
        for k in range(0, 22):
            want = lo + int(np.searchsorted(keys[lo:hi], k, side="left"))
            assert emul.emul_gm_inv_start(keys.ctypes.data, lo, hi, k) == want
    assert [emul.emul_gm_key_bits(v) for v in (1, 2, 3, 4, 255, 256, 2**31, 2**63)] == [1, 2, 2, 3, 8, 9, 32, 64]
    for v in (1, 2, 5, 1000, 2**31 - 1):
        assert (v - 1) >> emul.emul_gm_key_bits(v) == 0                                         # every key below the span fits the bits


def test_batches_are_contiguous_and_under_the_budget(emul):
    def ranges(weight, budget):
        w = np.array(weight, dtype=np.uint64)
        out, q = [], 0
        while q < len(w):
            e = emul.emul_gm_batch_end(w.ctypes.data, len(w), q, budget)
            assert e > q                                                                        # a range always takes a query
            out.append((q, e))
            q = e
        return out
    assert ranges([5, 5, 5, 5], 100) == [(0, 4)]
    assert ranges([5, 5, 5, 5], 11) == [(0, 2), (2, 4)]
    assert ranges([5, 5, 5, 5], 10) == [(0, 1), (1, 2), (2, 3), (3, 4)]                         # under the budget, not at it
    assert ranges([50, 1, 1, 50, 0, 0], 10) == [(0, 1), (1, 3), (3, 4), (4, 6)]                       # a query above the budget runs alone
    assert ranges([0, 0, 0], 1) == [(0, 3)]
    assert ranges([2**32 - 3, 1, 1], 2**40) == [(0, 2), (2, 3)]                                 # never 2^32 - 1 entries or more in one range
    rng = np.random.default_rng(4)
    w = rng.integers(0, 50, size=200)
    got = ranges(w.tolist(), 120)
    assert got[0][0] == 0 and got[-1][1] == 200 and all(a[1] == b[0] for a, b in zip(got, got[1:]))
    assert all(w[a:b].sum() < 120 or b - a == 1 for a, b in got)
    assert emul.emul_gm_batch_common() < 2**32 - 1


# ---- the whole pipeline on the host ------------------------------------------------------------------------------------------------------
def run_emul(emul, queries, rows, hits, cutoff=mc.U64_MAX, thr=0, max_query_hashes=0, max_candidates=0, want_lists=False):
    qh, qoff = mc.csr(queries)
    h, off = mc.csr(rows)
    qh, h = np.append(qh, np.uint64(0)), np.append(h, np.uint64(0))
    qoff, off = qoff.astype(np.uint64), off.astype(np.uint64)
    hq, hr, hc = (np.append(a, np.uint32(0)) for a in hits)
    n_hits, m = len(hits[0]), len(queries)
    out_rows, out_isect = np.full(n_hits + 2, MARK, dtype=np.uint32), np.full(n_hits + 2, MARK, dtype=np.uint32)
    rounds, status = np.full(m + 1, MARK, dtype=np.uint32), np.full(m + 1, MARK, dtype=np.uint32)
    total = int(hits[2].sum())
    fpos, inv = np.full(total + 1, MARK, dtype=np.uint32), np.full(total + 1, MARK, dtype=np.uint32)
    got = emul.emul_gm_gather(qh.ctypes.data, qoff.ctypes.data, m, h.ctypes.data, off.ctypes.data, len(rows), hq.ctypes.data, hr.ctypes.data, hc.ctypes.data,
                              n_hits, cutoff, thr, max_query_hashes, max_candidates, out_rows.ctypes.data, out_isect.ctypes.data, rounds.ctypes.data,
                              status.ctypes.data, fpos.ctypes.data if want_lists else None, inv.ctypes.data if want_lists else None)
    assert rounds[m] == status[m] == MARK and (out_rows[n_hits:] == MARK).all() and (out_isect[n_hits:] == MARK).all()
    return got, out_rows[:n_hits], out_isect[:n_hits], rounds[:m], status[:m], fpos[:total], inv[:total]


def check_against_oracle(emul, queries, rows, threshold_bp, scaled=1000, cutoff=mc.U64_MAX, counts=None):
    thr = gc.threshold_hashes(threshold_bp, scaled)
    hits = gc.hits_of(queries, rows, cutoff, thr, counts)
    got, out_rows, out_isect, rounds, status, _, _ = run_emul(emul, queries, rows, hits, cutoff, thr)
    want = gc.oracle_picks(queries, rows, threshold_bp, scaled, cutoff)
    assert not status.any()
    picks = gc.picks_from_slots(hits, out_rows, out_isect, rounds, len(queries))
    assert picks == want
    assert got == sum(len(w) for w in want)
    # the slots behind a query's rounds are untouched
    first = np.searchsorted(hits[0], np.arange(len(queries) + 1))
    for q in range(len(queries)):
        assert (out_rows[first[q] + rounds[q]:first[q + 1]] == MARK).all() and (out_isect[first[q] + rounds[q]:first[q + 1]] == MARK).all()
    return want


@pytest.mark.parametrize("threshold_bp", sorted(gc.HAND_PICKS))
def test_hand_case_equals_oracle(emul, threshold_bp):
    want = check_against_oracle(emul, gc.HAND_QUERIES, gc.HAND_ROWS, threshold_bp)
    assert want == [[], gc.HAND_PICKS[threshold_bp], []]


def test_hand_case_fill_order_and_inverted_lists(emul):
    hits = gc.hits_of(gc.HAND_QUERIES, gc.HAND_ROWS)
    assert [a.tolist() for a in hits] == [[1] * 5, [0, 1, 2, 3, 6], [4, 5, 5, 2, 1]]
    _, _, _, _, _, fpos, inv = run_emul(emul, gc.HAND_QUERIES, gc.HAND_ROWS, hits, want_lists=True)
    # forward CSR: per hit the positions in the query of the row's hashes, ascending (hash h of the query {1 .. 12} stands at h - 1)
    assert fpos.tolist() == [0, 1, 2, 3] + [2, 3, 4, 5, 6] + [2, 7, 8, 9, 10] + [0, 1] + [11]
    # inverted lists: by position, the candidates holding it in candidate order (hash 3 by candidates 0, 1, 2; hash 12 by candidate 4)
    by_pos = {0: [0, 3], 1: [0, 3], 2: [0, 1, 2], 3: [0, 1], 4: [1], 5: [1], 6: [1], 7: [2], 8: [2], 9: [2], 10: [2], 11: [4]}
    assert inv.tolist() == [c for p in range(12) for c in by_pos[p]]


@pytest.fixture(scope="module")
def random_sets():
    queries, rows = gc.random_case()
    return queries, rows, mc.dense_counts(queries, rows)


@pytest.mark.parametrize("threshold_bp,rounds_lo,rounds_hi", [(0, 21, 24), (20_000, 9, 11), (60_000, 0, 3)])
def test_random_case_equals_oracle(emul, random_sets, threshold_bp, rounds_lo, rounds_hi):
    queries, rows, counts = random_sets
    want = check_against_oracle(emul, queries, rows, threshold_bp, counts=counts)
    assert want[3] == [(40, len(queries[3]))]                               # the planted identical pair: one round
    n = [len(w) for q, w in enumerate(want) if q != 3]
    assert rounds_lo <= min(n) and max(n) <= rounds_hi
    if threshold_bp == 0:
        assert (np.count_nonzero(counts, axis=1) >= 298).all()            # more candidates than one stride of 256 lanes
    if threshold_bp == 60_000:
        assert min(n) == 0 and max(n) >= 1                                  # one query returns nothing


@pytest.mark.parametrize("scaled_q,scaled_db", [(1000, 2000), (2000, 1000), (1000, 1000)])
def test_cutoff_case_equals_oracle_on_downsampled_sides(emul, scaled_q, scaled_db):
    from sourmash_amd.minhash import _get_max_hash_for_scaled
    queries, rows, cutoff = gc.scaled_case(_get_max_hash_for_scaled(scaled_q), _get_max_hash_for_scaled(scaled_db))
    scaled = max(scaled_q, scaled_db)
    for threshold_bp in (0, 2 * scaled, 2 * scaled + 1):
        want = check_against_oracle(emul, queries, rows, threshold_bp, scaled, cutoff)
        assert want[1] == []
    if scaled_q != scaled_db:
        # the finer side holds the cutoff, its neighbours above and its own largest value: they are cut off, the cutoff itself counts
        finer = queries if scaled_q < scaled_db else rows
        assert sum(len(a) for a in finer) - sum(len(a) for a in gc.cut(finer, cutoff)) >= 8
        assert any(len(a) and a[-1] == cutoff for a in gc.cut(finer, cutoff))


def test_edge_case_equals_oracle(emul):
    queries, rows, owner = gc.edge_case()
    counts = mc.dense_counts(queries, rows)
    n_cand = np.count_nonzero(counts, axis=1).tolist()
    assert n_cand == gc.CANDIDATE_COUNTS + [5] * len(gc.QUERY_SIZES) + [2]
    assert [len(q) for q in queries] == [40] * len(gc.CANDIDATE_COUNTS) + gc.QUERY_SIZES + [70]
    want = check_against_oracle(emul, queries, rows, 0, counts=counts)
    first_row = np.searchsorted(owner, np.arange(len(queries)))
    for q, picks in enumerate(want[:-1]):
        if n_cand[q] >= 2:
            assert first_row[q] + 1 not in [r for r, _ in picks]            # the second of two identical rows is never picked
    assert want[-1] == [(len(rows) - 1, 70)]                                # a query identical to a row: one round


def test_long_rows_equal_oracle(emul):
    queries, rows = gc.long_row_case()
    assert [len(r) for r in rows] == gc.LONG_ROWS and [len(q) for q in queries] == [2000, 667]
    for threshold_bp in (0, 300_000):
        want = check_against_oracle(emul, queries, rows, threshold_bp)
    assert len(want[0]) >= 2


def test_caps_name_exactly_the_queries_beyond_them(emul):
    queries, rows, _ = gc.edge_case()
    counts = mc.dense_counts(queries, rows)
    hits = gc.hits_of(queries, rows, counts=counts)
    want = gc.oracle_picks(queries, rows)
    n_cand = np.count_nonzero(counts, axis=1)
    sizes = np.array([len(q) for q in queries])
    for mqh, mcand in ((40, 64), (64, 5), (1, 1), (70, 257)):
        got, out_rows, out_isect, rounds, status, _, _ = run_emul(emul, queries, rows, hits, max_query_hashes=mqh, max_candidates=mcand)
        beyond = (sizes > mqh) | (n_cand > mcand)
        assert status.tolist() == beyond.astype(int).tolist()
        assert (rounds[beyond] == MARK).all()                                # nothing is written for them
        picks = gc.picks_from_slots(hits, out_rows, out_isect, np.where(beyond, 0, rounds), len(queries))
        first = np.searchsorted(hits[0], np.arange(len(queries) + 1))
        for q in range(len(queries)):
            if beyond[q]:
                assert (out_rows[first[q]:first[q + 1]] == MARK).all()
            else:
                assert picks[q] == want[q]
        assert got == sum(len(want[q]) for q in range(len(queries)) if not beyond[q])
    assert beyond.sum() == 0


def test_a_wrong_common_count_is_found(emul):
    hits = gc.hits_of(gc.HAND_QUERIES, gc.HAND_ROWS)
    for delta in (1, -1):
        bad = [a.copy() for a in hits]
        bad[2][1] = int(hits[2][1]) + delta                                             # row 1 shares 5 hashes with the query, not 6 or 4
        assert run_emul(emul, gc.HAND_QUERIES, gc.HAND_ROWS, bad)[0] == 2**64 - 1


def test_emulation_under_sanitizers_as_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "gather_many_core_emul_san")
    try:
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-DGM_EMUL_MAIN", "-o", exe, SRC], stderr=subprocess.PIPE)
    except subprocess.CalledProcessError as exc:
        if b"asan" in exc.stderr or b"ubsan" in exc.stderr or b"sanitize" in exc.stderr:
            pytest.skip("this compiler has no sanitizer runtimes")
        raise
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok: 4 rounds"), out.stdout + out.stderr


# ---- without a device ----------------------------------------------------------------------------------------------------------------
def raw_call(p, **kw):
    ws = kw.get("ws", lib.smgpu_gather_many_workspace_bytes(1, 1, 1))
    return lib.smgpu_gather_many_raw(p, p, kw.get("m", 1), p, p, kw.get("n_rows", 1), p, p, p, kw.get("n_hits", 1), 2**64 - 1, 0, kw.get("mqh", 0),
                                     kw.get("mc", 0), kw.get("grid", 0), p, kw.get("out_isect", p), p, kw.get("status", p), kw.get("workspace", p), ws, None)


def test_entry_points_raise_without_gpu():
    if sourmash_amd.gpu_available():
        pytest.skip("a GPU is present: the calls succeed (covered by tests/test_gpu_gather_many.py)")
    from sourmash_amd import MinHash, SketchSet
    from sourmash_amd.exceptions import SourmashError
    buf = np.zeros(64, dtype=np.uint64)
    lib.sourmash_err_clear()
    assert lib.smgpu_gather_many_workspace_bytes(1, 1, 1) > 0 and lib.sourmash_err_get_last_code() == 0     # (a size: no device needed)
    assert raw_call(buf.ctypes.data) == 2**64 - 1
    assert lib.sourmash_err_get_last_code() != 0 and "no HIP device" in decode_str(lib.sourmash_err_get_last_message())
    lib.sourmash_err_clear()
    mh = MinHash(0, 21, scaled=1000)
    mh.add_many([5, 7])
    with pytest.raises(SourmashError, match="no HIP device"):              # the sets themselves live on the device
        SketchSet([mh]).gather_many(SketchSet([mh]))
    lib.sourmash_err_clear()


def test_raw_entry_refuses_bad_arguments_before_the_device():
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    wg, mqh, mc_ = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib.smgpu_gather_many_geometry(C.byref(wg), C.byref(mqh), C.byref(mc_))
    assert lib.smgpu_gather_many_workspace_bytes(1, 1, 100) > lib.smgpu_gather_many_workspace_bytes(1, 1, 1) > 0
    for kwargs in (dict(mc=2 * mc_.value), dict(mqh=8 * mqh.value), dict(grid=2**21), dict(ws=16), dict(workspace=None), dict(status=None),
                   dict(out_isect=None), dict(n_hits=2**32 - 1), dict(n_rows=2**32), dict(m=2**32)):
        lib.sourmash_err_clear()
        assert raw_call(p, **kwargs) == 2**64 - 1 and lib.sourmash_err_get_last_code() != 0, kwargs
        assert "no HIP device" not in decode_str(lib.sourmash_err_get_last_message()), kwargs
    lib.sourmash_err_clear()

