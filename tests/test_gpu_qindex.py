"""GPU parity of the query index (csrc/qindex.hpp over csrc/qindex_core.hpp) at its edges: the position of every probe through the
test-only entry smgpu_debug_qindex_find against the host emulation (tests/native/qindex_emul.cpp) and np.searchsorted, for every query
family of tests/qindex_cases.py and every lookup form; then the same queries through the passes that use the index -- the one-wave-
per-row overlap, both builders of gather's inverted index with its apply step, and the many-queries pass.  Run with -m gpu."""
import numpy as np
import pytest

import oracle
import qindex_cases as qc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    assert sourmash_amd.gpu_available()
    return sourmash_amd


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return qc.build_emul(tmp_path_factory.mktemp("qindex_gpu"))


@pytest.fixture(scope="module")
def cases():
    return qc.all_cases()


def dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


# ---- position-level ------------------------------------------------------------------------------------------------------------------
def gpu_positions(q, probes, form):
    import torch
    from sourmash_amd._lowlevel import lib
    d_q, d_p = dev_u64(q), dev_u64(probes)
    guard = 8
    out = torch.full((len(probes) + guard,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    lib.sourmash_err_clear()
    lib.smgpu_debug_qindex_find(d_q.data_ptr(), len(q), d_p.data_ptr(), len(probes), form, out.data_ptr(), None)
    assert lib.sourmash_err_get_last_code() == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint32)
    assert (host[len(probes):] == 0x5a5a5a5a).all()
    return host[:len(probes)]


@pytest.mark.parametrize("form", sorted(qc.FORMS))
def test_positions_are_the_emulations_and_searchsorted(sm, emul, cases, form):
    """Families A-G: one hash at every bit length (a shift of 63 from 2^63 on), two to five hashes, dense runs (shift 0), buckets of
    0 .. 9, 16 and 300 hashes with full buckets ending at q_max, uniform queries around powers of two, 0 with 2^64 - 1, one crowded
    bucket.  Probes: the query, its neighbours, both ends of the buckets, the fixed values, random ones below and above q_max."""
    for name, q in cases:
        probes = qc.probes_for(q)
        got = gpu_positions(q, probes, qc.FORMS[form])
        host, out_of_bounds = qc.emul_find(emul, q, probes, qc.FORMS[form])
        assert out_of_bounds == 0, name
        want = qc.expected_positions(q, probes)
        wrong = np.nonzero(got != want)[0]
        assert len(wrong) == 0, (name, [(hex(int(probes[i])), int(got[i]), int(want[i])) for i in wrong[:5]])
        assert np.array_equal(got, host), name


def test_probe_entry_refuses_what_it_cannot_index(sm):
    from sourmash_amd._lowlevel import lib
    d = dev_u64([1, 2, 3, 4])
    for nq, form in ((0, 0), (3, 3), (3, -1)):
        lib.sourmash_err_clear()
        lib.smgpu_debug_qindex_find(d.data_ptr(), nq, d.data_ptr(), 4, form, d.data_ptr(), None)
        assert lib.sourmash_err_get_last_code() != 0, (nq, form)
    lib.sourmash_err_clear()


# ---- through the real callers ----------------------------------------------------------------------------------------------------------
def caller_cases():
    out = [(f"A-{v:#x}", qc.u64([v])) for v in qc.FAMILY_A_CALLERS]
    return out + qc.family_d() + qc.family_g()


CALLER_NAMES = [f"A-{v:#x}" for v in qc.FAMILY_A_CALLERS] + [f"D-{c}" for c in qc.FAMILY_D_RUNS] + ["G-dense", "G-2^40"]


@pytest.fixture(scope="module")
def caller_data():
    "name -> (query, rows, |Q ∩ row| by numpy), computed once"
    out = {}
    for name, q in caller_cases():
        rows = qc.caller_database(q)
        assert len(rows) == 300 and len(rows[253]) == 0 and np.array_equal(rows[254], q) and np.array_equal(rows[251], rows[252])
        want = qc.membership_counts(q, rows)
        assert want[254] == len(q) and set(want[:250].tolist()) == {0, 1}      # one-hash rows: members and non-members
        out[name] = (q, rows, want)
    assert sorted(out) == sorted(CALLER_NAMES)
    return out


@pytest.mark.parametrize("name", CALLER_NAMES)
def test_overlaps_through_the_row_kernel(sm, caller_data, name):
    "be.overlaps (pair_ops.hip: the table form, one wave per row): op 0, then op 1 with half of the query and a counter pre-set to 1"
    import torch
    from sourmash_amd import device as smd, parallel
    q, rows, want = caller_data[name]
    assert np.array_equal(want, [oracle.intersection_size(q, r)[0] for r in rows])
    be = parallel.DeviceBackend()
    h, off = smd.pack_csr(rows)
    cnt = be.zeros((len(rows),), torch.int64)
    be.overlaps(dev_u64(q), len(q), h, off, len(rows), cnt, 0)
    assert np.array_equal(cnt.cpu().numpy(), want)
    part = q[::2].copy()                                          # (a one-hash query: the whole of it)
    low = 254                                                     # the row that is the whole query
    cnt[low] = 1                                                  # a counter someone lowered: must stop at 0
    be.overlaps(dev_u64(part), len(part), h, off, len(rows), cnt, 1)
    sub = np.array([oracle.intersection_size(part, r)[0] for r in rows], dtype=np.int64)
    assert sub[low] == len(part) >= 1
    before = want.copy()
    before[low] = 1
    assert np.array_equal(cnt.cpu().numpy(), np.maximum(before - sub, 0))


@pytest.mark.parametrize("build", ["atomic", "ranges-staged", "ranges-direct"])
@pytest.mark.parametrize("name", CALLER_NAMES)
def test_gather_index_and_apply(sm, caller_data, name, build, monkeypatch):
    """be.gather_state (gather_build.hip, gather.hip: the record form, where the POSITION matters -- a wrong one leaves a counter
    non-zero): counters, the number of postings, the greedy loop against the oracle's, and every counter zero at the end."""
    from sourmash_amd import device as smd, parallel
    monkeypatch.setenv("SMG_GATHER_BUILD", build.split("-")[0])
    monkeypatch.setenv("SMG_GATHER_FILL", build.split("-")[1] if "-" in build else "staged")
    q, rows, want = caller_data[name]
    be = parallel.DeviceBackend()
    d_q = dev_u64(q)
    # as built: the whole query as a row wins the first round and ends the gather.  Without that row: many rounds, the tie of the two
    # identical rows among them
    for whole in (True, False):
        if not whole:
            rows = rows[:254] + [np.zeros(0, dtype=np.uint64)] + rows[255:]
            want = want.copy()
            want[254] = 0
        h, off = smd.pack_csr(rows)
        st = be.gather_state(d_q, len(q), h, off, len(rows), 0)
        assert np.array_equal(st.counters(), want.astype(np.uint64)), whole
        assert int(be.lib.smgpu_gather_postings(st._ptr)) == int(want.sum()), whole
        st.begin(0, len(rows))
        got = st.run()
        assert got == oracle.gather(q, *oracle.make_csr(rows), threshold_bp=0, scaled=1000, nthreads=8), whole
        assert got[0] == (int(np.argmax(want)), int(want.max()))   # the fullest row, the lowest index among equals
        assert want.max() == len(q) if whole else len(got) >= 1
        assert not st.counters().any(), whole


@pytest.mark.parametrize("name", CALLER_NAMES)
def test_many_queries_pass(sm, caller_data, name):
    """smgpu_many_overlap_raw (overlap_many.hip: records over the union of the queries) with the family's query alone -- the union is
    the query -- and with three queries, against the per-query overlaps of the row kernel and numpy."""
    import torch
    import test_gpu_many as tgm
    from sourmash_amd import device as smd, parallel
    q, rows, want = caller_data[name]
    probes = np.unique(qc.probes_for(q, seed=3))
    queries = [q, q[::2].copy(), probes[::max(1, len(probes) // 500)].copy()]
    be = parallel.DeviceBackend()
    h, off = smd.pack_csr(rows)
    counts = np.zeros((3, len(rows)), dtype=np.int64)
    for i, a in enumerate(queries):
        cnt = be.zeros((len(rows),), torch.int64)
        be.overlaps(dev_u64(a), len(a), h, off, len(rows), cnt, 0)
        counts[i] = cnt.cpu().numpy()
        assert np.array_equal(counts[i], qc.membership_counts(a, rows)), i
    assert np.array_equal(counts[0], want)
    tgm.check_raw(queries[:1], rows, counts[:1])
    tgm.check_raw(queries, rows, counts)
