"""GPU parity at the edges of the flattened slice walk (csrc/slice_walk.hpp) in the kernels that use it: the range builder of the gather
index (csrc/gather_build.hip: pass 1 by lookups, the partition pass, the direct fill) and the apply of the two-kernel rounds
(csrc/gather.hip).  The dictionary index's walk is covered by test_gpu_compare.py (_index_builder_cases).  Run with -m gpu."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

RANGE = 32768                       # BR_RANGE of gather_build.hip: query positions per range
TOP = np.uint64(2**64 - 1)


def _query_and_strangers(n_query, n_strangers, seed):
    "a sorted query of distinct hashes below 2^64 - 1, and hashes that are not in it"
    rng = np.random.default_rng(seed)
    allh = np.unique(rng.integers(1, 2**63, size=2 * (n_query + n_strangers), dtype=np.int64).astype(np.uint64) * np.uint64(2))
    pick = rng.permutation(len(allh))
    qh = np.sort(allh[pick[:n_query]])
    return qh, allh[pick[n_query:n_query + n_strangers]], rng


@pytest.fixture(scope="module")
def range_case():
    """A query of two ranges, the second 300 positions long, and the rows every database below is cut from: the shapes first, so
    that a database of one row is the row with the long slice."""
    qh, strangers, rng = _query_and_strangers(RANGE + 300, 4000, 7)
    in_range_0 = strangers[(strangers > qh[0]) & (strangers < qh[RANGE - 1])]
    rows = [
        np.concatenate([qh[100:357], qh[RANGE + 5:RANGE + 50], [TOP]]),   # 257 elements in range 0 (> 4 x 64: a second batch of pass 1), some in
                                                                          # range 1, and the hash the walks' filler value looks like
        np.zeros(0, dtype=np.uint64),                                     # empty
        in_range_0[:90],                                                  # entirely outside the query
        qh[1000:1064],                                                    # exactly 64 elements
        qh[2000:2256],                                                    # exactly 256
        qh[RANGE + 10:RANGE + 300],                                       # only in the second range
        np.array([TOP], dtype=np.uint64),
        np.concatenate([qh[::7], in_range_0[100:400]]),                   # long, hits and misses interleaved
        np.concatenate([np.array([1, 3, 5], dtype=np.uint64), qh[:3]]),   # starts below Q[0]: pass 1 looks those up (and misses) as well
    ]
    assert qh[0] > 5
    while len(rows) < 129:
        i = len(rows)
        n_q, n_s = (0, 0) if i % 11 == 0 else (int(rng.integers(0, 140)), int(rng.integers(0, 60)))
        rows.append(np.concatenate([rng.choice(qh, size=n_q, replace=False), rng.choice(strangers, size=n_s, replace=False)]))
    rows[127] = qh[500:757].copy()                                        # 257 again: the last slice of a wave's group of 16 ...
    rows[128] = qh[600:857].copy()                                        # ... and a group of one row
    rows = [np.unique(r).astype(np.uint64) for r in rows]
    assert len(rows[0][rows[0] < qh[RANGE]]) == 257 and len(rows[3]) == 64 and len(rows[4]) == 256
    assert rows[5].min() >= qh[RANGE] and not np.isin(rows[2], qh).any()
    overlap = np.array([oracle.intersection_size(qh, r)[0] for r in rows], dtype=np.uint64)
    return qh, rows, overlap


@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, 127, 128, 129])
@pytest.mark.parametrize("fill", ["staged", "direct"])
def test_range_builder_at_group_and_batch_edges(range_case, fill, n_rows, monkeypatch):
    """Pass 1 by lookups, then the partition pass + scatter (staged) or the direct fill: one row short of a wave's 16 slices, exactly
    16, one more; one short of a workgroup's 128 rows, exactly, one more.  Every counter is |Q ∩ row|, the postings are their sum,
    the rounds give the oracle's picks and bring every counter to zero (every (hash, row) pair in exactly one posting)."""
    import torch
    from sourmash_amd import device as smd, parallel
    monkeypatch.setenv("SMG_GATHER_BUILD", "ranges")
    monkeypatch.setenv("SMG_GATHER_FILL", fill)
    monkeypatch.setenv("SMG_GATHER_PASS1", "ranges")
    qh, rows, overlap = range_case
    dbh, want = rows[:n_rows], overlap[:n_rows]
    be = parallel.DeviceBackend()
    h, off = smd.pack_csr(dbh)
    q = torch.from_numpy(qh.view(np.int64).copy()).cuda()
    st = be.gather_state(q, len(qh), h, off, len(dbh), 0)
    assert np.array_equal(st.counters(), want)
    assert int(be.lib.smgpu_gather_postings(st._ptr)) == int(want.sum())
    st.begin(0, len(dbh))
    assert st.run() == oracle.gather(qh, *oracle.make_csr(dbh), threshold_bp=0, scaled=1000, nthreads=4)
    assert not st.counters().any()


def test_apply_of_the_two_kernel_rounds_at_list_edges():
    """The apply kernel walks the posting lists of a wave's two row hashes as one list, 4 x 64 postings a batch.  The switch between
    the loop forms is read once per process: an interpreter of its own with SMG_GATHER_LOOP=scan."""
    import os, subprocess, sys
    from conftest import ROOT
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_slice_walk as t\nt._apply_cases()\nprint('ok')\n" % (ROOT, os.path.join(ROOT, "tests")))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, SMG_GATHER_LOOP="scan"))
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout[-1500:], p.stderr[-3000:])


def _apply_cases():
    import torch
    import sourmash_amd as sm
    from sourmash_amd import device as smd, parallel
    from sourmash_amd.index import CounterGather
    qh, strangers, rng = _query_and_strangers(3000, 500, 11)
    rows = []
    for i in range(600):
        rows.append(np.concatenate([rng.choice(qh[100:], size=int(rng.integers(0, 12)), replace=False), rng.choice(strangers, size=int(rng.integers(0, 4)))]))
    for i in range(0, 257):
        rows[i] = np.concatenate([rows[i], qh[10:11]])            # a query hash held by 257 rows: more than one batch of 256 postings
    for i in range(300, 556):
        rows[i] = np.concatenate([rows[i], qh[20:21]])            # ... and one held by exactly 256
    rows[0] = np.concatenate([qh[10:11], qh[100:160]])             # wins the first round: the list of 257 is walked there
    rows[300] = np.concatenate([qh[20:21], qh[200:240]])           # wins the second: the list of 256
    rows[590] = qh[30:31].copy()                                   # a row of one hash: a wave with one list
    rows[591] = qh[40:47].copy()                                   # odd length: the last wave has one list
    rows[592] = qh[100:160].copy()                                 # inside the first winner: never wins, its counter must reach zero
    rows = [np.unique(r).astype(np.uint64) for r in rows]
    holders = lambda x: sum(1 for r in rows if x in r)
    assert holders(qh[10]) == 257 and holders(qh[20]) == 256 and len(rows[591]) == 7
    be = parallel.DeviceBackend()
    h, off = smd.pack_csr(rows)
    q = torch.from_numpy(qh.view(np.int64).copy()).cuda()
    st = be.gather_state(q, len(qh), h, off, len(rows), 0)
    want = np.array([oracle.intersection_size(qh, r)[0] for r in rows], dtype=np.uint64)
    assert np.array_equal(st.counters(), want)
    picks = oracle.gather(qh, *oracle.make_csr(rows), threshold_bp=0, scaled=1000, nthreads=4)
    assert [i for i, _ in picks[:2]] == [0, 300] and 590 in [i for i, _ in picks] and 592 not in [i for i, _ in picks]
    st.begin(0, 1)                                                 # the first round alone: the two long lists, each holder one down
    assert st.run() == picks[:1]
    covered = np.isin(qh, rows[0])
    assert np.array_equal(st.counters(), np.array([oracle.intersection_size(qh[~covered], r)[0] for r in rows], dtype=np.uint64))
    st.begin(0, len(rows))
    assert st.run() == picks[1:]
    assert not st.counters().any()
    # A row none of whose hashes is still uncovered cannot WIN a round (its counter is zero: key 0, the rounds stop); what reaches
    # the apply kernel with nothing uncovered is an intersect consumed a second time (CounterGather.consume -> smgpu_counter_consume ->
    # gather_consume_list -> apply_kernel<false>; the only shortcut on that way is for an EMPTY intersect).  Every wave then finds no
    # hit and nothing moves -- which is also what no launch at all would show, so that this call reaches the kernel is read from the
    # code, not asserted.  What is asserted is the kernel's test per hash: a third intersect, the first one plus two hashes still
    # uncovered, takes exactly those two from the rows that hold them.
    sig = lambda hashes, name: sm.SourmashSignature(_mh(sm, hashes), name=name)
    query = sig(range(0, 20), "q")
    cg = CounterGather(query)
    for ss in (sig(range(0, 10), "a"), sig(range(7, 15), "b"), sig(range(13, 17), "c")):
        cg.add(ss)
    sr, isect = cg.peek(query.minhash.to_mutable())
    cg.consume(isect)
    assert sorted(cg.counter.values(), reverse=True) == [5, 4]
    cg.consume(isect)
    assert sorted(cg.counter.values(), reverse=True) == [5, 4]
    cg.consume(_mh(sm, list(range(0, 10)) + [13, 14]))             # b = 7..14 and c = 13..16 hold both
    assert sorted(cg.counter.values(), reverse=True) == [3, 2]


def _mh(sm, hashes):
    mh = sm.MinHash(0, 21, scaled=1)
    mh.add_many(hashes)
    return mh
