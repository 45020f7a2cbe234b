"""Inputs of the many-queries gather (csrc/gather_many.hip) shared by tests/test_gather_many_core_cpu.py and tests/test_gpu_gather_many.py,
with their expected answers from oracle.gather (the reference's CounterGather / GatherDatabases loop restated) on sketches cut at the
common scaled in plain numpy.  Nothing here touches the package."""
import numpy as np

import many_cases as mc
import oracle

# ---- written by hand: query {1 .. 12} at scaled 1000 against seven rows ------------------------------------------------------------------
# Round 1: rows 0, 1, 2 share 4, 5, 5 hashes -- a tie, the lowest row (1) wins with {3 .. 7}.  Round 2: row 2 keeps {8 .. 11} = 4, row 0
# keeps {1, 2} = 2 as does row 3.  Round 3: the tie of rows 0 and 3 after decrements goes to row 0, which drives row 3 to 0.  Round 4: row 6
# with {12}.  Row 4 is empty, row 5 disjoint.  ceil(4500 / 1000) = 5 keeps round 1 only, as does 5000; 5001 asks for 6 hashes.
HAND_QUERY = mc.u64(range(1, 13))
HAND_ROWS = [mc.u64([1, 2, 3, 4, 100]), mc.u64([3, 4, 5, 6, 7]), mc.u64([3, 8, 9, 10, 11]), mc.u64([1, 2]), mc.u64([]), mc.u64([500]), mc.u64([12])]
HAND_PICKS = {0: [(1, 5), (2, 4), (0, 2), (6, 1)], 2000: [(1, 5), (2, 4), (0, 2)], 4500: [(1, 5)], 5000: [(1, 5)], 5001: []}
# the hand query as one of three: beside an empty query and a query that no row overlaps
HAND_QUERIES = [mc.u64([]), HAND_QUERY, mc.u64([900, 901])]


def cut(rows, cutoff):
    return [r[r <= np.uint64(cutoff)] for r in rows]


def threshold_hashes(threshold_bp, scaled):
    "search.py:15-37 for integer counts: the loop stops below ceil(threshold_bp / scaled) hashes"
    return -(-int(threshold_bp) // int(scaled)) if threshold_bp else 0


def oracle_picks(queries, rows, threshold_bp=0, scaled=1000, cutoff=mc.U64_MAX):
    "[oracle.gather(q, rows)] with both sides cut at the cutoff (= downsampled to `scaled`)"
    hashes, offsets = oracle.make_csr(cut(rows, cutoff))
    return [oracle.gather(q, hashes, offsets, threshold_bp=threshold_bp, scaled=scaled) for q in cut(queries, cutoff)]


def hits_of(queries, rows, cutoff=mc.U64_MAX, need=1, counts=None):
    "(query, row, common) u32 arrays of the candidates, ordered by (query, row): what the many-queries pass leaves for need = max(1, threshold)"
    if counts is None:
        counts = mc.dense_counts(queries, rows, cutoff)
    return mc.expected_hits(counts, max(1, need))


def picks_from_slots(hits, out_rows, out_isect, rounds, m):
    "the raw entry's outputs as per-query [(row, isect)]: the picks of query q stand in the slots of its own hits"
    first = np.searchsorted(hits[0], np.arange(m))
    return [[(int(out_rows[first[q] + i]), int(out_isect[first[q] + i])) for i in range(int(rounds[q]))] for q in range(m)]


# ---- lane and word edges -----------------------------------------------------------------------------------------------------------------
CANDIDATE_COUNTS = [1, 63, 64, 65, 255, 256, 257]
QUERY_SIZES = [1, 31, 32, 33, 63, 64, 65]


def edge_case(seed=9):
    """One query per candidate count (40 hashes each) and one per query size (5 candidates each), every query over a hash range of its own, so
    that its candidates are exactly the rows built for it: random non-empty subsets of the query with hashes of their own beside.  The
    query's first hash is held by every one of its rows (one long inverted list); rows 1 and 0 of every query with two rows or more are
    identical.  Then a query identical to a row, beside a smaller row.  -> queries, rows, owner (the query each row was built for)."""
    rng = np.random.default_rng(seed)
    queries, rows, owner = [], [], []
    shapes = [(nc, 40) for nc in CANDIDATE_COUNTS] + [(5, qs) for qs in QUERY_SIZES]
    for k, (nc, qs) in enumerate(shapes):
        base = (k + 1) * 10**9
        q = np.sort(rng.choice(np.arange(base, base + 10 * qs + 10, dtype=np.uint64), size=qs, replace=False))
        queries.append(q)
        for r in range(nc):
            keep = q[rng.random(qs) < rng.uniform(0.1, 0.6)]
            own = np.arange(base + 10**6 + 8 * r, base + 10**6 + 8 * r + int(rng.integers(0, 4)), dtype=np.uint64)
            row = mc.u64(list(keep) + [q[0]] + list(own))
            rows.append(rows[-1].copy() if r == 1 else row)
            owner.append(k)
    k = len(queries)
    q = mc.u64(range(10**15, 10**15 + 70))
    queries.append(q)
    rows += [q[:30].copy(), q.copy()]
    owner += [k, k]
    return queries, rows, owner


def long_row_case(seed=13):
    """Rows around the 512 hashes a wave of the fill looks up at a time (8 groups of 64): 511, 512, 513, 1023, 1024, 1025 and 1537 hashes, half
    of each drawn from the one query's 2,000 hashes, beside a second query of 700 of them."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(1, mc.MAX_HASH_1000, size=6000, dtype=np.uint64))
    query = np.sort(rng.choice(pool, size=2000, replace=False))
    rest = np.setdiff1d(pool, query)
    rows = []
    for n in LONG_ROWS:
        rows.append(np.sort(np.concatenate([rng.choice(query, size=n // 2, replace=False), rng.choice(rest, size=n - n // 2, replace=False)])))
    return [query, query[::3][:700].copy()], rows


LONG_ROWS = [511, 512, 513, 1023, 1024, 1025, 1537]


def random_case():
    return mc.random_case(m=40, n=300)


def scaled_case(max_hash_q, max_hash_db):
    """hand_case-style sets for two scaled values: both sides hold the cutoff, the finer side alone cutoff + 1 .. cutoff + 3 and its own max_hash
    (a sketch never holds a hash above its own max_hash, so the coarser side has none of them).  Query 1 and row 3 are empty."""
    cutoff = min(max_hash_q, max_hash_db)
    finer_q = [cutoff + 1, cutoff + 2, cutoff + 3, max_hash_q] if max_hash_q > cutoff else []
    finer_db = [cutoff + 1, cutoff + 2, cutoff + 3, max_hash_db] if max_hash_db > cutoff else []
    queries = [mc.u64([7, 11, 13, 17, 1 << 20, cutoff - 1, cutoff] + finer_q), mc.u64([]), mc.u64([5, 6, cutoff] + finer_q)]
    rows = [mc.u64([7, 11, cutoff] + finer_db), mc.u64([13, 17, 1 << 20] + finer_db[:1]), mc.u64([13, 17, cutoff - 1, 5] + finer_db), mc.u64([]),
            mc.u64([6, 5, cutoff - 1])]
    return queries, rows, cutoff
