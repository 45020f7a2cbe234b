"""Inputs of the many-queries pass (csrc/overlap_many.hip) shared by tests/test_many_core_cpu.py and tests/test_gpu_many.py, with
their expected answers in plain numpy: a dense count matrix by np.intersect1d, taken at a cutoff.  Nothing here touches the package."""
import numpy as np

U64_MAX = 2**64 - 1
MAX_HASH_1000 = 18446744073709552          # max_hash of scaled = 1000
MAX_HASH_2000 = 9223372036854776           # ... of scaled = 2000


def u64(values):
    return np.array(sorted(set(int(v) for v in values)), dtype=np.uint64)


def dense_counts(queries, rows, cutoff=U64_MAX):
    "counts[q][r] = |query q ∩ row r| over hashes <= cutoff"
    out = np.zeros((len(queries), len(rows)), dtype=np.int64)
    cut = np.uint64(cutoff)
    for q, a in enumerate(queries):
        a = a[a <= cut]
        for r, b in enumerate(rows):
            out[q, r] = len(np.intersect1d(a, b[b <= cut], assume_unique=True))
    return out


def sizes_at(rows, cutoff=U64_MAX):
    return np.array([int(np.count_nonzero(r <= np.uint64(cutoff))) for r in rows], dtype=np.uint64)


def expected_hits(counts, need):
    "(query, row, common) of the pairs with counts >= need[q] (and > 0), ordered by (query, row)"
    need = np.broadcast_to(np.asarray(need, dtype=np.int64), (counts.shape[0],))
    q, r = np.nonzero((counts >= need[:, None]) & (counts > 0))
    return q.astype(np.uint32), r.astype(np.uint32), counts[q, r].astype(np.uint32)


def scatter(n_queries, n_rows, queries, rows, common):
    out = np.zeros((n_queries, n_rows), dtype=np.int64)
    assert len(set(zip(queries.tolist(), rows.tolist()))) == len(queries)      # no pair twice
    out[queries, rows] = common
    return out


def csr(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate(rows) if len(rows) and off[-1] else np.zeros(0, dtype=np.uint64)
    return flat.astype(np.uint64), off


def hand_case(max_hash_q=MAX_HASH_1000, max_hash_db=MAX_HASH_1000):
    """3 queries x 5 rows written by hand.  Hash 7 is held by every non-empty query and row; query 1 is empty, row 3 is empty; query 0 and
    row 0 are identical, query 2 and row 1 are disjoint but for hash 7; both sets hold max_hash of the coarser side, and the finer
    side alone holds max_hash + 1 and its own largest values."""
    cutoff = min(max_hash_q, max_hash_db)
    top_q = [max_hash_q, max_hash_q - 1] if max_hash_q > cutoff else []
    top_db = [max_hash_db, max_hash_db - 1] if max_hash_db > cutoff else []
    finer_q = [cutoff + 1] if max_hash_q > cutoff else []
    finer_db = [cutoff + 1] if max_hash_db > cutoff else []
    base = [7, 11, 13, 1 << 20, (1 << 40) + 3, cutoff]
    queries = [u64(base + finer_q + top_q), u64([]), u64([7, 5, 1 << 33, cutoff - 2] + finer_q)]
    rows = [u64(base + finer_db + top_db), u64([7, 6, (1 << 33) + 1, cutoff - 3]), u64([7, 11, 1 << 33, cutoff] + finer_db), u64([]),
            u64([7, 5, 13, cutoff - 2, cutoff - 1] + top_db)]
    return queries, rows, cutoff


def largest_values_case():
    """scaled = 1: max_hash is the largest u64, which the sketches hold beside its neighbours.  Query 0 and row 0 are identical, query 2 is
    disjoint from rows 0, 1 and 4 (and they are not empty)."""
    queries = [u64([U64_MAX]), u64([1, U64_MAX - 1, U64_MAX]), u64([U64_MAX - 2])]
    rows = [u64([U64_MAX]), u64([U64_MAX - 1, U64_MAX]), u64([2, U64_MAX - 2]), u64([]), u64([1, 2, 3])]
    return queries, rows, U64_MAX


def row_length_case(block):
    "rows of 0, 1, 63, 64, 65, block - 1, block, block + 1 and 4 block + 1 hashes over a pool that 3 queries sample"
    lengths = [0, 1, 63, 64, 65, block - 1, block, block + 1, 4 * block + 1]
    rng = np.random.default_rng(11)
    pool = np.unique(rng.integers(1, MAX_HASH_1000, size=3 * (4 * block + 1), dtype=np.uint64))
    rows = [np.sort(rng.choice(pool, size=n, replace=False)) for n in lengths]
    queries = [np.sort(rng.choice(pool, size=len(pool) // 2, replace=False)), pool.copy(), pool[::7].copy()]
    return queries, rows, lengths


def block_edge_case():
    """m = 9 queries for q_block = 4 (blocks 0-3, 4-7, 8): hash 100 is held by queries 2 .. 8, so its postings straddle both block edges;
    hash 200 by 3 and 4 (one edge), hash 300 by 7 and 8 (the other), hash 400 by every query."""
    held = {100: range(2, 9), 200: (3, 4), 300: (7, 8), 400: range(9)}
    queries = []
    for q in range(9):
        queries.append(u64([1000 + q, 2000 + (q % 3)] + [h for h, qs in held.items() if q in qs]))
    rows = [u64([100, 200, 300, 400]), u64([100]), u64([200, 1003]), u64([300, 2001]), u64([400, 1008, 2002]), u64([5]), u64([])]
    return queries, rows


def random_case(m=40, n=300, pool_size=3000, seed=5):
    "synth_sketches-style: every pool hash kept with probability 1 / 10 (rows) or 1 / 6 (queries); one empty row and one 1-hash row planted"
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(1, MAX_HASH_1000, size=pool_size, dtype=np.uint64))
    rows = [pool[rng.random(len(pool)) < 0.1] for _ in range(n)]
    queries = [pool[rng.random(len(pool)) < 1 / 6] for _ in range(m)]
    rows[17 % n] = u64([])
    rows[203 % n] = pool[5:6].copy()
    queries[3 % m] = rows[40 % n].copy()        # an identical pair: Jaccard 1
    return queries, rows
