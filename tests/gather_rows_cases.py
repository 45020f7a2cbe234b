"""Inputs of the gather-rows pass (csrc/gather_rows.hip) shared by tests/test_gather_rows_core_cpu.py and tests/test_gpu_gather_rows.py, with
their expected answers from a plain-numpy restatement of its rule: the owner of a query hash is the lowest rank among the query's picks
whose row holds it; per pick the overlap with the whole query, the hashes it owns, the sum of their abundances and those abundances in
hash order; per query its size and abundance sum.  Everything at a cutoff.  Nothing here touches the package."""
import functools

import numpy as np

import gather_many_cases as gc
import many_cases as mc

NONE = 0xffffffff
BIG_ABUNDS = [1, 2**32 + 1, 2**62 - 3]


def restate(queries, abunds, rows, picks, cutoff=mc.U64_MAX):
    """queries / rows: lists of ascending u64 arrays; abunds: one u64 array per query or None (every abundance 1); picks: per query the picked
    rows in rank order.  -> dict of the pass's outputs (owner is flat over all query hashes, those above the cutoff included)."""
    cut = np.uint64(cutoff)
    owner, orig_common, unique, weighted, values, query_sizes, total_weighted = [], [], [], [], [], [], []
    for q, query in enumerate(queries):
        ab = np.ones(len(query), dtype=np.uint64) if abunds is None else np.asarray(abunds[q], dtype=np.uint64)
        inside = query <= cut
        own = np.full(len(query), NONE, dtype=np.uint32)
        for rank, row in enumerate(picks[q]):
            held = inside & np.isin(query, rows[row][rows[row] <= cut])
            orig_common.append(int(held.sum()))
            own[held & (own == NONE)] = rank                       # ranks come in ascending order: the first to hold a hash keeps it
        for rank in range(len(picks[q])):
            mine = own == rank
            unique.append(int(mine.sum()))
            weighted.append(sum(int(a) for a in ab[mine]))
            values.append(ab[mine])                                 # (the query is ascending: so are these)
        owner.append(own)
        query_sizes.append(int(inside.sum()))
        total_weighted.append(sum(int(a) for a in ab[inside]))
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype=dtype)       # noqa: E731
    return dict(owner=cat(owner, np.uint32), orig_common=np.array(orig_common, dtype=np.uint32), unique=np.array(unique, dtype=np.uint32),
                weighted=np.array(weighted, dtype=np.uint64), abund_offsets=np.concatenate([[0], np.cumsum(unique)]).astype(np.uint64),
                abund_values=cat(values, np.uint64), query_sizes=np.array(query_sizes, dtype=np.uint64),
                total_weighted=np.array(total_weighted, dtype=np.uint64))


def pick_csr(picks):
    off = np.zeros(len(picks) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in picks])
    flat = np.array([r for p in picks for r in p], dtype=np.uint32)
    return off, flat


def random_abunds(queries, seed):
    "one abundance per hash, mostly small, with 1, 2^32 + 1 and a value near 2^62 planted in every query long enough"
    rng = np.random.default_rng(seed)
    out = []
    for q in queries:
        a = rng.integers(1, 50, size=len(q), dtype=np.uint64)
        for i, v in enumerate(BIG_ABUNDS[:len(q)]):
            a[(7 * i) % len(q) if len(q) > 2 else i] = v
        out.append(a)
    return out


# ---- written by hand: gather_many_cases' query {1 .. 12}, abundance[h] = h, picks (1, 5), (2, 4), (0, 2), (6, 1) ---------------------------------
# Hash 3 is held by rows 1, 2 and 0 and goes to rank 0.
HAND_ABUNDS = [mc.u64([]), gc.HAND_QUERY.copy(), np.array([5, 6], dtype=np.uint64)]
HAND_PICK_ROWS = [[], [r for r, _ in gc.HAND_PICKS[0]], []]
HAND_EXPECTED = dict(orig_common=[5, 5, 4, 1], unique=[5, 4, 2, 1], weighted=[25, 38, 3, 12], running=[25, 63, 66, 78], total_weighted=[0, 78, 11],
                     abund_values=[3, 4, 5, 6, 7, 8, 9, 10, 11, 1, 2, 12], query_sizes=[0, 12, 2])
# a pick list made by hand that gather would never give: row 1 twice (the second owns nothing), row 3 before row 0 (which then owns nothing:
# 1 and 2 went to row 3, 3 and 4 to row 1), and row 5, which shares nothing with the query at all
USELESS_PICK_ROWS = [[], [1, 1, 3, 0, 5, 2], [5]]


@functools.lru_cache(maxsize=None)
def cases():
    """-> {name: (queries, abunds or None, rows, picks per query as [(row, isect)] or None for hand-made lists, pick rows per query, cutoff)}"""
    from sourmash_amd.minhash import _get_max_hash_for_scaled
    out = {}
    out["hand"] = (gc.HAND_QUERIES, HAND_ABUNDS, gc.HAND_ROWS, gc.oracle_picks(gc.HAND_QUERIES, gc.HAND_ROWS), HAND_PICK_ROWS, mc.U64_MAX)
    out["useless_picks"] = (gc.HAND_QUERIES, HAND_ABUNDS, gc.HAND_ROWS, None, USELESS_PICK_ROWS, mc.U64_MAX)
    queries, rows, _ = gc.edge_case()
    picks = gc.oracle_picks(queries, rows)
    pick_rows = [[r for r, _ in p] for p in picks]
    out["edge"] = (queries, random_abunds(queries, 21), rows, picks, pick_rows, mc.U64_MAX)
    out["edge_flat"] = (queries, None, rows, picks, pick_rows, mc.U64_MAX)
    queries, rows = gc.long_row_case()
    picks = gc.oracle_picks(queries, rows)
    out["long_rows"] = (queries, random_abunds(queries, 22), rows, picks, [[r for r, _ in p] for p in picks], mc.U64_MAX)
    for sq, sdb in ((1000, 2000), (2000, 1000)):
        queries, rows, cutoff = gc.scaled_case(_get_max_hash_for_scaled(sq), _get_max_hash_for_scaled(sdb))
        picks = gc.oracle_picks(queries, rows, 0, 2000, cutoff)
        out[f"cutoff_{sq}_{sdb}"] = (queries, random_abunds(queries, 23), rows, picks, [[r for r, _ in p] for p in picks], cutoff)
    return out


def expected(name):
    queries, abunds, rows, picks, pick_rows, cutoff = cases()[name]
    want = restate(queries, abunds, rows, pick_rows, cutoff)
    if picks is not None:                                           # the hashes a pick owns are what gather reported for it
        assert want["unique"].tolist() == [n for p in picks for _, n in p], name
    return want
