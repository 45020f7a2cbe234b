"""Inputs of the abundance forms of the set algebra on a SketchSet (csrc/setops.hip: the filter that moves values, the merge that
sums) shared by tests/test_abund_set_core_cpu.py and tests/test_gpu_abund_set.py, with their expected answers in plain numpy and
dicts.  Nothing here touches the package."""
import numpy as np

import setops_cases as sc

U64 = np.uint64
U64_MAX = sc.U64_MAX
EDGE_ABUNDS = [1, 2**32 - 1, 2**32, 2**64 - 1]          # the carry is 64-bit
ROW_LENGTHS = sc.ROW_LENGTHS                            # 0, 1, 63, 64, 65, 255, 256, 257
KEPT_PATTERNS = ["none", "all", "alternating", "lane 0", "lane 63", "last"]
VALUES_CARRY, VALUES_TAKE, VALUES_RANGE = 1, 2, 3
MERGE_SUM, MERGE_COUNT = 1, 2


def abund_of(hashes, salt=0):
    "an abundance that is a function of the hash (>= 1): a value that lands beside another hash shows up"
    h = np.asarray(hashes, dtype=U64)
    with np.errstate(over="ignore"):
        return ((h * U64(0x9E3779B97F4A7C15) + U64(salt)) >> U64(44)) + U64(1)


def seeded_abunds(rows, seed, edges=True):
    "one abundance array per row: small counts, with the 64-bit edge values sprinkled in"
    rng = np.random.default_rng(seed)
    out = []
    for row in rows:
        a = rng.integers(1, 60, size=len(row), dtype=np.uint64)
        if edges and len(a):
            for k, v in enumerate(EDGE_ABUNDS):
                a[(7 * k) % len(a)] = U64(v)
        out.append(a)
    return out


def flat(arrays):
    return np.concatenate(arrays).astype(U64) if len(arrays) and sum(len(a) for a in arrays) else np.zeros(0, dtype=U64)


def kept_index(pattern, k):
    idx = np.arange(k)
    return {"none": idx[:0], "all": idx, "alternating": idx[::2], "lane 0": idx[idx % 64 == 0], "lane 63": idx[idx % 64 == 63],
            "last": idx[-1:] if k else idx[:0]}[pattern]


def filter_rows(split):
    "rows of every edge length, one of split + 1 and one of 2 split + 3 hashes (two and three work items), disjoint"
    return sc.disjoint_rows(ROW_LENGTHS + [split + 1, 2 * split + 3], 51)


def pattern_other(rows, pattern):
    "-> (one sketch, partner rows): the other side holds the hashes of `pattern` of every row, and strangers no row holds"
    strangers = sc.pool(40, 52)
    strangers = strangers[~np.isin(strangers, np.concatenate(rows))]
    partners = [np.union1d(row[kept_index(pattern, len(row))], strangers[r::len(rows)]).astype(U64) for r, row in enumerate(rows)]
    return np.unique(np.concatenate(partners)).astype(U64), partners


# ---- expectations ---------------------------------------------------------------------------------------------------------------
def expected_carry(rows, abunds, other, keep_present):
    "subtract / intersect on an abundance receiver: the kept hashes with their own abundances"
    out_h, out_a = [], []
    for r, (row, ab) in enumerate(zip(rows, abunds)):
        o = other if isinstance(other, np.ndarray) else other[r]
        keep = np.isin(row, o) == bool(keep_present)
        out_h.append(row[keep].astype(U64))
        out_a.append(ab[keep].astype(U64))
    return out_h, out_a


def expected_take(rows, other_hashes, other_abunds):
    "inflate: the hashes the other side holds, with ITS abundances (a dict per other sketch, as MinHash.inflate does)"
    out_h, out_a = [], []
    for r, row in enumerate(rows):
        oh, oa = (other_hashes, other_abunds) if isinstance(other_hashes, np.ndarray) else (other_hashes[r], other_abunds[r])
        d = dict(zip(oh.tolist(), oa.tolist()))
        kept = [h for h in row.tolist() if h in d]
        out_h.append(np.array(kept, dtype=U64))
        out_a.append(np.array([d[h] for h in kept], dtype=U64))
    return out_h, out_a


def expected_range(rows, abunds, lo, hi):
    "sig filter: min <= a and (max is None or a <= max)"
    out_h, out_a = [], []
    for row, ab in zip(rows, abunds):
        keep = np.array([lo <= int(a) and (hi is None or int(a) <= hi) for a in ab], dtype=bool)
        out_h.append(row[keep].astype(U64))
        out_a.append(ab[keep].astype(U64))
    return out_h, out_a


def expected_merge_values(rows, abunds, groups, n_groups, min_rows=1, num=0, count_rows=False):
    """row g = the hashes at least min_rows rows of group g hold, with the sum of their abundances modulo 2^64 (count_rows: the number
    of rows), cut to the num smallest"""
    groups = [0] * len(rows) if groups is None else list(groups)
    out_h, out_a = [], []
    for g in range(n_groups):
        members = [r for r in range(len(rows)) if groups[r] == g]
        need = len(members) if min_rows == "all" else int(min_rows)
        sums, counts = {}, {}
        for r in members:
            for h, a in zip(rows[r].tolist(), (abunds[r].tolist() if abunds is not None else [1] * len(rows[r]))):
                sums[h] = (sums.get(h, 0) + a) % 2**64
                counts[h] = counts.get(h, 0) + 1
        kept = sorted(h for h in sums if counts[h] >= need)
        if num:
            kept = kept[:num]
        out_h.append(np.array(kept, dtype=U64))
        out_a.append(np.array([counts[h] if count_rows else sums[h] for h in kept], dtype=U64))
    return out_h, out_a


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def take_bucket_cases():
    """-> [(k, rows, other hashes, other abundances)]: another sketch of k = 1, 3, 4, 7, 8, 20 hashes that all fall into ONE bucket of
    its index (the record's inline hashes, the quad step, the search behind them): even numbers above 2^50 + 2^40, as in
    setops_cases.bucket_cases; the rows hold them and the odd numbers between them"""
    out = []
    base = (1 << 50) + (1 << 40)
    for k in (1, 3, 4, 7, 8, 20):
        other = sc.u64([base + 2 * i for i in range(k)])
        rows = [sc.u64([base + i for i in range(-3, 2 * k + 3)]), other.copy(), sc.u64([base + 2 * i + 1 for i in range(k)]), sc.u64([5, base + 2 * (k - 1)])]
        out.append((k, rows, other, abund_of(other, salt=k)))
    return out


def take_edge_cases():
    "-> [(name, rows, other hashes, other abundances)] at scaled = 1: hash 0 and 2^64 - 1 as members, receiver hashes above the other's largest, an empty other"
    rows = [sc.u64([0, 7, 9, U64_MAX]), sc.u64([0]), sc.u64([U64_MAX]), sc.u64([5]), sc.u64([])]
    edge = sc.u64([0, U64_MAX])
    low = sc.u64([0, 5, 7])
    return [
        ("hash zero and the largest", rows, edge, np.array([2**64 - 1, 2**32], dtype=U64)),
        ("receiver above the other's largest", rows, low, np.array([3, 2**32 - 1, 1], dtype=U64)),
        ("empty other", rows, sc.u64([]), np.zeros(0, dtype=U64)),
    ]


def partner_take_case(lds_cap):
    "row-wise take: partner rows of lds_cap (staged) and lds_cap + 1 (read from global memory) hashes, an empty and a short one"
    p = sc.pool(3 * lds_cap + 4000, 55)
    rng = np.random.default_rng(56)

    def pick(k):
        return np.sort(rng.choice(p, size=k, replace=False))
    partners = [pick(lds_cap), pick(lds_cap + 1), pick(0), pick(50)]
    rows = [np.union1d(partners[0][::3], pick(200)).astype(U64), np.union1d(partners[1][1::2], pick(300)).astype(U64), pick(100),
            np.union1d(partners[3], pick(70)).astype(U64)]
    return rows, partners, [abund_of(q, salt=9) for q in partners]


def run_length_case():
    "one hash held by 1, 2, 64, 65, 256 and 257 rows of one group: runs that end on and cross the chunk borders of the run pass"
    rows, abunds, hashes = [], [], {}
    base = 1000
    for k, held in enumerate((1, 2, 64, 65, 256, 257)):
        hashes[held] = base + k
    for r in range(257):
        row = sorted(h for held, h in hashes.items() if r < held)
        rows.append(np.array(row, dtype=U64))
        abunds.append(np.array([(r + 1) * 3 + (h - base) for h in row], dtype=U64))
    return rows, abunds


def wrap_case():
    "addends on both sides of 2^32, and a sum of exactly 2^64 - 1 (and one that wraps past it)"
    rows = [sc.u64([10, 20, 30, 40]), sc.u64([10, 20, 30, 40]), sc.u64([10, 30])]
    abunds = [np.array([2**32 - 1, 2**63, 2**64 - 2, 2**64 - 1], dtype=U64), np.array([1, 2**63 - 1, 1, 5], dtype=U64), np.array([2**32, 7], dtype=U64)]
    return rows, abunds, [0, 0, 1], 2
