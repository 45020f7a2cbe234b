"""Inputs of the set algebra on a SketchSet (csrc/setops.hip) shared by tests/test_setops_core_cpu.py and tests/test_gpu_setops.py,
with their expected answers in plain numpy (np.unique with counts, np.intersect1d, np.setdiff1d).  Nothing here touches the package."""
import numpy as np

U64_MAX = 2**64 - 1
MAX_HASH_1000 = 18446744073709552          # max_hash of scaled = 1000 (55 bits)
MAX_HASH_10000 = 1844674407370955          # ... of scaled = 10000
ROW_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257]
FILTER_LENGTHS = ROW_LENGTHS + [511, 512, 513, 1300]


def u64(values):
    return np.array(sorted(set(int(v) for v in values)), dtype=np.uint64)


def csr(rows):
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    if len(rows):
        off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate(rows).astype(np.uint64) if len(rows) and off[-1] else np.zeros(0, dtype=np.uint64)
    return flat, off


def uncsr(flat, off):
    return [flat[int(off[r]):int(off[r + 1])] for r in range(len(off) - 1)]


def pool(size, seed, max_hash=MAX_HASH_1000):
    rng = np.random.default_rng(seed)
    return np.unique(rng.integers(1, max_hash, size=size, dtype=np.uint64))


# ---- merge ------------------------------------------------------------------------------------------------------------------------
def expected_merge(rows, groups, n_groups, min_rows=1, num=0):
    "row g = the hashes at least min_rows rows of group g hold ('all': every row of the group), cut to the num smallest"
    groups = [0] * len(rows) if groups is None else list(groups)
    out = []
    for g in range(n_groups):
        members = [rows[r] for r in range(len(rows)) if groups[r] == g]
        need = len(members) if min_rows == "all" else int(min_rows)
        if not members:
            out.append(np.zeros(0, dtype=np.uint64))
            continue
        values, counts = np.unique(np.concatenate(members), return_counts=True)
        kept = values[counts >= need].astype(np.uint64)
        out.append(kept[:num] if num else kept)
    return out


def merge_cases():
    """-> [(name, rows, groups or None, n_groups, max_hash)].  Rows overlap (they sample one pool), so unions, counts and intersections
    all have something to say."""
    p = pool(700, 21)
    rng = np.random.default_rng(22)
    by_length = [np.sort(rng.choice(p, size=k, replace=False)) for k in ROW_LENGTHS]
    cases = [
        ("one group", by_length, None, 1, MAX_HASH_1000),
        # groups out of row order; group 3 has no rows; group 4 has one row (the result is that row, bit for bit)
        ("scattered groups", by_length, [2, 0, 2, 1, 0, 2, 4, 1], 5, MAX_HASH_1000),
        ("identical rows", [by_length[5].copy() for _ in range(5)], [0, 0, 1, 0, 1], 2, MAX_HASH_1000),
        ("no rows", [], [], 0, MAX_HASH_1000),
        ("no rows, one group", [], None, 1, MAX_HASH_1000),
        ("all rows empty", [u64([]) for _ in range(4)], [1, 0, 1, 2], 3, MAX_HASH_1000),
        ("one row", [by_length[7]], None, 1, MAX_HASH_1000),
        # hash 0 is a member like any other
        ("hash zero", [u64([0, 5, 9]), u64([0, 9, 11]), u64([0]), u64([3])], [0, 0, 1, 1], 2, MAX_HASH_1000),
        # scaled = 1: 64 hash bits, the wide form for every G >= 2; the largest u64 beside 0
        ("scaled one", [u64([0, 1, U64_MAX]), u64([0, U64_MAX - 1, U64_MAX]), u64([U64_MAX]), u64([0])], [1, 1, 0, 0], 2, U64_MAX),
        ("scaled one, one group", [u64([0, 1, U64_MAX]), u64([0, U64_MAX - 1, U64_MAX])], None, 1, U64_MAX),
    ]
    return cases


def boundary_case(n_groups):
    "the same rows in the groups 0, 1 and 511 of n_groups >= 512 groups: at scaled = 1000, 512 groups pack into one key and 513 do not"
    p = pool(400, 23)
    rng = np.random.default_rng(24)
    rows = [np.sort(rng.choice(p, size=k, replace=False)) for k in (100, 257, 64, 1, 300, 65)]
    return rows, [511, 0, 1, 511, 0, 511], n_groups


# ---- filter -----------------------------------------------------------------------------------------------------------------------
def expected_filter(rows, other, keep_present):
    "other: one array (against every row) or one array per row"
    out = []
    for r, row in enumerate(rows):
        o = other if isinstance(other, np.ndarray) else other[r]
        out.append((np.intersect1d(row, o, assume_unique=True) if keep_present else np.setdiff1d(row, o, assume_unique=True)).astype(np.uint64))
    return out


def disjoint_rows(lengths, seed, max_hash=MAX_HASH_1000):
    "rows of the given lengths that share no hash, ascending in the pool's order (row r lies below row r + 1)"
    p = pool(2 * sum(lengths) + 64, seed, max_hash)[:sum(lengths)]
    assert len(p) == sum(lengths)
    rows, at = [], 0
    for k in lengths:
        rows.append(p[at:at + k].copy())
        at += k
    return rows


def present_patterns(k):
    "the index sets of a row of k hashes that the other sketch holds: each pattern and its complement"
    idx = np.arange(k)
    base = {"none": idx[:0], "alternating": idx[::2], "first": idx[:1], "last": idx[-1:] if k else idx[:0],
            "edges": idx[np.isin(idx, [63, 64, 255, 256])]}
    out = {}
    for name, sel in base.items():
        out[name] = sel
        out["all but " + name] = np.setdiff1d(idx, sel)
    return out


def pattern_names():
    return list(present_patterns(4).keys())


def filter_pattern_case(pattern, split):
    """rows of every length of FILTER_LENGTHS and one above the split cap, disjoint; the other side holds the hashes of `pattern` of
    every row and a few hashes no row holds -> (rows, one sketch, partner rows)"""
    rows = disjoint_rows(FILTER_LENGTHS + [split + 300], 31)
    strangers = pool(40, 32)
    strangers = strangers[~np.isin(strangers, np.concatenate(rows))]
    partners = [np.union1d(row[present_patterns(len(row))[pattern]], strangers[r::len(rows)]).astype(np.uint64) for r, row in enumerate(rows)]
    one = np.unique(np.concatenate(partners)).astype(np.uint64)
    return rows, one, partners


def one_sketch_edge_cases():
    "-> [(name, rows, other)]: the other sketch empty, of one hash, below the rows, and ending below a row's largest"
    rows = disjoint_rows([300, 1, 0, 70], 33)
    a = rows[0]
    low = u64([1, 2, 3])
    assert int(a[0]) > 3
    return [
        ("empty", rows, u64([])),
        ("a row's first hash", rows, a[:1].copy()),
        ("a row's last hash", rows, a[-1:].copy()),
        ("the last row's last hash", rows, rows[3][-1:].copy()),
        ("wholly below the smallest", rows, low),
        # ends inside row 0: every hash of the rows above other's largest is absent without a lookup
        ("wholly below the largest", rows, np.union1d(low, a[:150:3]).astype(np.uint64)),
        ("hash zero and the largest", [u64([0, 7, U64_MAX]), u64([0]), u64([U64_MAX]), u64([5])], u64([0, U64_MAX])),
    ]


def bucket_cases():
    """-> [(k, rows, other)]: an other sketch of k = 3, 4, 7, 8, 9 hashes that fall into ONE bucket of its index (the record's three
    inline hashes, the quad behind them, the binary search): even numbers above 2^50 + 2^40; the rows hold them and the odd numbers
    between them."""
    out = []
    base = (1 << 50) + (1 << 40)
    for k in (3, 4, 7, 8, 9):
        other = u64([base + 2 * i for i in range(k)])
        rows = [u64([base + i for i in range(-3, 2 * k + 3)]), u64([base + 2 * i for i in range(k)]), u64([base + 2 * i + 1 for i in range(k)]),
                u64([5, base + 2 * (k - 1)])]
        out.append((k, rows, other))
    return out


def partner_cases(lds_cap):
    "-> (rows, partners): partner rows empty, shorter, longer, equal, and above the LDS staging cap (with rows shorter and longer than it)"
    p = pool(3 * lds_cap + 4000, 35)
    rng = np.random.default_rng(36)

    def pick(k):
        return np.sort(rng.choice(p, size=k, replace=False))
    rows = [pick(300), pick(300), pick(40), pick(500), pick(0), pick(200), pick(lds_cap + 700), pick(lds_cap), pick(1)]
    partners = [pick(0), pick(50), pick(900), rows[3].copy(), pick(100), pick(lds_cap + 1), pick(lds_cap + 500), pick(lds_cap), pick(lds_cap + 1)]
    return rows, partners
