"""Queries and probes for the query index (csrc/qindex_core.hpp, qindex.hpp) shared by tests/test_qindex_core_cpu.py and
tests/test_gpu_qindex.py, with the expected answer in plain numpy: np.searchsorted on the unpadded query.  Every generator is seeded
with fixed integers.  Nothing here touches the package."""
import numpy as np

U64_MAX = 2**64 - 1
NONE32 = 0xFFFFFFFF
MAX_HASH_1000 = 18446744073709552          # max_hash of scaled = 1000
ALT = 0xAAAAAAAAAAAAAAAA
MAX_BUCKET_BITS = 26


def u64(values):
    return np.array(sorted(set(int(v) for v in values)), dtype=np.uint64)


def geometry(nq, q_max):
    "(shift, buckets) of the table for nq hashes with largest q_max, restated in Python integers"
    bucket_bits = min(MAX_BUCKET_BITS, (nq - 1).bit_length())
    shift = min(max(q_max.bit_length() - bucket_bits, 0), 63)
    buckets = (q_max >> shift) + 1
    if buckets < nq and shift > 0 and nq <= 2**MAX_BUCKET_BITS:
        shift -= 1
        buckets = (q_max >> shift) + 1
    return shift, buckets


def geometry_violations(nq, q_max, shift, buckets):
    "the invariants of a geometry (shift, buckets) reported for nq >= 1 hashes, q_max >= nq - 1; -> list of the broken ones"
    bad = []
    if shift > 63:
        return ["shift <= 63"]
    if buckets != (q_max >> shift) + 1:
        bad.append("buckets == (q_max >> shift) + 1")
    if buckets > 2 * nq + 1:
        bad.append("buckets <= 2 nq + 1")
    if nq <= 2**MAX_BUCKET_BITS and shift > 0 and buckets < nq:
        bad.append("buckets >= nq")
    return bad


def padded(q):
    "the query followed by its 4 readable entries, each the largest hash"
    return np.concatenate([q, np.full(4, q[-1], dtype=np.uint64)])


def expected_positions(q, probes):
    "np.searchsorted on the unpadded query: the position if present, else NONE32"
    pos = np.searchsorted(q, probes)
    hit = pos < len(q)
    hit[hit] = q[pos[hit]] == probes[hit]
    return np.where(hit, pos, NONE32).astype(np.uint32)


def bucket_counts(q):
    shift, buckets = geometry(len(q), int(q[-1]))
    return np.bincount((q >> np.uint64(shift)).astype(np.int64), minlength=buckets), shift, buckets


# ---- the host emulation (tests/native/qindex_emul.cpp) ----------------------------------------------------------------------------
def build_emul(directory, old_geometry=False):
    "compile the emulation with g++ into `directory` and declare its entries"
    import ctypes as C
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    so_path = os.path.join(str(directory), "libqindex_emul_old.so" if old_geometry else "libqindex_emul.so")
    flags = ["-DQINDEX_EMUL_OLD_GEOMETRY"] if old_geometry else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", *flags, "-o", so_path,
                           os.path.join(here, "native", "qindex_emul.cpp")])
    so = C.CDLL(so_path)
    so.emul_qindex_geometry.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    so.emul_qindex_geometry.restype = None
    so.emul_qindex_geometry_many.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    so.emul_qindex_geometry_many.restype = None
    so.emul_qindex_build.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    so.emul_qindex_build.restype = None
    so.emul_qindex_find.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    so.emul_qindex_find.restype = C.c_int64
    return so


def emul_geometry(so, nq, q_max):
    import ctypes as C
    shift, buckets = C.c_uint32(), C.c_uint32()
    so.emul_qindex_geometry(nq, q_max, C.byref(shift), C.byref(buckets))
    return shift.value, buckets.value


def emul_find(so, q, probes, form):
    "-> (positions, reads out of bounds) of the emulation's lookup of every probe; form 0 table, 1 record, 2 split record"
    qp = padded(q)
    probes = np.ascontiguousarray(probes, dtype=np.uint64)
    out = np.full(len(probes), 0xDEADBEEF, dtype=np.uint32)
    bad = so.emul_qindex_find(qp.ctypes.data, len(q), probes.ctypes.data, len(probes), form, out.ctypes.data)
    return out, bad


FORMS = {"table": 0, "record": 1, "split": 2}


# ---- query families --------------------------------------------------------------------------------------------------------------
def family_a_values():
    vals = [0, 1, ALT, U64_MAX]
    for b in range(1, 64):
        vals += [2**b - 1, 2**b]
    return sorted(set(vals))


FAMILY_A_CALLERS = (0, 2**63, ALT, U64_MAX)          # the four one-hash queries that go through the real callers


def family_a():
    "one hash"
    return [(f"A-{v:#x}", u64([v])) for v in family_a_values()]


def family_b():
    "two to five hashes"
    spread = [3, 2**17 + 5, 2**40 + 2**13, 2**62 + 12345, 2**64 - 7]
    return [("B-ends", u64([0, U64_MAX])), ("B-low", u64([0, 1])), ("B-mid", u64([2**63 - 1, 2**63])),
            ("B-high", u64([U64_MAX - 1, U64_MAX])), ("B-spread", u64(spread))]


def family_c():
    "dense: base + arange(n), shift 0 or nearly"
    out = []
    for n in (255, 256, 257, 4096):
        for tag, base in (("0", 0), ("2^40", 2**40), ("top", 2**64 - n)):
            out.append((f"C-{n}-{tag}", np.arange(n, dtype=np.uint64) + np.uint64(base)))
    return out


FAMILY_D_RUNS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 300)


def _family_d_one(c, seed):
    """3,000 uniform 54-bit hashes with four runs of c consecutive integers planted: at the start of a bucket, straddling a bucket
    boundary, at the start of bucket 0 (hash 0 included), and ending exactly at q_max."""
    rng = np.random.default_rng(seed)
    base = np.unique(rng.integers(1, 2**54, size=3000, dtype=np.uint64))
    q_max = int(base[-1])
    shift, _ = geometry(len(base) + 4 * c - 1, q_max)
    base = base[((base >> np.uint64(shift)) < np.uint64(q_max >> shift)) | (base == np.uint64(q_max))]   # q_max alone in its bucket
    shift, buckets = geometry(len(base) + 4 * c - 1, q_max)          # (q_max itself is in the base and in the last run)
    counts = np.bincount((base >> np.uint64(shift)).astype(np.int64), minlength=buckets)
    # two pairs of neighbouring empty buckets, away from both ends: planted counts are then exact
    empty = [b for b in range(2, buckets - 2) if counts[b] == 0 and counts[b - 1] == 0]
    b_start, b_straddle = empty[len(empty) // 3], empty[2 * len(empty) // 3]
    assert b_straddle - b_start > 2 and c <= 2**shift
    runs = [np.arange(c, dtype=np.uint64) + np.uint64(b_start << shift),
            np.arange(c, dtype=np.uint64) + np.uint64((b_straddle << shift) - (c + 1) // 2),
            np.arange(c, dtype=np.uint64),
            np.arange(c, dtype=np.uint64) + np.uint64(q_max - c + 1)]
    q = np.unique(np.concatenate([base] + runs))
    assert int(q[-1]) == q_max and geometry(len(q), q_max) == (shift, buckets), "planting moved the geometry"
    got, _, _ = bucket_counts(q)
    assert got[b_start] == c and got[b_straddle - 1] == (c + 1) // 2 and got[b_straddle] == c - (c + 1) // 2
    assert got[0] >= c and got[buckets - 1] >= c and int(q[0]) == 0
    return q


def family_d():
    "bucket fills: buckets of every count 0 .. 9, of 16 and of 300 hashes, full buckets at both ends of the query"
    out = [(f"D-{c}", _family_d_one(c, 400 + c)) for c in FAMILY_D_RUNS]
    seen, last = set(), set()
    for _, q in out:
        counts, _, buckets = bucket_counts(q)
        seen |= set(counts.tolist())
        last.add(int(counts[buckets - 1]))
    assert set(range(10)) <= seen and max(seen) >= 300, sorted(seen)
    # the last bucket is where the loads after a full bucket run into the padding: one hash (the table form's four from nq - 1),
    # exactly four (the record form's second load starts at nq - 1), and eight or more (the binary search ends at nq)
    assert {1, 4} <= last and max(last) >= 8, sorted(last)
    return out


def family_e():
    """uniform random: nq hashes below 2^bits (every value of that width where 2^bits <= nq, which is then a dense query), and the
    scaled = 1000 shape: 54 bits with q_max <= MAX_HASH_1000"""
    out = []
    for i, nq in enumerate((1000, 2**10 - 1, 2**10, 2**10 + 1, 2**13 + 1)):
        for k, bits in enumerate((10, 24, 54, 64)):
            rng = np.random.default_rng(5000 + 10 * i + k)
            if 2**bits <= nq:
                q = np.arange(2**bits, dtype=np.uint64)
            else:
                top = MAX_HASH_1000 + 1 if bits == 54 else 2**bits
                pool = set()
                while len(pool) < nq:
                    draw = rng.integers(0, top, size=2 * nq, dtype=np.uint64, endpoint=False) if top < 2**64 else \
                        rng.integers(0, U64_MAX, size=2 * nq, dtype=np.uint64, endpoint=True)
                    pool |= set(draw.tolist())
                q = np.array(sorted(pool), dtype=np.uint64)
                q = np.sort(rng.choice(q, size=nq, replace=False))
            out.append((f"E-{nq}-{bits}", q))
    return out


def family_f():
    "a query that holds both 0 and 2^64 - 1"
    rng = np.random.default_rng(77)
    body = rng.integers(0, U64_MAX, size=500, dtype=np.uint64, endpoint=True)
    return [("F", np.unique(np.concatenate([body, np.array([0, U64_MAX], dtype=np.uint64)])))]


def family_g():
    "one crowded bucket under a large shift"
    ten = np.arange(10, dtype=np.uint64)
    return [("G-dense", ten + np.uint64(2**63)), ("G-2^40", ten * np.uint64(2**40) + np.uint64(2**63))]


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f, "G": family_g}


def all_cases():
    out = []
    for name in sorted(FAMILIES):
        out += FAMILIES[name]()
    return out


# ---- probes ----------------------------------------------------------------------------------------------------------------------
def probes_for(q, seed=9):
    """What a query is asked: every hash of it and its neighbours, both ends of every bucket (of 4,096 random ones where there are
    more), the fixed values where widths and signs change, 1,000 uniform values up to q_max and 1,000 over 64 bits."""
    rng = np.random.default_rng(seed)
    q_max = int(q[-1])
    shift, buckets = geometry(len(q), q_max)
    vals = [q, q[q > 0] - np.uint64(1), q[q < np.uint64(U64_MAX)] + np.uint64(1)]
    b = np.arange(buckets, dtype=np.uint64) if buckets <= 4096 else \
        np.unique(np.concatenate([rng.integers(0, buckets, size=4094, dtype=np.uint64), np.array([0, buckets - 1], dtype=np.uint64)]))
    edges = b << np.uint64(shift)
    vals += [edges, edges[edges > 0] - np.uint64(1)]
    fixed = [0, 1, q_max, 2**63 - 1, 2**63, U64_MAX] + ([q_max + 1] if q_max < U64_MAX else [])
    vals.append(np.array(fixed, dtype=np.uint64))
    vals.append(rng.integers(0, q_max, size=1000, dtype=np.uint64, endpoint=True))
    vals.append(rng.integers(0, U64_MAX, size=1000, dtype=np.uint64, endpoint=True))
    probes = np.concatenate(vals)
    rng.shuffle(probes)                          # neighbouring lanes ask unrelated questions
    return probes


# ---- a database for the real callers -----------------------------------------------------------------------------------------------
def caller_database(q, seed=31):
    """300 rows around the query q: 250 one-hash rows drawn from its probe set (a count is then a membership bit) and 50 ragged rows of
    0 .. 700 hashes, half of them the query's (as far as it has that many).  Rows 251 and 252 are duplicates (a tie), row 253 is
    empty, row 254 is the whole query."""
    rng = np.random.default_rng(seed)
    probes = np.unique(probes_for(q, seed))
    rows = [probes[i:i + 1].copy() for i in rng.choice(len(probes), size=250, replace=len(probes) < 250)]
    rows[0], rows[1], rows[2] = q[:1].copy(), q[-1:].copy(), np.array([0], dtype=np.uint64)
    for _ in range(50):
        n = int(rng.integers(0, 701))
        own = rng.choice(q, size=min(n // 2, len(q)), replace=False)
        other = rng.choice(probes, size=min(n - len(own), len(probes)), replace=False)
        rows.append(np.unique(np.concatenate([own, other])))
    rows[252] = rows[251].copy()
    rows[253] = np.zeros(0, dtype=np.uint64)
    rows[254] = q.copy()
    return rows


def membership_counts(q, rows):
    return np.array([int(np.isin(r, q).sum()) for r in rows], dtype=np.int64)
