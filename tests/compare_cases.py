"""Collections for the all-pairs compare family (csrc/compare_core.hpp; compare.hip, compare_ext.hip, abund_pairs.hip) shared by
tests/test_compare_core_cpu.py (the host emulation, tests/native/compare_core_emul.cpp) and tests/test_gpu_compare_edges.py (the
kernels), with the expected matrices in plain numpy.  Every generator is seeded with fixed integers; every case is small.  Nothing
here touches the package."""
import os
import subprocess

import numpy as np

U64_MAX = 2**64 - 1
HERE = os.path.dirname(os.path.abspath(__file__))

# the geometry the cases aim at (csrc/compare_core.hpp)
SLICE_LEN_FEW_TILES = 1024      # cmp_pick_slice_len below 512 tiles
XSLICE_SMALL = 1700             # cmp_ext_slice_len below 16,384 tiles
ZMAX = 16
AP_T, AP_CHUNK, AP_INLINE, SM_CAP = 64, 4096, 16, 2048


def _pool(seed, size, top=2**62):
    rng = np.random.default_rng(seed)
    return np.unique(rng.integers(1, top, size=size, dtype=np.int64).astype(np.uint64))


def _rows_from(pool, lengths, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(pool, size=int(k), replace=False)) for k in lengths]


# ---- expected values ---------------------------------------------------------------------------------------------------------------
def common_matrix(sk):
    "u32 |A ∩ B| for every pair, the diagonal a row's size"
    n = len(sk)
    out = np.zeros((n, n), dtype=np.uint32)
    for i in range(n):
        out[i, i] = len(sk[i])
        for j in range(i + 1, n):
            out[i, j] = out[j, i] = len(np.intersect1d(sk[i], sk[j], assume_unique=True))
    return out


def num_reference(sk, nums):
    """bottom-k (minhash.rs:593-621): merge both into a sketch truncated to the LOWER index's num, intersect A ∩ B with it.
    -> common, union size, jaccard; the diagonal as the library writes it: the row's size, min(size, num), 1.0"""
    n = len(sk)
    common, usize, jac = np.zeros((n, n), np.uint32), np.zeros((n, n), np.uint32), np.ones((n, n), np.float64)
    for i in range(n):
        common[i, i], usize[i, i] = len(sk[i]), min(len(sk[i]), int(nums[i]))
        for j in range(i + 1, n):
            merged = np.union1d(sk[i], sk[j])[:int(nums[i])]
            c = len(np.intersect1d(np.intersect1d(sk[i], sk[j], assume_unique=True), merged, assume_unique=True))
            common[i, j] = common[j, i] = c
            usize[i, j] = usize[j, i] = len(merged)
            jac[i, j] = jac[j, i] = np.float64(c) / np.float64(max(1, len(merged)))
    return common, usize, jac


def abund_reference(sk, ab):
    "common and the u64 (wrapping) sum of abundance products over the common hashes; the diagonal: size and sum of squares"
    n = len(sk)
    common, prod = np.zeros((n, n), np.uint32), np.zeros((n, n), np.uint64)
    with np.errstate(over="ignore"):
        for i in range(n):
            common[i, i] = len(sk[i])
            prod[i, i] = np.sum(ab[i] * ab[i], dtype=np.uint64)
            for j in range(i + 1, n):
                _, ia, ib = np.intersect1d(sk[i], sk[j], assume_unique=True, return_indices=True)
                common[i, j] = common[j, i] = len(ia)
                prod[i, j] = prod[j, i] = np.sum(ab[i][ia] * ab[j][ib], dtype=np.uint64)
    return common, prod


# ---- scaled: (name, sketches) and the launch forms ---------------------------------------------------------------------------------
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)
STRIP = (5, 21)                 # rows [5, 21) of 33
BLOCKS = (1, 2)                 # 16-row tiles 1, 3, ...


def long_row_case(long_len, seed, n=17, slice_len=SLICE_LEN_FEW_TILES, short=64):
    """one row of long_len hashes among rows of `short`; every pivot value of the long row's slices is present in other rows too (a
    common hash on a slice boundary is counted once)"""
    rng = np.random.default_rng(seed)
    long = _pool(seed, long_len + 500)[:long_len]
    assert len(long) == long_len
    zt = min(ZMAX, -(-long_len // slice_len))
    pivots = np.array([long[z * long_len // zt] for z in range(1, zt)], dtype=np.uint64)
    others = np.setdiff1d(np.concatenate([long, _pool(seed + 1, 4000)]), pivots)
    rows = []
    for i in range(n - 1):                                    # every other row holds all the pivots
        own = pivots if i % 2 == 0 else pivots[:0]
        rows.append(np.unique(np.concatenate([own, rng.choice(others, size=short - len(own), replace=False)])))
    rows.insert(3, long)
    assert all(len(r) == short for i, r in enumerate(rows) if i != 3) and len(pivots) == zt - 1
    assert sum(int(np.isin(pivots, r).all()) for r in rows) == 1 + (n - 1 + 1) // 2
    return rows, zt


def scaled_cases():
    out = []
    pool = _pool(1, 300)
    for k, n in enumerate((1, 15, 16, 17, 31, 32, 33, 49)):
        rng = np.random.default_rng(100 + n)
        lengths = list(LENGTHS) * 7
        rng.shuffle(lengths)
        out.append((f"ragged-{n}", _rows_from(pool, lengths[:n], 200 + k)))
    out.append(("all-shared-33", [pool[:129].copy() for _ in range(33)]))
    wide = _pool(2, 33 * 129)
    out.append(("none-shared-33", [wide[i * 129:(i + 1) * 129] for i in range(33)]))
    for long_len, want_zt in ((1025, 2), (2049, 3), (16385, 16)):
        rows, zt = long_row_case(long_len, 300 + long_len)
        assert zt == want_zt
        out.append((f"long-{long_len}", rows))
    # 0 is an ordinary key; 2^64 - 1 (possible with scaled = 1) stays out of the table and is counted out of band
    ends = _rows_from(pool, [70, 64, 1, 0, 130, 65, 64, 129, 3, 64, 200, 64, 63, 64, 65, 1, 90, 64], 400)
    for i, r in enumerate(ends):
        extra = ([0] if i % 2 == 0 else []) + ([U64_MAX] if i % 3 == 0 else [])
        ends[i] = np.unique(np.concatenate([r, np.array(extra, dtype=np.uint64)]))
    out.append(("ends-18", ends))
    return out


def scaled_forms(n):
    "(form, row_lo, row_hi, rb_first, rb_stride, rb_count) a collection of n sketches is run in"
    forms = [("whole", 0, n, 0, 1, 0)]
    if n > STRIP[1]:
        forms.append(("strip", STRIP[0], STRIP[1], 0, 1, 0))
    owned = len(range(BLOCKS[0], (n + 15) // 16, BLOCKS[1]))
    if owned:
        forms.append(("blocks", 0, n, BLOCKS[0], BLOCKS[1], owned))
    return forms


def expected_for_form(want, form):
    "(rows of the full matrix the form's output rows are, mask of the entries the form defines)"
    kind, lo, hi, first, stride, count = form
    n = want.shape[0]
    if kind == "whole":
        return want, np.ones_like(want, dtype=bool)
    if kind == "strip":
        return want[lo:hi], np.ones((hi - lo, n), dtype=bool)
    rows = np.zeros((count * 16, n), dtype=want.dtype)
    mask = np.zeros((count * 16, n), dtype=bool)
    for t in range(count):
        for r in range(16):
            g = (first + t * stride) * 16 + r
            if g < n:
                rows[t * 16 + r] = want[g]
                mask[t * 16 + r, g:] = True                  # on or above the diagonal
    return rows, mask


# ---- bottom-k ----------------------------------------------------------------------------------------------------------------------
def num_cases():
    """(name, sketches, nums).  nums drawn from {1, 64, 65, the row's length}, different per sketch.  In the collections of 15 and
    more, rows 0 / 1 and rows 2 / 3 are identical pairs with num 64 and 65: the cut falls after their 64th / 65th common hash, in
    whichever round the tile's bound puts that.  The two collections of two sketches pin the position: the tile holds nothing but
    one identical pair of 200 hashes, so a round is exactly 64 steps, each consuming a hash of both -- with num 64 the cut falls on
    the first round's last step, with num 65 inside the second round."""
    out = []
    pool = _pool(5, 600)
    for n in (1, 15, 16, 17, 33):
        rng = np.random.default_rng(500 + n)
        rows = _rows_from(pool, rng.choice([0, 1, 63, 64, 65, 130, 200], size=n), 600 + n)
        nums = []
        for i, r in enumerate(rows):
            nums.append([1, 64, 65, max(1, len(r))][(i + n) % 4])
        if n >= 15:
            rows[0] = rows[1] = pool[:200].copy()
            rows[2] = rows[3] = pool[100:300].copy()
            nums[0], nums[2] = 64, 65
        out.append((f"num-{n}", rows, np.array(nums, dtype=np.uint32)))
    for what, num in (("last-step", 64), ("inside", 65)):
        out.append((f"num-2-{what}", [pool[:200].copy(), pool[:200].copy()], np.array([num, 200], dtype=np.uint32)))
    return out


# ---- abundances --------------------------------------------------------------------------------------------------------------------
def _abunds(rows, wide, seed):
    rng = np.random.default_rng(seed)
    ab = []
    for i, r in enumerate(rows):
        a = (r % np.uint64(13)) * (r % np.uint64(5)) + np.uint64(1 + i % 3)
        if wide and len(a):
            a = a.copy()
            a[rng.integers(0, len(a))] = np.uint64(2**32)                      # the first value that needs the wide form
            if i % 4 == 0:
                a = (a << np.uint64(31)) + np.uint64(i)
        ab.append(a.astype(np.uint64))
    return ab


def _plant_wrap(rows, ab, i, j):
    "a hash common to rows i and j with abundances 2^63 and 2: their product wraps to 0"
    h = np.uint64(2**62 + 12345)
    for r, a in ((i, 2**63), (j, 2)):
        at = int(np.searchsorted(rows[r], h))
        assert at == len(rows[r]) or rows[r][at] != h
        rows[r] = np.insert(rows[r], at, h)
        ab[r] = np.insert(ab[r], at, np.uint64(a))


def walk_cases():
    "(name, sketches, abundances, narrow) for the per-pair walk: a row of 1,701 (two slices) and one of 27,201 (the cap of 16) among rows of 64"
    out = []
    for long_len, want_zt in ((1701, 2), (27201, 16)):
        for wide in (False, True):
            rows, zt = long_row_case(long_len, 700 + long_len, n=17, slice_len=XSLICE_SMALL)
            assert zt == want_zt
            ab = _abunds(rows, wide, 800 + long_len)
            if wide:
                _plant_wrap(rows, ab, 1, 5)
            out.append((f"walk-{long_len}-{'wide' if wide else 'narrow'}", rows, ab, not wide))
    return out


def join_cases():
    "(name, sketches, abundances, narrow) for the join of per-block lists"
    out = []
    pool = _pool(9, 3000)
    for n in (1, 63, 64, 65, 129):
        rng = np.random.default_rng(900 + n)
        rows = _rows_from(pool, rng.choice([0, 1, 2, 40, 64, 300], size=n), 1000 + n)
        if n == 129:                                          # hashes held by 16, 17 and 64 rows of both blocks: the inline limit and the worklist
            for holders, h in ((16, 2**61 + 1), (17, 2**61 + 3), (64, 2**61 + 5)):
                for r in list(range(holders)) + list(range(64, 64 + holders)):
                    rows[r] = np.unique(np.append(rows[r], np.uint64(h)))
        wide = n in (64, 129)
        ab = _abunds(rows, wide, 1100 + n)
        if wide and n > 5:
            _plant_wrap(rows, ab, 1, 5)
        out.append((f"join-{n}", rows, ab, not wide))
    # a block list longer than a chunk in which a run of equal hashes straddles entry 4,096 (with one slice per tile)
    rows = [r for r in np.sort(_pool(11, 65 * 79 + 400)[:65 * 79].reshape(79, 65).T.copy(), axis=1)]
    flat = np.sort(np.concatenate(rows[:64]))
    v = flat[AP_CHUNK - 20] + np.uint64(1)
    assert v < flat[AP_CHUNK - 19]
    for r in range(40):
        rows[r] = np.unique(np.append(rows[r], v))
    rows[64] = np.unique(np.append(rows[64], v))
    block = np.sort(np.concatenate(rows[:64]))
    at = np.nonzero(block == v)[0]
    assert len(block) > AP_CHUNK and at[0] < AP_CHUNK <= at[-1] and len(at) == 40
    out.append(("join-straddle-65", rows, _abunds(rows, False, 1200), True))
    # clustered hashes with one far-out maximum: everything but it falls into hash slice 0 of the list build, more entries than the
    # slice merge holds in LDS -- the ranking branch
    low = _pool(12, 9000, top=20_000)
    rows = _rows_from(low, [100] * 70, 1300)
    rows[3] = np.array([2**63 + 12345], dtype=np.uint64)
    rows[69] = np.append(rows[69], np.uint64(2**63 + 12345))
    assert sum(len(r) for r in rows[:64]) - 1 > SM_CAP
    out.append(("join-skewed-70", rows, _abunds(rows, True, 1400), False))
    return out


JOIN_SLICES = (1, 2, 15, 16)


# ---- the path choice, restated ------------------------------------------------------------------------------------------------------
RATE_MERGE_STEPS, MERGE_ROUND_FLOOR, RATE_BIT_WORDS, RATE_PAIR_ATOMICS = 6.0e12, 6.0e-8, 9.5e12, 4.0e9


def path_model(n, total, forced, one_shot):
    "(threshold, t_merge, try the dictionary builder, try the sort builder) in Python floats (IEEE doubles, like the library's)"
    t_merge = max(float(n) * float(total) / RATE_MERGE_STEPS, float(total) / float(n) * MERGE_ROUND_FLOOR)
    threshold = int(float(n) * np.sqrt(np.float64(RATE_PAIR_ATOMICS / (64.0 * RATE_BIT_WORDS))))
    threshold = forced if forced else max(threshold, 1)
    pays = one_shot and not forced
    try_dict = n <= 2 * 2**20 and not (pays and t_merge < 0.1e-3 + float(total) / 4.0e10)
    try_sort = not (pays and t_merge < 0.6e-3 + float(total) / 1.4e9)
    return threshold, t_merge, try_dict, try_sort


def index_accept(n, n_freq, rare_pairs, total, t_merge, forced):
    "(accepted, words of a bit row)"
    words = ((n_freq + 31) // 32 + 31) // 32 * 32 if n_freq else 0
    words &= 0xffffffff
    pairs = 0.5 * float(n) * float(n)
    t_index = 0.5 * (pairs * float(words) / RATE_BIT_WORDS + 2.0 * float(rare_pairs) / RATE_PAIR_ATOMICS) + float(total) / 2.0e10
    refuse = (t_index > t_merge and not forced) or float(n) * words * 4.0 > 8.0 * 2**30
    return (not refuse), words


# ---- the host emulation -------------------------------------------------------------------------------------------------------------
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build_emul(directory, sanitize=False):
    exe = os.path.join(str(directory), "compare_core_emul_san" if sanitize else "compare_core_emul")
    flags = ["-O1", "-g", *SAN_FLAGS] if sanitize else ["-O2"]
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "native", "compare_core_emul.cpp")])
    return exe


def run_emul(exe, directory, mode, sketches=(), abunds=None, nums=None, par=(), table=None):
    "-> the result words (u64) of one run of the emulation; raises with the program's own message when it finds something wrong"
    n = len(table) if table is not None else len(sketches)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    if table is None:
        offsets[1:] = np.cumsum([len(s) for s in sketches])
    total = int(offsets[-1])
    head = [mode, n, total, int(abunds is not None), int(nums is not None)] + (list(par) + [0] * 8)[:8]
    parts = [np.array(head, dtype=np.uint64)]
    if table is not None:
        parts.append(np.ascontiguousarray(table, dtype=np.uint64).ravel())
    else:
        parts.append(offsets)
        parts += [np.asarray(s, dtype=np.uint64) for s in sketches]
        if abunds is not None:
            parts += [np.asarray(a, dtype=np.uint64) for a in abunds]
        if nums is not None:
            parts.append(np.asarray(nums, dtype=np.uint64))
    case, result = os.path.join(str(directory), "case.bin"), os.path.join(str(directory), "result.bin")
    np.concatenate(parts).tofile(case)
    p = subprocess.run([exe, case, result], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: "), (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    return np.fromfile(result, dtype=np.uint64)
