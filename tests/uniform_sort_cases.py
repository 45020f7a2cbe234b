"""Inputs of the uniform sort's tests (sourmash_amd/csrc/uniform_sort.hip): the same seeded key arrays go through the host emulation
(tests/test_uniform_sort_core_cpu.py, which also proves that the plan's own rule keeps the uniform ones inside their leaves) and
through the kernels (tests/test_gpu_uniform_sort.py).  Not a test module."""
import collections
import functools

import numpy as np

SMALL_MAX = 16384                 # US_SMALL_MAX
LEAF_CAP = 1024                   # US_LEAF_CAP
MAX_HASH = 18446744073709551      # scaled = 1000
U64_MAX = 0xFFFFFFFFFFFFFFFF
# under MAX_HASH the plan offers 132 leaves (shift 47) up to 798 keys each, then 263 (shift 46): one scatter pass up to here
ONE_PASS_MAX = 132 * 798
NO_FALLBACK, FALLBACK = 0, 1
FORM_SMALL, FORM_ONE_PASS, FORM_TWO_PASS = 1, 2, 3

# name; keys (u64, len = n_max); the count put on the device; thr; whether the call must fall back; the plan's form
Case = collections.namedtuple("Case", "name keys count thr want form")


def uniform(n, thr, seed, again=0.0):
    "n keys uniform on [1, thr]; a share `again` of them are copies of other keys of the array (drawn twice or more)"
    rng = np.random.default_rng(seed)
    keys = rng.integers(1, thr, size=n, dtype=np.uint64, endpoint=True)
    m = int(n * again)
    if m:
        keys[rng.choice(n, m, replace=False)] = keys[rng.integers(0, n, size=m)]
    return keys


def one_full_leaf(extra, seed):
    "140,000 uniform keys outside leaf 5 of the plan's 263 leaves (shift 46) and LEAF_CAP + extra distinct keys inside it"
    keys = uniform(141500, MAX_HASH, seed)
    keys = keys[(keys >> np.uint64(46)) != 5][:140000]
    assert len(keys) == 140000
    full = (np.uint64(5) << np.uint64(46)) + np.arange(LEAF_CAP + extra, dtype=np.uint64) * np.uint64(977)
    keys = np.concatenate([keys, full])
    np.random.default_rng(seed + 1).shuffle(keys)
    return keys


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, keys, want, form, count=None, thr=MAX_HASH):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out.append(Case(name, keys, len(keys) if count is None else count, thr, want, form))
    add("n0", np.zeros(0, dtype=np.uint64), NO_FALLBACK, FORM_SMALL)
    add("n1", uniform(1, MAX_HASH, 1), NO_FALLBACK, FORM_SMALL)
    add("n2", uniform(2, MAX_HASH, 2), NO_FALLBACK, FORM_SMALL)
    add("n2-equal", np.array([7, 7]), NO_FALLBACK, FORM_SMALL)
    add("small-limit", uniform(SMALL_MAX, MAX_HASH, 3, 0.3), NO_FALLBACK, FORM_SMALL)
    add("small-limit+1", uniform(SMALL_MAX + 1, MAX_HASH, 4, 0.3), NO_FALLBACK, FORM_ONE_PASS)
    add("one-pass-limit", uniform(ONE_PASS_MAX, MAX_HASH, 5, 0.3), NO_FALLBACK, FORM_ONE_PASS)
    add("one-pass-limit+1", uniform(ONE_PASS_MAX + 1, MAX_HASH, 6, 0.3), NO_FALLBACK, FORM_TWO_PASS)
    add("2e6-a-third-again", uniform(2_000_000, MAX_HASH, 7, 1 / 3), NO_FALLBACK, FORM_TWO_PASS)
    add("all-64-bits", np.concatenate([uniform(40000, U64_MAX, 8, 0.3), np.array([1, U64_MAX, U64_MAX], dtype=np.uint64)]), NO_FALLBACK,
        FORM_ONE_PASS, thr=U64_MAX)
    add("count-below-small", uniform(5000, MAX_HASH, 9, 0.3), NO_FALLBACK, FORM_SMALL, count=1234)
    add("count-below", uniform(200_000, MAX_HASH, 10, 0.3), NO_FALLBACK, FORM_TWO_PASS, count=123_457)
    add("count-above-small", uniform(5000, MAX_HASH, 11, 0.3), NO_FALLBACK, FORM_SMALL, count=1 << 40)
    add("count-above", uniform(200_000, MAX_HASH, 12, 0.3), NO_FALLBACK, FORM_TWO_PASS, count=200_001)
    add("all-equal-1e5", np.full(100_000, 12345678901234567, dtype=np.uint64), FALLBACK, FORM_ONE_PASS)
    add("leaf-cap+1", one_full_leaf(1, 13), FALLBACK, FORM_TWO_PASS)
    add("leaf-cap", one_full_leaf(0, 13), NO_FALLBACK, FORM_TWO_PASS)
    alt = np.where(np.arange(100_000) % 2 == 0, np.uint64(3), np.uint64(MAX_HASH - 5))
    add("two-values-1e5", alt, FALLBACK, FORM_ONE_PASS)
    add("two-values-1000", alt[:1000], NO_FALLBACK, FORM_SMALL)
    return tuple(out)


def expected(case):
    "-> (sorted distinct keys, their multiplicities) of the keys the call may look at"
    n = min(case.count, len(case.keys))
    return np.unique(case.keys[:n], return_counts=True)
