"""CPU checks of the flattened slice walk (csrc/slice_walk_core.hpp: flattened position -> slice, and the lanes of a step that belong to
a slice) compiled for the host (tests/native/slice_walk_emul.cpp), against the plain concatenation of the slices; and of the gather
rounds' pick key and stop rule (csrc/gather_key.hpp) against the reference's rules.  None of this needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "slice_walk_emul.cpp")
EPWS = (2, 16)                      # APPLY_EPW of gather.hip; BR_EPW of gather_build.hip and DX_EPW of dictindex.hip


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("slice_walk") / "libslice_walk_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so_path, SRC])
    so = C.CDLL(so_path)
    so.emul_slice_walk.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    so.emul_slice_walk.restype = C.c_int64
    so.emul_gather_key.argtypes = [C.c_uint64, C.c_uint64]
    so.emul_gather_key.restype = C.c_uint64
    so.emul_gather_key_index.argtypes = [C.c_uint64]
    so.emul_gather_key_index.restype = C.c_uint64
    so.emul_gather_stops.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    so.emul_gather_stops.restype = C.c_int
    return so


def split(total, parts, rng):
    "`parts` lengths that sum to `total`, about a third of them empty"
    cuts = np.sort(rng.integers(0, total + 1, size=parts - 1))
    n = np.diff(np.concatenate([[0], cuts, [total]]))
    for i in np.nonzero(rng.random(parts - 1) < 0.33)[0]:      # fold a slice into its right neighbour: the total stays
        n[i + 1] += n[i]
        n[i] = 0
    return [int(v) for v in n]


def slice_sets(epw):
    """name -> (lengths, first indices or None).  A kernel walks `epw` slices as one list, so what a name promises holds inside a group
    of epw consecutive slices: every set is a whole number of groups unless it says otherwise."""
    rng = np.random.default_rng(epw)
    pad = lambda n: n + [0] * (-len(n) % epw)
    sets = {
        "all empty": ([0] * epw, None),
        "three empty groups": ([0] * (3 * epw), None),
        "one slice of 1": ([1], None),
        "one slice of 1, last of its group": ([0] * (epw - 1) + [1], None),
        "starts at lane 63 of a step": (pad([63, 10]), None),
        "starts at lane 63 of the second step": (pad([127, 2]), None),
        "spans three steps": (pad([10, 150]), None),
        "spans three steps exactly": (pad([64, 192]), None),
        "ends at 64": (pad([30, 34]), None),
        "one slice of 64": (pad([64]), None),
        "ends at 256": (pad([100, 156]), None),
        "one slice of 256": (pad([256]), None),
        "ends at 257": (pad([200, 57]), None),
        "one slice of 257": (pad([257]), None),
        "257 then 1": (pad([257, 1]), None),
        "a short last group": ([5] * (epw + 1), None),
    }
    if epw == 16:
        sets["empties before, between and after"] = ([0, 0, 5, 0, 64, 0, 0, 7, 0, 0, 0, 0, 130, 0, 0, 0], None)
    else:
        sets["empties before, between and after"] = ([0, 5, 0, 0, 64, 0, 7, 0, 0, 130, 0, 0], None)
    for total in (0, 1, 63, 64, 65, 255, 256, 257):
        sets[f"total {total}"] = (split(total, epw, rng), None)
        sets[f"total {total}, last slice"] = ([0] * (epw - 1) + [total], None)
    n = split(300, epw, rng) + split(257, epw, rng)
    sets["first indices above 2^32"] = (n, [2**32 + 2**20 * s for s in range(len(n))])
    across = pad([10, 300]) + n                                     # the first two slices reach across 2^32: a carry into the high word
    sets["first indices around 2^32"] = (across, [2**32 - 3, 2**32 - 100] + [2**32 + 1000 * s for s in range(2, len(across))])
    sets["first indices above 2^40"] = (n, [2**40 + 2**33 * s + 7 for s in range(len(n))])
    return sets


def walk(so, epw, n, lo, hit, ahead):
    n = np.ascontiguousarray(n, dtype=np.uint32)
    lo = np.ascontiguousarray(lo, dtype=np.uint64)
    hit = np.ascontiguousarray(hit, dtype=np.uint8)
    cap = len(hit)
    got_slice, got_index = np.full(cap + 1, 0xDEADBEEF, dtype=np.uint32), np.full(cap + 1, 0xDEADBEEF, dtype=np.uint64)
    got_hits = np.full(len(n), 2**64 - 1, dtype=np.uint64)
    r = so.emul_slice_walk(epw, lo.ctypes.data, n.ctypes.data, len(n), hit.ctypes.data, cap, ahead, got_slice.ctypes.data, got_index.ctypes.data,
                           got_hits.ctypes.data)
    assert got_slice[cap] == 0xDEADBEEF and got_index[cap] == 0xDEADBEEF
    return r, got_slice[:cap], got_index[:cap], got_hits


@pytest.mark.parametrize("ahead", [1, 4])
@pytest.mark.parametrize("epw", EPWS)
def test_the_walk_is_the_concatenation(emul, epw, ahead):
    """every flattened position is given exactly the (slice, offset) that concatenating the slices gives, in that order, and the hit
    counts of the steps add up to every slice's own hits, for random hit patterns, none and all"""
    rng = np.random.default_rng(100 * epw + ahead)
    for name, (n, lo) in slice_sets(epw).items():
        if lo is None:
            lo = [10_000 * s + 17 for s in range(len(n))]
        want_slice = np.repeat(np.arange(len(n), dtype=np.uint32), n)
        want_index = np.concatenate([np.arange(l, l + k, dtype=np.uint64) for l, k in zip(lo, n)] + [np.zeros(0, dtype=np.uint64)])
        total = int(sum(n))
        for hit in (rng.integers(0, 2, size=total), rng.random(total) < 0.05, np.zeros(total), np.ones(total)):
            hit = np.asarray(hit, dtype=np.uint8)
            r, got_slice, got_index, got_hits = walk(emul, epw, n, lo, hit, ahead)
            assert r == total, (name, r)
            assert np.array_equal(got_slice, want_slice), name
            assert np.array_equal(got_index, want_index), name
            want_hits = np.bincount(want_slice, weights=hit, minlength=len(n)).astype(np.uint64)
            assert np.array_equal(got_hits, want_hits), (name, got_hits.tolist(), want_hits.tolist())


@pytest.mark.parametrize("epw", EPWS)
def test_slice_sets_hold_what_they_promise(epw):
    sets = slice_sets(epw)
    groups = lambda n: [n[i:i + epw] for i in range(0, len(n), epw)]
    ends = lambda g: set(np.cumsum(g).tolist())
    starts = lambda g: set((np.cumsum(g) - np.array(g))[np.array(g) > 0].tolist())
    assert all(sum(n) == 0 for n in (sets["all empty"][0], sets["three empty groups"][0]))
    assert {sum(g) for name, (n, _) in sets.items() if name.startswith("total ") for g in groups(n)} == {0, 1, 63, 64, 65, 255, 256, 257}
    assert 63 in starts(sets["starts at lane 63 of a step"][0][:epw]) and 127 in starts(sets["starts at lane 63 of the second step"][0][:epw])
    g = sets["spans three steps"][0][:epw]
    assert g[1] > 0 and (g[0] // 64, (g[0] + g[1] - 1) // 64) == (0, 2)
    for end in (64, 256, 257):
        assert end in ends(sets[f"ends at {end}"][0][:epw]) and sets[f"one slice of {end}"][0][0] == end
    g = sets["empties before, between and after"][0]
    assert g[0] == 0 and g[-1] == 0 and any(a > 0 and b == 0 and c > 0 for a, b, c in zip(g, g[1:], g[2:]))
    assert min(sets["first indices above 2^32"][1]) >= 2**32
    lo, n = sets["first indices around 2^32"][1], sets["first indices around 2^32"][0]
    assert lo[0] < 2**32 < lo[0] + n[0] and lo[1] < 2**32 < lo[1] + n[1]


def test_emulation_under_sanitizers_as_a_program_of_its_own(tmp_path):
    "the header's own arithmetic with -fsanitize=address,undefined: no shift by 64 in a step mask, no read or write past a vector's end"
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + probe.stderr.strip().splitlines()[-1])
    exe = str(tmp_path / "slice_walk_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSLICE_WALK_EMUL_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok: ") and " slice sets" in out.stdout, out.stdout + out.stderr


# ---- the pick key and the stop rule ----------------------------------------------------------------------------------------------------
def reference_peek_stops(best_overlap, query_left, n_threshold_hashes):
    """CounterGather.peek (index/__init__.py) with calc_threshold_from_bp (search.py:15-37), in hashes: an empty counter, an empty
    query, a threshold the remaining query cannot reach (threshold > 1.0 raises, peek returns nothing), a best match below it"""
    if best_overlap == 0:                                           # `if not counter` (rows at zero have been dropped)
        return True
    if query_left == 0:                                             # `if not cur_query_mh`
        return True
    if n_threshold_hashes and n_threshold_hashes / query_left > 1.0:
        return True
    return best_overlap < n_threshold_hashes


def test_stop_rule_is_the_reference_peek(emul):
    values = [0, 1, 2, 3, 49, 50, 51, 2**31, 2**32 - 1]
    seen = set()
    for count in values:
        for qlen in values:
            for thr in values:
                key = emul.emul_gather_key(count, 12345) if count else 0
                want = reference_peek_stops(count, qlen, thr)
                assert bool(emul.emul_gather_stops(key, qlen, thr)) == want, (count, qlen, thr)
                seen.add((count == 0, qlen == 0, qlen < thr, count < thr))
    # each of the four conditions fires alone somewhere (the overlap never exceeds what is left of the query in a real gather, so
    # "unattainable" cannot fire without "below the threshold" there; here it can)
    assert {(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
            (False, False, False, False)} <= seen


def test_key_round_trip_and_order(emul):
    for index in (0, 1, 2**31, 2**32 - 2, 2**32 - 1):
        for count in (1, 2**16, 2**32 - 1):
            key = emul.emul_gather_key(count, index)
            assert emul.emul_gather_key_index(key) == index and key >> 32 == count and key != 0
    k = emul.emul_gather_key
    assert k(5, 3) > k(5, 4) > k(4, 0)                              # the larger overlap, then the row inserted first
    assert k(1, 2**32 - 1) == 1 << 32
