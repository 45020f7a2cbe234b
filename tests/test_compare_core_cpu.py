"""CPU checks of the all-pairs compare family's rules (csrc/compare_core.hpp) compiled for the host: tests/native/compare_core_emul.cpp
walks the collections of tests/compare_cases.py as the kernels do -- plan, slices, rounds, table, nibble counters; the bottom-k and
abundance walks; the list build and the join -- with the core's functions alone, and the results are held to numpy.  The path choice
of a compare() is held to its formulas restated in Python.  None of this needs a GPU."""
import os
import subprocess

import numpy as np
import pytest

import compare_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    d = tmp_path_factory.mktemp("compare_core")
    return cc.build_emul(d), d


@pytest.fixture(scope="module")
def references():
    "the numpy matrices, computed once for the plain and the sanitizer run"
    ref = {}
    for name, sk in cc.scaled_cases():
        ref[name] = cc.common_matrix(sk)
    for name, sk, nums in cc.num_cases():
        ref[name] = cc.num_reference(sk, nums)
    for name, sk, ab, _ in cc.walk_cases() + cc.join_cases():
        ref[name] = cc.abund_reference(sk, ab)
    return ref


def check_scaled(exe, d, ref):
    forms_seen = set()
    for name, sk in cc.scaled_cases():
        n = len(sk)
        for form in cc.scaled_forms(n):
            kind, lo, hi, first, stride, count = form
            whole = kind == "whole"
            got = cc.run_emul(exe, d, 0, sk, par=[{"strip": 0, "whole": 1, "blocks": 2}[kind], lo, hi, first, stride, count, int(whole)])
            want, mask = cc.expected_for_form(ref[name], form)
            counts = got[:want.size].reshape(want.shape)
            assert np.array_equal(counts[mask], want[mask].astype(np.uint64)), (name, form)
            if whole:                                          # jaccard_scaled, bit for bit
                jac = got[want.size:].view(np.float64).reshape(n, n)
                sizes = np.array([len(s) for s in sk], dtype=np.float64)
                union = np.maximum(sizes[:, None] + sizes[None, :] - want, 1.0)
                expect = np.where(np.eye(n, dtype=bool), 1.0, want / union)
                assert np.array_equal(jac.view(np.uint64), expect.view(np.uint64)), name
            forms_seen.add(kind)
    assert forms_seen == {"whole", "strip", "blocks"}


def check_num(exe, d, ref):
    for name, sk, nums in cc.num_cases():
        n = len(sk)
        got = cc.run_emul(exe, d, 1, sk, nums=nums).reshape(3, n, n)
        common, usize, jac = ref[name]
        assert np.array_equal(got[0], common.astype(np.uint64)), name
        assert np.array_equal(got[1], usize.astype(np.uint64)), name
        assert np.array_equal(got[2], jac.view(np.uint64)), name


def check_abund(exe, d, ref, cases, mode, pars):
    for name, sk, ab, narrow in cases:
        n = len(sk)
        for par in pars:
            got = cc.run_emul(exe, d, mode, sk, abunds=ab, par=[int(narrow), *par]).reshape(2, n, n)
            common, prod = ref[name]
            assert np.array_equal(got[0], common.astype(np.uint64)), (name, par)
            assert np.array_equal(got[1], prod), (name, par)


def test_scaled_counts_in_all_three_launch_forms(emul, references):
    check_scaled(*emul, references)


def test_bottom_k_rounds(emul, references):
    check_num(*emul, references)


def test_abundance_walk(emul, references):
    check_abund(*emul, references, cc.walk_cases(), 2, [()])


def test_abundance_join(emul, references):
    "plan, cuts, both branches of the slice merge, slice bounds, chunk trim, fixed searches, worklist; every list position once"
    check_abund(*emul, references, cc.join_cases(), 3, [(0,)] + [(z,) for z in cc.JOIN_SLICES])


def test_cases_hold_the_shapes_they_promise():
    names = [c[0] for c in cc.scaled_cases()]
    assert {f"ragged-{n}" for n in (1, 15, 16, 17, 31, 32, 33, 49)} <= set(names) and len(set(names)) == len(names)
    for name, sk in cc.scaled_cases():
        assert all(r.dtype == np.uint64 and (r[1:] > r[:-1]).all() for r in sk), name
    lengths = {len(r) for name, sk in cc.scaled_cases() if name.startswith("ragged") for r in sk}
    assert lengths == set(cc.LENGTHS)
    for name, sk, nums in cc.num_cases():
        assert len(nums) == len(sk) and (nums >= 1).all(), name
    assert {int(v) for _, _, nums in cc.num_cases() for v in nums} >= {1, 64, 65}
    by_name = {c[0]: c for c in cc.walk_cases() + cc.join_cases()}
    assert max(int(a.max()) for a in by_name["walk-1701-narrow"][2]) < 2**32
    assert any((a == np.uint64(2**32)).any() for a in by_name["walk-1701-wide"][2])
    assert any((a == np.uint64(2**63)).any() for a in by_name["walk-27201-wide"][2])
    assert {len(c[1]) for c in cc.join_cases()} >= {1, 63, 64, 65, 129}
    rows = by_name["join-129"][1]
    for holders, h in ((16, 2**61 + 1), (17, 2**61 + 3), (64, 2**61 + 5)):
        for block in (rows[:64], rows[64:128]):
            assert sum(int(np.uint64(h) in r) for r in block) == holders


# ---- the path choice ---------------------------------------------------------------------------------------------------------------
def path_grid():
    "rows (n, total, forced threshold, one_shot, n_freq, rare_pairs)"
    ns = sorted({2, 3, 15, 16, 17, 128, 1000, 2000, 10_000, 2**20, 2**21 - 1, 2**21, 2**21 + 1})
    totals = [0, 1, 2**32 - 1, 2**32]
    rows = []
    for n in ns:
        cap_words = 8 * 2**30 // (4 * n)                       # n * words * 4 on either side of the 8 GiB cap
        freqs = sorted({0, 1, 32 * 32, 32 * 32 + 1, 50_000, max(1, (cap_words - 32) * 32), (cap_words + 32) * 32})
        for total in totals + [5000 * n, 5_000_000]:
            for forced in (0, 8):
                for one_shot in (0, 1):
                    for n_freq in freqs:
                        for rare_pairs in (0, 10_000, 10**9):
                            rows.append((n, total, forced, one_shot, n_freq, rare_pairs))
    return np.array(rows, dtype=np.uint64)


def emul_path(emul, table):
    exe, d = emul
    return cc.run_emul(exe, d, 4, table=table).reshape(len(table), 6)


def test_path_model_and_accept_against_their_formulas(emul):
    table = path_grid()
    got = emul_path(emul, table)
    sides = set()
    for row, g in zip(table.tolist(), got):
        n, total, forced, one_shot, n_freq, rare_pairs = row
        threshold, t_merge, try_dict, try_sort = cc.path_model(n, total, forced, bool(one_shot))
        accept, words = cc.index_accept(n, n_freq, rare_pairs, total, t_merge, bool(forced))
        want = (threshold, int(np.float64(t_merge).view(np.uint64)), int(try_dict), int(try_sort), int(accept), words)
        assert tuple(int(v) for v in g) == want, row
        sides.add(float(n) * words * 4.0 > 8.0 * 2**30)
    assert sides == {True, False} and len(table) > 5000


def test_path_of_the_documented_shapes(emul):
    """DESIGN 4.3 and profiles/r06_compare_small.jsonl: C3 (1,000 x 5,000 of a 50,000 pool) and C4 (10,000) take an index; 1,000 and
    2,000 sketches of 5,000 mostly private hashes take the general kernel.  A shared-pool collection is all bit columns (every
    hash held by a tenth of the sketches, far above the threshold of 0.0026 n); a private one all rare, two holders a hash at most."""
    shapes = {"c3": (1000, 5_000_000, 55_000, 0), "c4": (10_000, 50_000_000, 55_000, 0),
              "private-1000": (1000, 5_000_000, 0, 2 * 250_000), "private-2000": (2000, 10_000_000, 0, 2 * 500_000)}
    table = np.array([(n, total, 0, 1, n_freq, rare) for n, total, n_freq, rare in shapes.values()], dtype=np.uint64)
    got = dict(zip(shapes, emul_path(emul, table).tolist()))
    for name in ("c3", "c4"):
        threshold, _, try_dict, try_sort, accept, words = got[name]
        assert try_dict and accept and words == 1728 and threshold == {"c3": 2, "c4": 25}[name], (name, got[name])
    # mostly private hashes: the dictionary is tried, the sort is not worth starting
    for name in ("private-1000", "private-2000"):
        _, _, try_dict, try_sort, accept, words = got[name]
        assert try_dict and not try_sort, (name, got[name])


# ---- the same program under the sanitizers -----------------------------------------------------------------------------------------
def test_under_the_sanitizers(tmp_path, references):
    "a program of its own with -fsanitize=address,undefined on the same cases: no read past a staged segment, a list or the table"
    exe = cc.build_emul(tmp_path, sanitize=True)
    check_scaled(exe, tmp_path, references)
    check_num(exe, tmp_path, references)
    check_abund(exe, tmp_path, references, cc.walk_cases(), 2, [()])
    check_abund(exe, tmp_path, references, cc.join_cases(), 3, [(0,), (1,), (16,)])
    got = cc.run_emul(exe, tmp_path, 4, table=path_grid()[::7])
    assert len(got) == 6 * len(path_grid()[::7])


def test_one_search_one_slice_rule_one_accept_block():
    "what the family's units may no longer hold: a lower bound, a slice rule or an accept block of their own"
    import re
    src = {f: open(os.path.join(ROOT, "sourmash_amd", "csrc", f)).read()
           for f in ("compare.hip", "compare_ext.hip", "abund_pairs.hip", "pair_ops.hip", "bitindex.hip", "capi_compare.cpp")}
    core = open(os.path.join(ROOT, "sourmash_amd", "csrc", "compare_core.hpp")).read()
    for f, text in src.items():
        assert '#include "compare_core.hpp"' in text, f
        assert not re.search(r"\b(lower_bound\w*|ap_lower_bound)\s*\(const uint64_t\*", text), f      # no definition of a search
        for m in re.finditer(r"if \((\w+)\[mid\] < (\w+)\) lo = mid \+ 1", text):                     # ... and no open loop
            raise AssertionError((f, m.group(0)))
        assert "slice_len - 1) / slice_len" not in text, f
    assert core.count("slice_len - 1) / slice_len") == 1 and len(re.findall(r"\[mid\] < x\) lo = mid \+ 1", core)) == 2
    assert src["capi_compare.cpp"].count("compare_index_accept(") == 1 and "RATE_BIT_WORDS" not in src["capi_compare.cpp"]
    hd = [f for f in os.listdir(os.path.join(ROOT, "sourmash_amd", "csrc")) if f.endswith(".hpp") and
          "define SMG_HD" in open(os.path.join(ROOT, "sourmash_amd", "csrc", f)).read()]
    assert "smg_hd.hpp" in hd and "compare_core.hpp" not in hd
