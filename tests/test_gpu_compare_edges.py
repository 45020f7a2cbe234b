"""GPU parity of the all-pairs compare family at its edges: the collections of tests/compare_cases.py -- tile and round boundaries,
hash-range slices up to the cap, the three launch forms, bottom-k cuts inside and at the end of a round, abundance walks and joins
with runs across the inline limit, the worklist, the chunk boundary and the ranking branch -- through the raw entry points, against
numpy.  tests/test_compare_core_cpu.py walks the same cases on the host with the rules of csrc/compare_core.hpp.  Run with -m gpu."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import compare_cases as cc

pytestmark = pytest.mark.gpu

SCALED = dict(cc.scaled_cases())
NUM = {name: (sk, nums) for name, sk, nums in cc.num_cases()}


def _gpu():
    import torch
    import sourmash_amd
    from sourmash_amd import device as smd
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.utils import rustcall
    assert sourmash_amd.gpu_available()
    return torch, smd, lib, rustcall


@functools.lru_cache(maxsize=None)
def _want_scaled(name):
    return cc.common_matrix(SCALED[name])


@pytest.mark.parametrize("name", sorted(SCALED))
def test_scaled_counts_in_every_launch_form(name):
    torch, smd, lib, rustcall = _gpu()
    sk = SCALED[name]
    n = len(sk)
    want = _want_scaled(name)
    h, off = smd.pack_csr(sk)
    for form in cc.scaled_forms(n):
        kind, lo, hi, first, stride, count = form
        rows, mask = cc.expected_for_form(want, form)
        if kind == "blocks":
            out = torch.full((count * 16, n), -1, dtype=torch.int32, device="cuda")
            rustcall(lib.smgpu_compare_blocks_raw, smd._ptr(h), smd._ptr(off), n, first, stride, count, smd._ptr(out), smd._stream(torch))
            jac = None
        else:
            out, jac = smd.compare_rows(h, off, lo, hi)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[mask], rows[mask]), (name, form)
        if jac is not None:
            sizes = np.array([len(s) for s in sk], dtype=np.float64)
            union = np.maximum(sizes[lo:hi, None] + sizes[None, :] - rows, 1.0)
            expect = np.where(np.arange(lo, hi)[:, None] == np.arange(n)[None, :], 1.0, rows / union)
            assert np.array_equal(jac.cpu().numpy().view(np.uint64), expect.view(np.uint64)), (name, form)


@pytest.mark.parametrize("name", sorted(NUM))
def test_bottom_k_cuts(name):
    torch, smd, lib, rustcall = _gpu()
    sk, nums = NUM[name]
    n = len(sk)
    want_c, want_u, want_j = cc.num_reference(sk, nums)
    h, off = smd.pack_csr(sk)
    d_nums = torch.from_numpy(nums.view(np.int32).copy()).cuda()
    common = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    union = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    jac = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    rustcall(lib.smgpu_compare_num_raw, smd._ptr(h), smd._ptr(off), smd._ptr(d_nums), n, smd._ptr(common), smd._ptr(union), smd._ptr(jac),
             smd._stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(common.cpu().numpy().view(np.uint32), want_c), name
    assert np.array_equal(union.cpu().numpy().view(np.uint32), want_u), name
    assert np.array_equal(jac.cpu().numpy().view(np.uint64), want_j.view(np.uint64)), name


def _abund_child(kind):
    "runs in a child process (the switches are read once per process): every case of one kind against numpy"
    torch, smd, lib, rustcall = _gpu()
    for name, sk, ab, narrow in (cc.walk_cases() if kind == "walk" else cc.join_cases()):
        n, total = len(sk), sum(len(s) for s in sk)
        want_c, want_p = cc.abund_reference(sk, ab)
        h, off = smd.pack_csr(sk)
        flat = np.concatenate(ab) if total else np.zeros(2, dtype=np.uint64)
        d_ab = torch.from_numpy(flat.view(np.int64).copy()).cuda()
        common = torch.full((n, n), -1, dtype=torch.int32, device="cuda")
        prod = torch.full((n, n), -1, dtype=torch.int64, device="cuda")
        sq = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        rustcall(lib.smgpu_compare_abund_raw_n, smd._ptr(h), smd._ptr(d_ab), smd._ptr(off), n, total, bool(narrow), smd._ptr(common),
                 smd._ptr(prod), smd._ptr(sq), smd._stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(common.cpu().numpy().view(np.uint32), want_c), name
        assert np.array_equal(prod.cpu().numpy().view(np.uint64), want_p), name
        assert np.array_equal(sq.cpu().numpy().view(np.uint64), np.diag(want_p)), name
    print("ok")


def _run_children(kind, envs):
    from conftest import ROOT
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_compare_edges as t\nt._abund_child(%r)\n" % (ROOT, os.path.join(ROOT, "tests"), kind))
    for extra in envs:                                         # one after another, each under its own time limit
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, **extra))
        if p.returncode < 0:
            pytest.fail("the child died of signal %d and no further one is started: %r\n%s" % (-p.returncode, extra, p.stderr[-3000:]))
        assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (extra, p.stdout[-1500:], p.stderr[-3000:])


def test_abundance_walk_slices_and_wide_products():
    "compare_ext_kernel: a tile cut into 2 and into the cap of 16 hash ranges; u32 and u64 abundances, 2^32 among them; 2^63 x 2 wraps"
    _run_children("walk", [{"SMG_COMPARE_ABUND": "walk"}])


def test_abundance_join_at_every_slice_count():
    """abund_pairs.hip: blocks of 1 .. 129 sketches, runs of 16 / 17 / 64 equal hashes (the inline limit, the worklist), a run across
    entry 4,096 of a staged list, a (block, slice) too large for the LDS merge, diagonal tiles; with 1, 2, 15 and 16 hash slices per
    tile"""
    _run_children("join", [{"SMG_ABUND_SLICES": str(z)} for z in cc.JOIN_SLICES])
