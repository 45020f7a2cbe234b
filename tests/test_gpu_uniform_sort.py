"""The sort + unique for uniform keys on the GPU (csrc/uniform_sort.hip) through sourmash_amd.device.sort_unique_uniform, against
numpy.unique(return_counts=True), with the sort_counters() deltas saying which form ran: the one-workgroup form, the bucket form,
or the general sort after the bucket form gave up.  The inputs (tests/uniform_sort_cases.py) are seeded; the CPU emulation
(tests/test_uniform_sort_core_cpu.py) has been through every one of them and shows that the plan's own rule keeps the uniform ones
inside their leaves -- that they do not fall back here is a condition of these tests, not a measurement.  Run with -m gpu."""
import numpy as np
import pytest

import uniform_sort_cases as uc

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def smd():
    import torch  # noqa: F401
    import sourmash_amd
    from sourmash_amd import device
    assert sourmash_amd.gpu_available()
    return device


def delta(before, after):
    return {k: after[k] - before[k] for k in before}


def served_by(case):
    if case.want == uc.FALLBACK:
        return {"bucket": 0, "small": 0, "fellback": 1}
    if case.form == uc.FORM_SMALL:
        return {"bucket": 0, "small": 1, "fellback": 0}
    return {"bucket": 1, "small": 0, "fellback": 0}


@pytest.mark.parametrize("case", uc.cases(), ids=lambda c: c.name)
def test_against_numpy_unique(smd, case):
    import torch
    want_keys, want_counts = uc.expected(case)
    max_hash = 0 if case.thr == uc.U64_MAX else case.thr
    for counts in (False, True):
        keys = torch.from_numpy(case.keys.view(np.int64).copy()).cuda()
        before = smd.sort_counters()
        got = smd.sort_unique_uniform(keys, max_hash, n=case.count, counts=counts)
        assert delta(before, smd.sort_counters()) == served_by(case), (case.name, counts)
        got_keys = (got[0] if counts else got).cpu().numpy().view(np.uint64)
        assert np.array_equal(got_keys, want_keys), (case.name, counts, len(got_keys), len(want_keys))
        if counts:
            assert np.array_equal(got[1].cpu().numpy().view(np.uint64), want_counts.astype(np.uint64)), case.name
        if case.want != uc.FALLBACK:                       # the input is the caller's unless the general sort had to take it
            assert np.array_equal(keys.cpu().numpy().view(np.uint64), case.keys), case.name


@pytest.mark.parametrize("name", ["count-above-small", "count-above"])
def test_a_count_above_n_max_writes_nothing_past_the_end(smd, name):
    "the raw call with guard words behind the n_max entries of the output and of the counts"
    import torch
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.utils import rustcall
    case = next(c for c in uc.cases() if c.name == name)
    n_max, pad = len(case.keys), 64
    keys = torch.from_numpy(case.keys.view(np.int64).copy()).cuda()
    guard = np.array([GUARD], dtype=np.uint64).view(np.int64)[0]
    out = torch.full((n_max + pad,), int(guard), dtype=torch.int64, device="cuda")
    cnt = torch.full((n_max + pad,), int(guard), dtype=torch.int64, device="cuda")
    d_n = torch.tensor([case.count], dtype=torch.int64, device="cuda")
    result = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.smgpu_sort_unique_uniform_workspace_bytes(n_max, 1)), dtype=torch.uint8, device="cuda")
    m = rustcall(lib.smgpu_sort_unique_uniform_raw, keys.data_ptr(), d_n.data_ptr(), n_max, case.thr, out.data_ptr(), cnt.data_ptr(),
                 result.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    want_keys, want_counts = uc.expected(case)
    assert m == len(want_keys) == int(result[0].item())
    assert np.array_equal(out[:m].cpu().numpy().view(np.uint64), want_keys)
    assert np.array_equal(cnt[:m].cpu().numpy().view(np.uint64), want_counts.astype(np.uint64))
    assert (out[n_max:].cpu().numpy().view(np.uint64) == GUARD).all() and (cnt[n_max:].cpu().numpy().view(np.uint64) == GUARD).all()
    assert int(d_n[0].item()) == case.count
