"""GPU parity of the FASTA / FASTQ parser (sourmash_amd/csrc/fastx.hip) at every edge its three kernels hand state across -- lane,
wavefront, block, the spans of the offsets walk, the carry between pieces -- with exact expected bytes, record starts, counts and
carry from the per-line reference of tests/fastx_cases.py (never from the host emulation or the library).  The cases go through
smgpu_fastx_compact_raw back to back on one stream and are read back once per group; a dozen named files go through the entry
points users call, against the oracle on the reference's records.  Run with -m gpu."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import fastx_cases as fc
from conftest import ROOT

pytestmark = pytest.mark.gpu

MARK = 0xEE                                    # fills the output buffers: no input holds this byte
GUARD = 0xA5A5A5A5A5A5A5A5
N_GUARD = 4


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    import sourmash_amd.device  # noqa: F401
    import sourmash_amd.sketch  # noqa: F401
    assert sourmash_amd.gpu_available(), "these tests need a real GPU"
    return sourmash_amd


def al16(x):
    return (x + 15) & ~15


class Job:
    "one file through the parser: whole (cuts None, record capacity `cap`) or in pieces with the carry chained on the device"
    def __init__(self, case, cuts=None, cap=None):
        self.case, self.n = case, len(case.raw)
        self.cuts = None if cuts is None else [int(c) for c in cuts]
        want = fc.expected(case.name)
        self.cap = (want.records if cap is None else cap) if cuts is None else self.n + 1
        self.pieces = [(0, self.n)] if cuts is None else list(zip(self.cuts[:-1], self.cuts[1:]))


def run_jobs(sm, jobs):
    """every piece of every job queued on the current stream, then one synchronisation and one read-back.  Layout: every piece's
    input begins at a 16-byte aligned offset of one buffer; a job's output region is n + 16 marker bytes, and the piece that begins
    at input offset c writes at c of it (a piece keeps at most its own length); its record starts likewise lie at entry c of the
    job's region, whose capacity is the piece's length (whole files: the job's capacity), with guard words behind the region."""
    import torch
    from sourmash_amd._lowlevel import lib
    in_off, out_off, st_off = [], [], []
    n_in = n_out = n_st = n_pieces = 0
    for j in jobs:
        offs = []
        for c0, c1 in j.pieces:
            offs.append(n_in)
            n_in = al16(n_in + (c1 - c0)) + 16
        in_off.append(offs)
        out_off.append(n_out)
        n_out += j.n + 16
        st_off.append(n_st)
        n_st += j.cap + N_GUARD
        n_pieces += len(j.pieces)
    h_in = np.full(n_in + 16, MARK, dtype=np.uint8)
    for j, offs in zip(jobs, in_off):
        raw = np.frombuffer(j.case.raw, dtype=np.uint8)
        for (c0, c1), o in zip(j.pieces, offs):
            h_in[o:o + c1 - c0] = raw[c0:c1]
    d_in = torch.from_numpy(h_in).cuda()
    d_out = torch.full((n_out + 16,), MARK, dtype=torch.uint8, device="cuda")
    d_st = torch.from_numpy(np.full(n_st + N_GUARD, GUARD, dtype=np.uint64).view(np.int64)).cuda()
    carry0 = np.zeros((len(jobs), 4), dtype=np.uint8)
    carry0[:, 0] = [3 if j.case.fastq else 1 for j in jobs]
    carry0[:, 1] = 1
    d_carry = torch.from_numpy(carry0.copy()).cuda()
    d_res = torch.zeros((len(jobs), 2), dtype=torch.int64, device="cuda")
    d_log = torch.full((n_pieces, 2), -1, dtype=torch.int64, device="cuda")
    assert d_in.data_ptr() % 16 == 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p_in, p_out, p_st, p_carry, p_res = d_in.data_ptr(), d_out.data_ptr(), d_st.data_ptr(), d_carry.data_ptr(), d_res.data_ptr()
    at = 0
    for ji, j in enumerate(jobs):
        whole = j.cuts is None
        for (c0, c1), o in zip(j.pieces, in_off[ji]):
            lib.sourmash_err_clear()
            lib.smgpu_fastx_compact_raw(p_in + o, c1 - c0, j.case.fastq, p_carry + 4 * ji, p_out + out_off[ji] + c0, p_res + 16 * ji,
                                        p_st + 8 * (st_off[ji] + c0), j.cap if whole else c1 - c0, 1 if whole else 0, stream)
            assert lib.sourmash_err_get_last_code() == 0, (j.case.name, c0, c1)
            if not whole:
                d_log[at].copy_(d_res[ji])                       # kept is per piece: logged in stream order
            at += 1
    torch.cuda.synchronize()
    out, st = d_out.cpu().numpy(), d_st.cpu().numpy().view(np.uint64)
    carry, res, log = d_carry.cpu().numpy(), d_res.cpu().numpy().view(np.uint64), d_log.cpu().numpy()
    results, at = [], 0
    for ji, j in enumerate(jobs):
        region = out[out_off[ji]:out_off[ji] + j.n + 16].copy()
        sreg = st[st_off[ji]:st_off[ji] + j.cap + N_GUARD]
        if j.cuts is None:
            kept, recs = int(res[ji, 0]), int(res[ji, 1])
            data = region[:kept].tobytes()
            region[:kept] = MARK
            starts = sreg[:min(recs, j.cap)].copy()
            untouched = sreg[min(recs, j.cap):]
            kept_per_piece = [kept]
            at += 1
            state = (int(carry[ji, 2]), int(carry[ji, 3]))
            assert tuple(carry[ji, :2]) == tuple(carry0[ji, :2]), j.case.name      # last_piece: the carry is not copied forward
        else:
            parts, starts, kept_per_piece, seen, total = [], [], [], 0, 0
            used = np.zeros(len(sreg), dtype=bool)
            for c0, c1 in j.pieces:
                k, r = int(log[at, 0]), int(log[at, 1])
                at += 1
                assert 0 <= k <= c1 - c0 and seen <= r <= seen + (c1 - c0), (j.case.name, c0, c1, k, r)
                parts.append(region[c0:c0 + k].tobytes())
                region[c0:c0 + k] = MARK
                starts.append(sreg[c0:c0 + r - seen] + np.uint64(total))
                used[c0:c0 + r - seen] = True
                kept_per_piece.append(k)
                total, seen = total + k, r
            data = b"".join(parts)
            starts = np.concatenate(starts) if starts else np.zeros(0, dtype=np.uint64)
            untouched = sreg[~used]
            kept, recs = total, int(res[ji, 1])
            assert int(res[ji, 0]) == kept_per_piece[-1] and recs == seen, j.case.name   # kept is the last piece's, records the sum
            state = (int(carry[ji, 0]), int(carry[ji, 1]))
        assert (region == MARK).all(), (j.case.name, "bytes written behind the kept ones")
        assert (untouched == np.uint64(GUARD)).all(), (j.case.name, "record starts written at or behind the capacity")
        results.append((data, starts, kept, recs, state, kept_per_piece))
    return results


def check(job, got, cap=None):
    want = fc.expected(job.case.name)
    data, starts, kept, recs, state, _ = got
    what = (job.case.name, job.cuts if job.cuts is None or len(job.cuts) < 12 else len(job.cuts))
    assert (kept, recs) == (want.kept, want.records), (what, kept, want.kept, recs, want.records)
    assert data == want.out, what
    assert np.array_equal(starts, want.starts if cap is None else want.starts[:cap]), what
    assert state == want.carry, (what, state, want.carry)


def test_whole_files(sm):
    "every case as one piece: bytes, record starts, kept and record counts, the carry behind it, nothing written behind the kept bytes"
    jobs = [Job(c) for c in fc.small_cases()]
    for job, got in zip(jobs, run_jobs(sm, jobs)):
        check(job, got)


def test_1025_blocks_whole(sm):
    "two blocks per span of the offsets walk (and spans with none), FASTA with CRLF and FASTQ, headers that cover whole blocks"
    jobs = [Job(c) for c in fc.big_cases()]
    for job, got in zip(jobs, run_jobs(sm, jobs)):
        check(job, got)


@pytest.mark.parametrize("size", fc.PIECE_SIZES)
def test_pieces_with_the_carry_chained_on_the_device(sm, size):
    """every case of at most three blocks in pieces of `size` bytes and one empty piece (fc.piece_cuts): the concatenated bytes, the
    shifted starts, the summed records and the final carry are the whole file's; kept is per piece, records accumulate"""
    jobs = [Job(c, cuts=fc.piece_cuts(c, size)) for c in fc.piece_cases()]
    for job, got in zip(jobs, run_jobs(sm, jobs)):
        check(job, got)
        empty = [i for i, (c0, c1) in enumerate(job.pieces) if c0 == c1]
        assert empty and all(got[5][i] == 0 for i in empty), job.case.name


@pytest.mark.parametrize("cut", fc.BIG_CUTS)
def test_1025_blocks_in_two_pieces(sm, cut):
    jobs = [Job(c, cuts=[0, cut, cut, len(c.raw)]) for c in fc.big_cases()]
    for job, got in zip(jobs, run_jobs(sm, jobs)):
        check(job, got)


def test_an_empty_piece_leaves_carry_and_records_untouched(sm):
    import torch
    from sourmash_amd import device
    case = fc.by_name()["sweep-fastq-line1-p8192-lf-nolf"]
    raw = torch.from_numpy(np.frombuffer(case.raw, dtype=np.uint8).copy()).cuda()
    out = torch.full((len(case.raw),), MARK, dtype=torch.uint8, device="cuda")
    carry, res = device.fastx_carry(True), torch.zeros(2, dtype=torch.int64, device="cuda")
    device.fastx_compact(raw[:8192], True, carry, out, res)
    before = (carry.cpu().tolist(), res.cpu().tolist())
    assert before[1][0] > 0 and before[1][1] > 0 and before[0][:2] == before[0][2:]
    device.fastx_compact(raw[:0], True, carry, out[8192:], res)
    assert carry.cpu().tolist() == before[0] and res.cpu().tolist() == [0, before[1][1]]
    assert (out[8192:] == MARK).all().item()


def test_record_capacity(sm):
    "capacities 0, 1 and records - 1 with guard words behind the array: nothing at or behind the capacity, every record counted"
    cases = [c for c in fc.small_cases() if fc.expected(c.name).records >= 2][::7] + list(fc.big_cases())
    jobs = [Job(c, cap=cap) for c in cases for cap in (0, 1, fc.expected(c.name).records - 1)]
    for job, got in zip(jobs, run_jobs(sm, jobs)):
        check(job, got, cap=job.cap)


def test_misaligned_input_is_refused_on_the_host(sm):
    "d_raw is 16-byte aligned (fastx_api.hpp): any other pointer is an error before anything is launched, and nothing is written"
    import torch
    from sourmash_amd import device
    raw = torch.from_numpy(np.frombuffer(b">a\nACGT\n" * 40, dtype=np.uint8).copy()).cuda()
    out = torch.full((raw.numel(),), MARK, dtype=torch.uint8, device="cuda")
    carry, res = device.fastx_carry(False), torch.full((2,), 77, dtype=torch.int64, device="cuda")
    for shift in (1, 8, 15):
        with pytest.raises(sm.exceptions.SourmashError, match="16-byte aligned"):
            device.fastx_compact(raw[shift:], False, carry, out, res)
    torch.cuda.synchronize()
    assert carry.cpu().tolist() == [1, 1, 0, 0] and res.cpu().tolist() == [77, 77] and (out == MARK).all().item()
    device.fastx_compact(raw[16:], False, carry, out, res, last_piece=True)
    assert res.cpu().tolist() == [5 * 38, 77 + 38]


# ---- through the entry points users call ----------------------------------------------------------------------------------------------
PARAMS = "k=21,k=31,k=51,scaled=1,abund"
KS = (21, 31, 51)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    "name -> (path, path of the gzip form, raw bytes, fastq, the reference's records)"
    d = tmp_path_factory.mktemp("fastx_edges")
    out = {}
    for name, raw in fc.named_files().items():
        fastq = int(raw[:1] == b"@")
        p, z = d / name, d / (name + ".gz")
        p.write_bytes(raw)
        z.write_bytes(gzip.compress(raw, 6))
        out[name] = (str(p), str(z), raw, fastq, fc.records_of(raw, fastq))
    assert len(out) >= 12
    return out


@pytest.fixture(scope="module")
def wants(files):
    "the oracle on the reference's records, once: name -> {k: (mins, abunds)}"
    from test_gpu_ingest import _oracle_sig
    out = {}
    for name, (_, _, _, _, recs) in files.items():
        sigs = {k: _oracle_sig([(None, r) for r in recs], k, scaled=1, abund=True) for k in KS}
        out[name] = {k: (mh.mins.copy(), mh.abunds.copy()) for k, mh in sigs.items()}
        assert len(out[name][21][0]) > 100, name
    return out


def assert_sig(sig, want, what):
    got = {mh.ksize: mh for mh in sig.minhashes()}
    assert sorted(got) == list(KS), what
    for k in KS:
        assert np.array_equal(got[k]._mins_array(), want[k][0]), (what, k)
        assert list(got[k].hashes.values()) == want[k][1].tolist(), (what, k)          # one wrong byte changes a count


def test_sketch_file(sm, files, wants):
    for name, (path, _, _, _, _) in files.items():
        sig, = sm.sketch.sketch_file(path, PARAMS)
        assert_sig(sig, wants[name], name)


@pytest.mark.parametrize("chunk", [256, 8192, 8193])
def test_sketch_file_in_chunks(sm, files, wants, chunk):
    """the streaming ingest in pieces of a lane multiple, a block, and a block and a byte (the chunk size is read once per process):
    the plain files in chunks copied up from the host, their .gz forms inflated on the device and parsed as slices of that block
    (there an odd chunk is rounded down to 16 bytes, so that every slice is aligned)"""
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import torch
from sourmash_amd.sketch import sketch_file
for path in {[f[i] for f in files.values() for i in (0, 1)]!r}:
    sig, = sketch_file(path, {PARAMS!r})
    for mh in sig.minhashes():
        np.save(path + f".c{chunk}.k{{mh.ksize}}.npy", np.array([list(mh.hashes.keys()), list(mh.hashes.values())], dtype=np.uint64))
"""
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, SMG_INGEST_CHUNK=str(chunk)))
    for name, (plain, gz, _, _, _) in files.items():
        for path in (plain, gz):
            for k in KS:
                got = np.load(path + f".c{chunk}.k{k}.npy")
                assert np.array_equal(got[0], wants[name][k][0]) and np.array_equal(got[1], wants[name][k][1]), (path, chunk, k)


def test_sketch_file_singleton(sm, files):
    "the record starts of the singleton path: one signature per header line, each the oracle's sketch of that record alone"
    from test_gpu_ingest import _oracle_sig
    for name, (path, _, raw, fastq, _) in files.items():
        out, starts = fc.reference(raw, fastq)
        recs = [out[s:starts[j + 1] - 1 if j + 1 < len(starts) else len(out)] for j, s in enumerate(starts)]
        sigs = sm.sketch.sketch_file(path, PARAMS, singleton=True)
        assert len(sigs) == len(recs), name
        for r in range(len(recs)):
            for mh in sigs[r].minhashes():
                want = _oracle_sig([(None, recs[r])], mh.ksize, scaled=1, abund=True)
                assert np.array_equal(mh._mins_array(), want.mins) and list(mh.hashes.values()) == want.abunds.tolist(), (name, r, mh.ksize)


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
def test_sketch_files_as_one_batch(sm, files, wants, gz):
    "the whole dozen as one batch: plain through the per-file pipeline, .gz inflated on the device and parsed as slices of one block"
    names = list(files)
    sigs = sm.sketch.sketch_files([files[n][1 if gz else 0] for n in names], PARAMS, threads=1)
    assert len(sigs) == len(names)
    for name, sig in zip(names, sigs):
        assert_sig(sig, wants[name], (name, gz))


@pytest.mark.parametrize("name", ["cr-last-in-block.fa", "block-entered-in-phase-2.fq"])
def test_hll_and_nodegraph_add_file(sm, files, name):
    from test_gpu_hll import _hll, _regs, _want
    from test_gpu_nodegraph import all_hashes, assert_model
    path, _, raw, fastq, recs = files[name]
    want = fc.expected_of(raw, fastq)
    h = _hll(sm, 21, 14)
    n_rec, n_bases = h.add_file(path)
    assert (n_rec, n_bases) == (want.records, want.kept - want.records)
    assert np.array_equal(_regs(h), _want(recs, 21, 14))
    g = sm.Nodegraph(21, 100000, 4)
    n_rec, n_bases = g.add_file(path)
    assert (n_rec, n_bases) == (want.records, want.kept - want.records)
    assert_model(g, all_hashes(recs, 21))
