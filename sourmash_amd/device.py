"""Device-resident batch API: torch tensors in, torch tensors out.

PyTorch is plumbing here -- it owns the HBM allocations, the current HIP stream
and (in parallel.py) the RCCL process group; every computation is one of the
raw C-ABI entry points of include/sourmash_amd.h (smgpu_*_raw), i.e. the
hand-written HIP kernels.  Nothing in this module runs on the CPU: without a GPU
every function raises.
"""
import ctypes as C

from ._lowlevel import lib
from .minhash import _get_max_hash_for_scaled
from .exceptions import SourmashError, exceptions_by_code
from .utils import decode_str, rustcall


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sourmash_amd.device needs a HIP device (no CPU fallback)")
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _u64(torch, n, device):
    # torch has no uint64 arithmetic but int64 storage is all we need (bit patterns)
    return torch.empty(int(n), dtype=torch.int64, device=device)


def arena_stats():
    "the library's device arena (csrc/arena.hpp): driver calls, time in the driver, reuse hits, bytes live / cached"
    out = (C.c_uint64 * 8)()
    lib.smgpu_arena_stats(out)
    keys = ("driver_allocs", "driver_frees", "driver_ns", "reuse_hits", "live_bytes", "cached_bytes", "peak_bytes",
            "cross_stream_waits")
    return dict(zip(keys, (int(v) for v in out)))


def arena_trim(keep_bytes=0):
    "give the arena's cached blocks back to the driver"
    lib.smgpu_arena_trim(int(keep_bytes))


def synth_dna(n, seed=42, record_len=0, start=0, device="cuda", out=None):
    "n bytes of the BASELINE C2 random-DNA stream generated in HBM (uint8 tensor)."
    torch = _torch()
    if out is None:
        out = torch.empty(int(n), dtype=torch.uint8, device=device)
    rustcall(lib.smgpu_synth_dna_raw, _ptr(out), int(start), int(n), int(seed), int(record_len), _stream(torch))
    return out


def fastx_carry(fastq, device="cuda"):
    "the 4-byte parser carry in front of a file's first piece: {1, 1, 0, 0} for FASTA, {3, 1, 0, 0} for FASTQ"
    torch = _torch()
    return torch.tensor([3 if fastq else 1, 1, 0, 0], dtype=torch.uint8, device=device)


def fastx_compact(raw, fastq, carry, out, result, record_starts=None, last_piece=False):
    """The FASTA / FASTQ parser by itself (smgpu_fastx_compact_raw, csrc/fastx.hip) on the next piece of a file held in HBM.

    raw: uint8 tensor, 16-byte aligned (any other pointer raises before anything is launched); carry: the file's 4 bytes
    (fastx_carry); out: uint8, room for raw.numel() bytes; result: int64[2], [0] = bytes kept of this piece, [1] += its header
    lines; record_starts: int64 tensor or None, entry j = offset in `out` just behind the j-th kept header byte of this piece.
    Asynchronous on the current stream."""
    torch = _torch()
    assert raw.dtype == torch.uint8 and out.dtype == torch.uint8 and carry.dtype == torch.uint8 and carry.numel() >= 4
    assert result.dtype == torch.int64 and result.numel() >= 2 and out.numel() >= raw.numel()
    assert record_starts is None or record_starts.dtype == torch.int64
    rustcall(lib.smgpu_fastx_compact_raw, _ptr(raw), raw.numel(), 1 if fastq else 0, _ptr(carry), _ptr(out), _ptr(result),
             _ptr(record_starts) if record_starts is not None else None, record_starts.numel() if record_starts is not None else 0,
             1 if last_piece else 0, _stream(torch))


def sigjson_parse(text, text_len, docs, keep_max, values, spans=None, parsed_capacity=None):
    """The signature JSON array parser by itself (smgpu_sigjson_parse_raw, csrc/sigjson.hip) on a block of JSON text held in HBM.

    text: uint8 tensor holding text_len bytes of text and at least sigjson_text_pad() readable bytes behind them; docs: the
    documents as (off, len) pairs; values: int64 tensor that takes the values of every parsed `mins` array side by side (u64 bit
    patterns; what lies behind them is not touched); spans: a numpy array of len(docs) * 8 span records to fill in place (a new
    one, zeroed, if None).  -> (spans, doc_flags uint32[len(docs)], parsed: n_jobs records {n_kept, flags}, n_values), all numpy
    on the host.  The jobs are every `mins` array, in order, of every document with no odd bit and no odd array.  Synchronous."""
    import numpy as np
    torch = _torch()
    span_t = np.dtype([("begin", "<u8"), ("end", "<u8"), ("n_values", "<u4"), ("kind", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
    parsed_t = np.dtype([("n_kept", "<u4"), ("flags", "<u4")])
    assert text.dtype == torch.uint8 and values.dtype == torch.int64 and text.numel() >= int(text_len) + int(lib.smgpu_sigjson_text_pad())
    d = np.ascontiguousarray(np.asarray(docs, dtype=np.uint64).reshape(-1, 2))
    n = len(d)
    if spans is None:
        spans = np.zeros(n * 8, dtype=span_t)
    assert spans.dtype == span_t and len(spans) >= n * 8 and spans.flags.c_contiguous
    flags = np.zeros(n, dtype=np.uint32)
    cap = n * 8 if parsed_capacity is None else int(parsed_capacity)
    parsed = np.zeros(cap, dtype=parsed_t)
    counts = np.zeros(2, dtype=np.uint64)
    rustcall(lib.smgpu_sigjson_parse_raw, _ptr(text), int(text_len), d.ctypes.data, n, int(keep_max), spans.ctypes.data, flags.ctypes.data,
             _ptr(values), values.numel(), parsed.ctypes.data, cap, counts.ctypes.data, _stream(torch))
    return spans, flags, parsed[:int(counts[0])], int(counts[1])


def sigjson_text_pad():
    "readable bytes sigjson_parse needs behind the text (the parse kernel loads whole 16-byte lines)"
    return int(lib.smgpu_sigjson_text_pad())


def _records_error(code, message):
    "the exception of a failed per-record call: starts the library refuses are the caller's ValueError"
    if "record starts" in message or "record ends" in message:
        return ValueError(message)
    return exceptions_by_code.get(code, SourmashError)(message)


def _residue_hash_function(moltype):
    "the library's hash_function number of a molecule type name (1 DNA, 2 protein, 3 dayhoff, 4 hp)"
    try:
        return {"DNA": 1, "PROTEIN": 2, "DAYHOFF": 3, "HP": 4}[str(moltype).upper()]
    except KeyError:
        raise ValueError(f"unknown moltype {moltype!r}") from None


def _check_records(torch, seq, starts, moltype, is_protein, ends):
    "the argument checks of the two sketch_records (DeviceSketcher, SketchSet) -> the library's hash_function number"
    assert seq.dtype == torch.uint8 and seq.is_cuda and seq.is_contiguous()
    assert starts.dtype == torch.int64 and starts.is_cuda and starts.is_contiguous()
    if starts.numel() < 1:
        raise ValueError("record starts: n_records + 1 offsets are needed")
    hf = _residue_hash_function(moltype)
    if hf == 1 and (is_protein or ends is not None):
        raise ValueError("is_protein and ends go with moltype protein, dayhoff or hp")
    if ends is not None:
        assert ends.dtype == torch.int64 and ends.is_cuda and ends.is_contiguous()
        if ends.numel() != starts.numel() - 1:
            raise ValueError("record ends: n_records offsets are needed")
    return hf


class DeviceSketcher:
    """Reusable scratch for sketching device-resident sequence buffers.

    sketch(seq) -> int64 tensor viewing the sorted unique kept hashes (u64 bit patterns).
    Capacity is sized from scaled (expected kept = len/scaled) with slack; on
    overflow the buffers grow and the call is repeated.
    """

    def __init__(self, ksize=31, scaled=1000, seed=42, device="cuda"):
        self.torch = _torch()
        self.ksize, self.scaled, self.seed, self.device = int(ksize), int(scaled), int(seed), device
        self.max_hash = _get_max_hash_for_scaled(scaled)
        self.cap = 0
        self.out = self.ws = None
        self.result = self.torch.zeros(2, dtype=self.torch.int64, device=device)

    def _reserve(self, cap):
        if cap <= self.cap:
            return
        torch = self.torch
        self.cap = int(cap)
        self.out = _u64(torch, self.cap, self.device)
        nbytes = lib.smgpu_sketch_workspace_bytes(self.cap)
        self.ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)

    def capacity_for(self, n_bases):
        expect = n_bases / max(self.scaled, 1)
        return int(expect * 1.25 + 8 * expect ** 0.5 + 4096)

    def sketch(self, seq):
        torch = self.torch
        assert seq.dtype == torch.uint8 and seq.is_cuda and seq.is_contiguous()
        n = seq.numel()
        self._reserve(self.capacity_for(n))
        for attempt in range(2):
            lib.sourmash_err_clear()
            got = lib.smgpu_sketch_dna_raw(_ptr(seq), n, self.ksize, self.seed, self.max_hash, _ptr(self.out),
                                           self.cap, _ptr(self.result), _ptr(self.ws), self.ws.numel(),
                                           _stream(torch))
            code = lib.sourmash_err_get_last_code()
            if code == 0:
                return self.out[:got]
            message = decode_str(lib.sourmash_err_get_last_message())
            kept = int(self.result[0].item())
            if attempt == 0 and kept > self.cap:   # repetitive input beat the estimate: grow and retry once
                self._reserve(kept + 1024)
                continue
            raise exceptions_by_code.get(code, SourmashError)(message)

    def sketch_records(self, seq, starts, *, abund=False, moltype="DNA", is_protein=False, ends=None):
        """One sketch per record of `seq` in one pass (smgpu_sketch_records_raw, csrc/sketch_records.hip).

        moltype protein / dayhoff / hp (smgpu_sketch_residue_records_raw, csrc/protein_records.hip): the sketcher's ksize counts
        residues, 1 .. 79; is_protein: the records are residues, otherwise DNA that is translated in six frames record by
        record.  ends (these moltypes only): int64 device tensor of n_records offsets, record r = seq[starts[r]:ends[r]] with
        starts[r] <= ends[r] <= starts[r + 1]; None: records touch.  An end outside its record raises ValueError.

        starts: int64 device tensor of n_records + 1 ascending offsets, record r = seq[starts[r]:starts[r + 1]]; records may
        touch, and a k-mer counts only for the record it lies in entirely.  -> (hashes, offsets[, abunds]): the CSR of
        sorted distinct kept hashes (int64 tensors of u64 bit patterns; row r is hashes[offsets[r]:offsets[r + 1]]), new
        tensors.  ksize 1 .. 88.  Starts that are not ascending or end behind the buffer raise ValueError."""
        torch = self.torch
        hf = _check_records(torch, seq, starts, moltype, is_protein, ends)
        n, n_records = seq.numel(), starts.numel() - 1
        translate = hf != 1 and not is_protein
        windows = 2 * n if translate else n
        expect = windows / max(self.scaled, 1)
        cap = max(1, min(windows, int(expect * 2 + 16 * (expect + 1) ** 0.5) + 4096))   # the slack of the batched ingest (csrc/ingest.hpp)
        result = torch.zeros(4, dtype=torch.int64, device=seq.device)
        offsets = _u64(torch, n_records + 1, seq.device)
        for attempt in range(2):
            hashes = _u64(torch, cap, seq.device)
            abunds = _u64(torch, cap, seq.device) if abund else None
            if hf == 1:
                ws = torch.empty(int(lib.smgpu_sketch_records_workspace_bytes(cap, n_records)), dtype=torch.uint8, device=seq.device)
                lib.sourmash_err_clear()
                got = lib.smgpu_sketch_records_raw(_ptr(seq), n, _ptr(starts), n_records, self.ksize, self.seed, self.max_hash,
                                                   _ptr(hashes), _ptr(abunds) if abund else None, cap, _ptr(offsets), _ptr(result),
                                                   _ptr(ws), ws.numel(), _stream(torch))
            else:
                ws = torch.empty(int(lib.smgpu_sketch_residue_records_workspace_bytes(cap, n_records, n, int(translate))), dtype=torch.uint8,
                                 device=seq.device)
                lib.sourmash_err_clear()
                got = lib.smgpu_sketch_residue_records_raw(_ptr(seq), n, _ptr(starts), _ptr(ends) if ends is not None else None, n_records,
                                                           self.ksize, hf, int(translate), self.seed, self.max_hash, _ptr(hashes),
                                                           _ptr(abunds) if abund else None, cap, _ptr(offsets), _ptr(result), _ptr(ws),
                                                           ws.numel(), _stream(torch))
            code = lib.sourmash_err_get_last_code()
            if code == 0:
                return (hashes[:got], offsets, abunds[:got]) if abund else (hashes[:got], offsets)
            message = decode_str(lib.sourmash_err_get_last_message())
            kept = int(result[0].item())
            if attempt == 0 and kept > cap:                            # repetitive input beat the estimate: grow and retry once
                cap = kept
                continue
            raise _records_error(code, message)

    def records_kernel_only(self, seq, out_hashes, out_positions, count):
        "Just the (hash, position) kernel of sketch_records: appends to the two arrays, adds to `count` (int64[1], caller zeroes)."
        torch = self.torch
        rustcall(lib.smgpu_sketch_records_kernel_raw, _ptr(seq), seq.numel(), self.ksize, self.seed, self.max_hash,
                 _ptr(out_hashes), _ptr(out_positions), min(out_hashes.numel(), out_positions.numel()), _ptr(count), _stream(torch))

    def residue_kernel_only(self, aa, out_hashes, out_positions, count, n_dev=None):
        """Just the window kernel of the per-record residue sketches on a residue buffer `aa` (8-byte aligned): appends to the two
        arrays, adds to `count` (int64[1], caller zeroes).  out_positions None: the hash-only kernel of the record-by-record route
        on the same buffer.  n_dev (int64[1]): the buffer's size on the device; with it 0xFF bytes separate."""
        torch = self.torch
        cap = out_hashes.numel() if out_positions is None else min(out_hashes.numel(), out_positions.numel())
        rustcall(lib.smgpu_residue_records_kernel_raw, _ptr(aa), aa.numel(), _ptr(n_dev) if n_dev is not None else None, self.ksize, self.seed,
                 self.max_hash, _ptr(out_hashes), _ptr(out_positions) if out_positions is not None else None, cap, _ptr(count), _stream(torch))

    def kernel_only(self, seq, out, count, grid=0):
        """Just the k-mer kernel (no sort): appends to `out`, adds to `count` (int64[1], caller zeroes).  grid: 0 for the
        library's own number of workgroups, otherwise exactly that many (ksize <= 88)."""
        torch = self.torch
        rustcall(lib.smgpu_sketch_dna_kernel_grid_raw, _ptr(seq), seq.numel(), self.ksize, self.seed, self.max_hash,
                 _ptr(out), out.numel(), _ptr(count), int(grid), _stream(torch))


def sort_unique(keys):
    """int64 tensor of u64 bit patterns, any order, duplicates allowed -> the sorted (as unsigned) distinct values, a new
    tensor: the library's radix sort + run-length encode (smgpu_sort_unique_raw, csrc/device_sort.hip).  `keys` is consumed."""
    torch = _torch()
    assert keys.dtype == torch.int64 and keys.is_cuda and keys.is_contiguous()
    n = keys.numel()
    out = _u64(torch, max(n, 1), keys.device)
    if n == 0:
        return out[:0]
    ws = torch.empty(int(lib.smgpu_sketch_workspace_bytes(n)), dtype=torch.uint8, device=keys.device)
    n_out = torch.zeros(1, dtype=torch.int64, device=keys.device)
    m = rustcall(lib.smgpu_sort_unique_raw, _ptr(keys), n, _ptr(out), _ptr(n_out), _ptr(ws), ws.numel(), _stream(torch))
    return out[:m]


def sort_unique_uniform(keys, max_hash, n=None, counts=False):
    """The same for keys that are uniform on [0, max_hash] (max_hash 0: all 64 bits), e.g. kept hashes, through the sort that
    uses it (smgpu_sort_unique_uniform_raw, csrc/uniform_sort.hip): the number of keys is read on the device -- `n` (default
    len(keys)) is put there, and anything above len(keys) counts as len(keys).  `keys` is not modified unless the keys turn
    out not to be uniform and the general sort takes over (sort_counters() tells).  -> the sorted distinct values, with
    counts=True also their multiplicities; new tensors."""
    torch = _torch()
    assert keys.dtype == torch.int64 and keys.is_cuda and keys.is_contiguous()
    n_max = keys.numel()
    out = _u64(torch, max(n_max, 1), keys.device)
    cnt = _u64(torch, max(n_max, 1), keys.device) if counts else None
    d_n = torch.tensor([n_max if n is None else int(n)], dtype=torch.int64, device=keys.device)
    result = torch.zeros(1, dtype=torch.int64, device=keys.device)
    ws = torch.empty(int(lib.smgpu_sort_unique_uniform_workspace_bytes(n_max, int(counts))), dtype=torch.uint8, device=keys.device)
    thr = int(max_hash) if max_hash else 0xFFFFFFFFFFFFFFFF
    m = rustcall(lib.smgpu_sort_unique_uniform_raw, _ptr(keys) if n_max else _ptr(out), _ptr(d_n), n_max, thr, _ptr(out),
                 _ptr(cnt) if counts else None, _ptr(result), _ptr(ws), ws.numel(), _stream(torch))
    return (out[:m], cnt[:m]) if counts else out[:m]


def sort_counters():
    """{"bucket", "small", "fellback"}: sketch / sort_unique_uniform calls since the library was loaded that the uniform sort's
    bucket form served, its one-workgroup form, and calls that fell back to the general sort (smgpu_sort_counters)."""
    import ctypes
    out = (ctypes.c_uint64 * 3)()
    lib.smgpu_sort_counters(out)
    return {"bucket": int(out[0]), "small": int(out[1]), "fellback": int(out[2])}


def pack_csr(sketches, device="cuda"):
    "list of sorted u64 numpy arrays -> (hashes int64 tensor, offsets int64 tensor) on device."
    import numpy as np
    torch = _torch()
    offsets = np.zeros(len(sketches) + 1, dtype=np.int64)
    for i, s in enumerate(sketches):
        offsets[i + 1] = offsets[i] + len(s)
    flat = np.concatenate([np.asarray(s, dtype=np.uint64) for s in sketches]) if len(sketches) and offsets[-1] \
        else np.zeros(0, dtype=np.uint64)
    hashes = torch.from_numpy(flat.view(np.int64).copy()).to(device)
    if hashes.numel() == 0:
        hashes = torch.zeros(2, dtype=torch.int64, device=device)
    return hashes, torch.from_numpy(offsets).to(device)


class BitIndex:
    """Compare index of a device CSR (smgpu_bitindex_*): hashes held by many sketches as bit columns, hashes held
    by few as inverted lists.  `BitIndex.build` returns None when the merge kernel is the cheaper tool."""

    def __init__(self, ptr, n):
        self._ptr, self.n = ptr, n

    @classmethod
    def build(cls, hashes, offsets, threshold=None, one_shot=False):
        """threshold: hashes held by more sketches than this become bit columns (None: the library's cost model);
        one_shot: the index serves one compare only, so its own build time counts against it."""
        torch = _torch()
        n = offsets.numel() - 1
        ptr = rustcall(lib.smgpu_bitindex_new_ex, _ptr(hashes), _ptr(offsets), n, 0, int(threshold or 0), bool(one_shot),
                       _stream(torch))
        return cls(ptr, n) if ptr else None

    @property
    def universe(self):
        return lib.smgpu_bitindex_universe(self._ptr)

    @property
    def builder(self):
        "which builder made the index: 'dictionary' (sort-free passes, csrc/dictindex.hip) or 'sort' (radix sort of all pairs)"
        return {1: "dictionary", 2: "sort"}.get(int(lib.smgpu_bitindex_builder(self._ptr)), "?")

    @property
    def stats(self):
        "(frequent hashes = bit columns, matrix increments the rare hashes cost per compare, threshold)"
        f, r, t = C.c_uint64(), C.c_uint64(), C.c_uint32()
        lib.smgpu_bitindex_stats(self._ptr, C.byref(f), C.byref(r), C.byref(t))
        return f.value, r.value, t.value

    def compare_tiles(self, first, stride, count, out=None, upper=False):
        """u32 counts for the 16-row tiles first, first+stride, ... (count of them): all columns, or with upper=True only
        the entries on or above the diagonal (for callers that mirror the triangle afterwards; the rest is left as it was)"""
        torch = _torch()
        if out is None:
            out = torch.empty((count * 16, self.n), dtype=torch.int32, device="cuda")
        fn = lib.smgpu_bitindex_compare_upper_raw if upper else lib.smgpu_bitindex_compare_raw
        rustcall(fn, self._ptr, first, stride, count, _ptr(out), _stream(torch))
        return out

    def __del__(self):
        if getattr(self, "_ptr", None) and lib is not None:        # (module globals are gone at interpreter exit)
            lib.smgpu_bitindex_free(self._ptr)
            self._ptr = None


def compare_rows(hashes, offsets, row_lo=0, row_hi=None, want_jaccard=True, common=None, jaccard=None, index=None,
                 method="merge"):
    """common[(row_hi-row_lo), n] (int32 view of u32) and jaccard (float64) for a row block of the
    all-pairs matrix of a device CSR.  Asynchronous on the current stream.

    index: a BitIndex built for this CSR -> indexed path (bit columns + inverted lists).  Without one, method
    "merge" runs the LDS-tiled merge kernel and "auto" first lets the library build a one-shot index if its cost
    model says that beats merging (what smgpu_compare_all_pairs does)."""
    torch = _torch()
    if index is None and method == "auto":
        index = BitIndex.build(hashes, offsets, one_shot=True)
    n = offsets.numel() - 1
    row_hi = n if row_hi is None else row_hi
    rows = row_hi - row_lo
    if want_jaccard and jaccard is None:
        jaccard = torch.empty((rows, n), dtype=torch.float64, device=hashes.device)
    if index is not None and row_lo % 16 == 0:
        count = (rows + 15) // 16
        if common is None or common.shape[0] < count * 16:
            common = torch.empty((count * 16, n), dtype=torch.int32, device=hashes.device)
        if row_lo == 0 and row_hi == n:                         # the whole matrix: the triangle, then its mirror image
            index.compare_tiles(0, 1, count, out=common, upper=True)
            rustcall(lib.smgpu_symmetrize_raw, _ptr(common), n, _stream(torch))
        else:
            index.compare_tiles(row_lo // 16, 1, count, out=common)
        if want_jaccard:
            rustcall(lib.smgpu_jaccard_raw, _ptr(common), _ptr(offsets), n, row_lo, row_hi, _ptr(jaccard), _stream(torch))
        return common[:rows], (jaccard if want_jaccard else None)
    if common is None:
        common = torch.empty((rows, n), dtype=torch.int32, device=hashes.device)
    rustcall(lib.smgpu_compare_raw, _ptr(hashes), _ptr(offsets), n, row_lo, row_hi, _ptr(common),
             _ptr(jaccard) if want_jaccard else None, _stream(torch))
    return common, (jaccard if want_jaccard else None)
