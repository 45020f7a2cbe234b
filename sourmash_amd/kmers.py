"""The way back from a sketch to the sequences it came from: `sourmash sig kmers`.

The reference (src/sourmash/sig/__main__.py:1087-1310) sketches every record of the sequence files, intersects it with the
merged query and then walks the k-mers of each matching record in Python with one membership test per k-mer.  Here a whole
buffer or file goes through one kernel pass that keeps only the k-mers whose hash is in the query (csrc/sketch_find.hip):

    query = KmerQuery([sig1, sig2])            # the union of compatible flat scaled DNA sketches
    m = query.find_file("reads.fq.gz")         # or query.find(seq, starts) on tensors already in HBM
    for name, kmer, hashval in m.rows(): ...

Reported is every position i of a record whose window s[i:i+k] holds only ACGTacgt and whose canonical hash is in the query:
the k-mer text is the window as it stands in the record (upper-cased), not the canonical strand -- what
`MinHash.kmers_and_hashes` yields -- and a k-mer that occurs several times, or on both strands, is reported at each position.
Rows are ordered by record, then position: the reference's CSV row order.

One deliberate difference from the reference: a k-mer holding a byte outside ACGTacgt never matches and never raises.  The
reference sketches a record with force=True but then calls kmers_and_hashes(force=False), so with --save-kmers it dies on an
`N` in a matching record.

Scope: flat scaled DNA sketches of one ksize.  num sketches, protein / dayhoff / hp sketches and --translate are refused.
"""
import csv
import ctypes as C

import numpy as np

from ._lowlevel import lib
from .exceptions import SourmashError, exceptions_by_code
from .minhash import MinHash, to_bytes
from .signature import SourmashSignature
from .utils import decode_str, rustcall

__all__ = ["KmerQuery", "KmerMatches", "find_kmers"]

FIND_MAX_KSIZE = 88                  # the longest k-mer of the kernel (csrc/sketch_kernel.hpp: SK_FAST_MAX_K)
CHUNK_BYTES = 256 << 20              # sequence bytes find_file keeps in HBM at a time where the one-pass file path is not taken


def _as_minhash(obj):
    if isinstance(obj, MinHash):
        return obj
    if isinstance(obj, SourmashSignature):
        return obj.minhash
    raise TypeError(f"KmerQuery takes MinHash or SourmashSignature objects, not {type(obj).__name__}")


class KmerMatches:
    """The rows of a search, on the host.  Row i is (records[i], positions[i], hashes[i], kmers()[i]); the rows of record r
    are offsets[r]:offsets[r + 1].  positions count from the start of the row's record."""

    def __init__(self, ksize, names, lengths, offsets, positions, hashes, kmer_bytes, sequences, owner=None):
        self.ksize = int(ksize)
        self._names = names                                        # list of str, or a callable that makes it
        self.record_lengths = np.asarray(lengths, dtype=np.uint64)
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        self.positions = np.asarray(positions, dtype=np.uint64)
        self.hashes = np.asarray(hashes, dtype=np.uint64)
        self._kmer_bytes = np.asarray(kmer_bytes, dtype=np.uint8).reshape(-1, self.ksize) if self.ksize else np.zeros((0, 0), np.uint8)
        self._sequences = sequences                                # {record: bytes} or a callable record -> bytes
        self._owner = owner
        assert len(self.offsets) == len(self.record_lengths) + 1
        assert len(self.positions) == len(self.hashes) == len(self._kmer_bytes) == int(self.offsets[-1])

    def __len__(self):
        return len(self.positions)

    @property
    def n_records(self):
        return len(self.record_lengths)

    @property
    def n_bases(self):
        return int(self.record_lengths.sum())

    @property
    def names(self):
        if callable(self._names):
            self._names = self._names()
        return self._names

    @property
    def records(self):
        "the record (row number of the input) of every row"
        return np.repeat(np.arange(self.n_records, dtype=np.uint64), np.diff(self.offsets).astype(np.int64))

    def kmers(self):
        "the k-mer text of every row: the window as it stands in the record, upper-cased"
        if not len(self):
            return []
        flat = self._kmer_bytes.tobytes().decode("ascii")
        k = self.ksize
        return [flat[i:i + k] for i in range(0, len(flat), k)]

    @property
    def matched_records(self):
        "[(record, name)] of the records with at least one row"
        names = self.names
        return [(int(r), names[int(r)]) for r in np.flatnonzero(np.diff(self.offsets))]

    def sequence(self, record):
        "the sequence of a matched record, as the file or buffer holds it (str)"
        record = int(record)
        if not 0 <= record < self.n_records or self.offsets[record] == self.offsets[record + 1]:
            raise KeyError(f"record {record} has no matching k-mer")
        s = self._sequences(record) if callable(self._sequences) else self._sequences[record]
        return bytes(s).decode("ascii", "replace")

    @property
    def found_hashes(self):
        "the distinct reported hashes, sorted"
        return np.unique(self.hashes)

    def rows(self):
        "yield (record name, k-mer, hashval) row by row: the reference's CSV columns behind the file name"
        names = self.names
        for r, kmer, h in zip(self.records.tolist(), self.kmers(), self.hashes.tolist()):
            yield names[r], kmer, h

    @classmethod
    def concat(cls, ksize, parts):
        "the matches of consecutive pieces of one input as one"
        if len(parts) == 1:
            return parts[0]
        names, seqs, at = [], {}, 0
        for p in parts:
            names.extend(p.names)
            for r, _ in p.matched_records:
                seqs[at + r] = p.sequence(r).encode("ascii", "replace")
            at += p.n_records
        offsets, base = [np.zeros(1, dtype=np.uint64)], 0
        for p in parts:
            offsets.append(p.offsets[1:] + np.uint64(base))
            base += len(p)

        def cat(arrs, dtype):
            return np.concatenate(arrs) if arrs else np.zeros(0, dtype=dtype)
        return cls(ksize, names, cat([p.record_lengths for p in parts], np.uint64), np.concatenate(offsets),
                   cat([p.positions for p in parts], np.uint64), cat([p.hashes for p in parts], np.uint64),
                   cat([p._kmer_bytes.reshape(-1) for p in parts], np.uint8), seqs)

    def __eq__(self, other):
        return (isinstance(other, KmerMatches) and self.ksize == other.ksize and list(self.names) == list(other.names)
                and np.array_equal(self.record_lengths, other.record_lengths) and np.array_equal(self.offsets, other.offsets)
                and np.array_equal(self.positions, other.positions) and np.array_equal(self.hashes, other.hashes)
                and np.array_equal(self._kmer_bytes, other._kmer_bytes)
                and all(self.sequence(r) == other.sequence(r) for r, _ in self.matched_records))

    __hash__ = None


class _MatchesHandle:
    "owner of a SmgpuKmerMatches handle"

    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        ptr, self.ptr = self.ptr, None
        if ptr and lib is not None:
            lib.smgpu_kmermatches_free(ptr)


def _find_error(code, message):
    "the exception of a failed find: starts the library refuses are the caller's ValueError"
    if "record starts" in message:
        return ValueError(message)
    return exceptions_by_code.get(code, SourmashError)(message)


class KmerQuery:
    """The union of one or more compatible sketches, built as the reference merges them (sig/__main__.py:1113-1135): the
    first one's copy_and_clear(), track_abundance off, merge of each -- an incompatible sketch raises what merge raises."""

    def __init__(self, sketches):
        if isinstance(sketches, (MinHash, SourmashSignature)):
            sketches = [sketches]
        mhs = [_as_minhash(s) for s in sketches]
        if not mhs:
            raise ValueError("no signatures in query")
        first = mhs[0]
        if first.moltype != "DNA":
            raise ValueError(f"k-mer finding takes DNA sketches, not {first.moltype} sketches (and no --translate)")
        query = first.copy_and_clear().to_mutable()
        query.track_abundance = False
        for mh in mhs:
            if mh.num or not mh.scaled:
                raise ValueError("k-mer finding takes scaled sketches, not num sketches")
            flat = mh.to_mutable()
            flat.track_abundance = False
            query.merge(flat)
        if not len(query):
            raise ValueError("no hashes in query signature")
        self.minhash = query.to_frozen()
        self._hashes = query._mins_array()
        self._ptr = rustcall(lib.smgpu_kmerquery_new, (C.c_void_p * 1)(query._get_objptr()), 1)

    def __del__(self):
        ptr, self._ptr = getattr(self, "_ptr", None), None
        if ptr and lib is not None:
            lib.smgpu_kmerquery_free(ptr)

    def __len__(self):
        return int(lib.smgpu_kmerquery_len(self._ptr))

    ksize = property(lambda self: self.minhash.ksize)
    scaled = property(lambda self: self.minhash.scaled)
    seed = property(lambda self: self.minhash.seed)

    # ---- device buffers -----------------------------------------------------------------------------------------------------
    def find(self, seq, starts, names=None):
        """Every k-mer of the records of `seq` that hashes into the query -> KmerMatches.

        seq: uint8 device tensor; starts: int64 device tensor of n_records + 1 ascending offsets, record r =
        seq[starts[r]:starts[r + 1]]; records may touch, and a k-mer counts only for the record it lies in entirely.  Starts
        that are not ascending or end behind the buffer raise ValueError.  names: one per record (default: the row numbers)."""
        from .device import _ptr, _stream, _torch, _u64
        torch = _torch()
        assert seq.dtype == torch.uint8 and seq.is_cuda and seq.is_contiguous()
        assert starts.dtype == torch.int64 and starts.is_cuda and starts.is_contiguous()
        if starts.numel() < 1:
            raise ValueError("record starts: n_records + 1 offsets are needed")
        n, n_records, k = seq.numel(), starts.numel() - 1, self.ksize
        if names is None:
            names = [str(r) for r in range(n_records)]
        if k > FIND_MAX_KSIZE:
            return self._find_long(seq, starts, names)
        expect = n / max(self.scaled, 1)
        cap = max(1, min(n, int(expect * 2 + 16 * (expect + 1) ** 0.5) + 4096))   # the slack of DeviceSketcher.sketch_records
        result = torch.zeros(4, dtype=torch.int64, device=seq.device)
        offsets = _u64(torch, n_records + 1, seq.device)
        for attempt in range(2):
            positions, hashes = _u64(torch, cap, seq.device), _u64(torch, cap, seq.device)
            kmers = torch.empty(cap * k, dtype=torch.uint8, device=seq.device)
            ws = torch.empty(int(lib.smgpu_find_kmers_workspace_bytes(cap, n_records)), dtype=torch.uint8, device=seq.device)
            lib.sourmash_err_clear()
            got = lib.smgpu_find_kmers_raw(self._ptr, _ptr(seq), n, _ptr(starts), n_records, _ptr(positions), _ptr(hashes), _ptr(kmers),
                                           cap, _ptr(offsets), _ptr(result), _ptr(ws), ws.numel(), _stream(torch))
            code = lib.sourmash_err_get_last_code()
            if code == 0:
                break
            message = decode_str(lib.sourmash_err_get_last_message())
            matched = int(result[0].item())
            if attempt == 0 and matched > cap:                         # repetitive input beat the estimate: grow and retry once
                cap = matched
                continue
            raise _find_error(code, message)
        h_starts = starts.cpu().numpy().astype(np.uint64)
        h_offsets = offsets.cpu().numpy().view(np.uint64)
        h_pos = positions[:got].cpu().numpy().view(np.uint64)
        rel = h_pos - np.repeat(h_starts[:-1], np.diff(h_offsets).astype(np.int64))

        def sequence(r):
            return seq[int(h_starts[r]):int(h_starts[r + 1])].cpu().numpy().tobytes()
        return KmerMatches(k, names, np.diff(h_starts), h_offsets, rel, hashes[:got].cpu().numpy().view(np.uint64),
                           kmers[:got * k].cpu().numpy(), sequence)

    def kernel_only(self, seq, out_hashes, out_positions, count, grid=0):
        """Just the find kernel (no assign, no sort): appends the matched hashes and the positions of their k-mers in `seq` to
        the two arrays, unordered, and adds to `count` (int64[1], caller zeroes).  grid: 0 for the library's own number of
        workgroups, otherwise exactly that many.  ksize 1 .. 88."""
        from .device import _ptr, _stream, _torch
        torch = _torch()
        rustcall(lib.smgpu_find_kmers_kernel_raw, self._ptr, _ptr(seq), seq.numel(), _ptr(out_hashes), _ptr(out_positions),
                 min(out_hashes.numel(), out_positions.numel()), _ptr(count), int(grid), _stream(torch))

    def _find_long(self, seq, starts, names):
        "k > 88 on device tensors: the records come to the host and go record by record"
        h_starts = starts.cpu().numpy()
        if np.any(np.diff(h_starts) < 0):
            raise ValueError("record starts: the offsets are not ascending")
        if len(h_starts) and h_starts[-1] > seq.numel():
            raise ValueError(f"record starts: the last offset lies behind the end of the buffer ({seq.numel()} bytes)")
        buf = seq.cpu().numpy().tobytes()
        return self._find_records([(names[r], buf[h_starts[r]:h_starts[r + 1]]) for r in range(len(h_starts) - 1)])

    def _find_records(self, records):
        """Record by record, for any DNA ksize: the hash of every position from MinHash.seq_to_hashes(force=True,
        bad_kmers_as_zeroes=True) -- the GPU's per-position kernel -- and numpy.isin against the query."""
        k = self.ksize
        probe = self.minhash.copy_and_clear()
        names, lengths, offsets, pos, hs, text, seqs = [], [], [0], [], [], [], {}
        for r, (name, s) in enumerate(records):
            s = to_bytes(s)
            names.append(name)
            lengths.append(len(s))
            if len(s) >= k:
                dense = np.asarray(probe.seq_to_hashes(s, force=True, bad_kmers_as_zeroes=True), dtype=np.uint64)
                at = np.flatnonzero((dense != 0) & np.isin(dense, self._hashes))
                if len(at):
                    pos.append(at.astype(np.uint64))
                    hs.append(dense[at])
                    up = np.frombuffer(s.upper(), dtype=np.uint8)
                    text.append(up[at[:, None] + np.arange(k)[None, :]].reshape(-1))
                    seqs[r] = s
            offsets.append(offsets[-1] + (len(pos[-1]) if r in seqs else 0))

        def cat(arrs, dtype):
            return np.concatenate(arrs) if arrs else np.zeros(0, dtype=dtype)
        return KmerMatches(k, names, lengths, offsets, cat(pos, np.uint64), cat(hs, np.uint64), cat(text, np.uint8), seqs)

    # ---- files ----------------------------------------------------------------------------------------------------------------
    def find_file(self, path):
        """Every record of a FASTA / FASTQ file (plain or gzip) -> KmerMatches with the records' names.

        A file the one-pass per-record path takes (k <= 88, at most 2 GiB of text) is parsed and searched on the device in one
        call (smgpu_find_kmers_file).  Any other goes through `find` in pieces of whole records, at most 256 MiB of sequence each
        (a longer record is a piece of its own), or, for k > 88, record by record; the results are the same."""
        from .sketch import _records_path_takes, read_records
        path = str(path)
        k = self.ksize
        if _records_path_takes(path, [k]):
            return self._find_file_native(path)
        if k > FIND_MAX_KSIZE:
            return self._find_records(read_records(path))
        from .device import _torch
        torch = _torch()
        parts, recs, size = [], [], 0

        def flush():
            buf = np.frombuffer(b"".join(s for _, s in recs), dtype=np.uint8)
            starts = np.concatenate([[0], np.cumsum([len(s) for _, s in recs])]).astype(np.int64)
            seq_t = torch.from_numpy(buf.copy()).cuda() if len(buf) else torch.zeros(0, dtype=torch.uint8, device="cuda")
            m = self.find(seq_t, torch.from_numpy(starts).cuda(), names=[n for n, _ in recs])
            m._sequences = {r: recs[r][1] for r, _ in m.matched_records}      # the host copies: the tensor goes away
            parts.append(m)

        for name, s in read_records(path):
            if recs and size + len(s) > CHUNK_BYTES:
                flush()
                recs, size = [], 0
            recs.append((name, s))
            size += len(s)
        if recs or not parts:
            flush()
        return KmerMatches.concat(k, parts)

    def _find_file_native(self, path):
        ptr = rustcall(lib.smgpu_find_kmers_file, self._ptr, path.encode("utf-8"))
        owner = _MatchesHandle(ptr)
        n_records, n_rows, k = int(lib.smgpu_kmermatches_n_records(ptr)), int(lib.smgpu_kmermatches_n_rows(ptr)), self.ksize

        def arr(fn, n, dtype):
            p = fn(ptr)
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype=dtype)

        def names():
            return [decode_str(lib.smgpu_kmermatches_record_name(owner.ptr, r)) for r in range(n_records)]

        def sequence(r):
            n = C.c_uint64(0)
            p = lib.smgpu_kmermatches_record_sequence(owner.ptr, r, C.byref(n))
            return C.string_at(p, n.value) if p else b""
        return KmerMatches(k, names, arr(lib.smgpu_kmermatches_record_lengths, n_records, np.uint64),
                           arr(lib.smgpu_kmermatches_offsets, n_records + 1, np.uint64), arr(lib.smgpu_kmermatches_positions, n_rows, np.uint64),
                           arr(lib.smgpu_kmermatches_hashes, n_rows, np.uint64), arr(lib.smgpu_kmermatches_kmers, n_rows * k, np.uint8),
                           sequence, owner=owner)


def find_kmers(signatures, sequence_files, *, save_kmers=None, save_sequences=None):
    """The body of `sourmash sig kmers --signatures ... --sequences ... [--save-kmers CSV] [--save-sequences FASTA]`.

    signatures: MinHash / SourmashSignature objects (or one); sequence_files: paths of FASTA / FASTQ(.gz) files.  The CSV has
    the reference's columns sequence_file, sequence_name, kmer, hashval in its row order; the FASTA is `>{name}\\n{sequence}\\n`
    per matching record.  -> dict of the totals the reference reports.  The counts of rows, matching records and their bases
    are returned whether or not a file is written.  Raises ValueError("no sequences searched") when the files hold no records.
    A k-mer with a byte outside ACGTacgt never matches and never raises (see the module docstring)."""
    query = signatures if isinstance(signatures, KmerQuery) else KmerQuery(signatures)
    if isinstance(sequence_files, (str, bytes)) or hasattr(sequence_files, "__fspath__"):
        sequence_files = [sequence_files]
    out = dict(n_files_searched=0, n_sequences_searched=0, n_bp_searched=0, n_kmers_found=0, n_sequences_found=0, n_bp_saved=0,
               n_query_hashes=len(query), n_found_hashes=0)
    found = []
    kmer_fp = open(save_kmers, "w", newline="") if save_kmers else None
    seq_fp = open(save_sequences, "w") if save_sequences else None
    try:
        kmer_w = csv.writer(kmer_fp) if kmer_fp else None
        if kmer_w:
            kmer_w.writerow(["sequence_file", "sequence_name", "kmer", "hashval"])
        for path in sequence_files:
            path = str(path)
            m = query.find_file(path)
            out["n_files_searched"] += 1
            out["n_sequences_searched"] += m.n_records
            out["n_bp_searched"] += m.n_bases
            out["n_kmers_found"] += len(m)
            found.append(m.found_hashes)
            for r, name in m.matched_records:
                out["n_sequences_found"] += 1
                out["n_bp_saved"] += int(m.record_lengths[r])
                if seq_fp:
                    seq_fp.write(f">{name}\n{m.sequence(r)}\n")
            if kmer_w:
                kmer_w.writerows((path, name, kmer, h) for name, kmer, h in m.rows())
    finally:
        if kmer_fp:
            kmer_fp.close()
        if seq_fp:
            seq_fp.close()
    if not out["n_sequences_searched"]:
        raise ValueError("no sequences searched")
    out["n_found_hashes"] = len(np.unique(np.concatenate(found))) if found else 0
    return out
