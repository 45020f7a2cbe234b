"""Index / CounterGather -- search, prefetch and gather over collections of signatures.

API of src/sourmash/index/__init__.py: IndexSearchResult (:55), Index.find (:115-170),
search (:202-239), prefetch (:241-256), best_containment (:258-270), counter_gather
(:302-320), LinearIndex (:397-453) and CounterGather (:735-909).

What changes underneath: the collection lives in HBM as one CSR (`SketchSet`), so
  * find() scores the query against EVERY signature with one overlap kernel
    (the reference loops over signatures, two FFI clones + one merge each);
  * CounterGather keeps its counters on the GPU: add-time overlaps, the arg-max with
    the reference tie-break, and consume() are single kernel launches.
Results (which signatures, which order, which numbers) are those of the reference.
"""
import csv
import ctypes as C
import io
import math
import os
from collections import Counter, namedtuple

import numpy as np

from ._lowlevel import lib
from .minhash import flatten_and_downsample_num, flatten_and_downsample_scaled, flatten_and_intersect_scaled
from .search import calc_threshold_from_bp, make_containment_query, make_jaccard_search_query
from .signature import SourmashSignature, load_signatures_from_json, save_signatures_to_json
from .utils import RustObject, decode_str, objptr_array, rustcall

__all__ = ["IndexSearchResult", "Collection", "SketchSet", "GatherStats", "many_need", "score_hits", "rank_scored", "SketchSetWriter", "select_signature", "Index", "LinearIndex", "CounterGather"]

IndexSearchResult = namedtuple("Result", "score, signature, location")


def _path_array(paths):
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    enc = [os.fsencode(p) for p in paths]
    return (C.c_char_p * max(len(enc), 1))(*enc), len(enc)


def _manifest_rows(csv_text):
    "manifest CSV -> list of dict rows with the reference's column types (manifest.py:84-98)"
    lines = csv_text.splitlines(keepends=True)
    rows = list(csv.DictReader(io.StringIO("".join(lines[1:]), newline="")))
    for row in rows:
        for k in ("num", "scaled", "ksize", "n_hashes"):
            row[k] = int(row[k])
        row["with_abundance"] = bool(int(row["with_abundance"]))
    return rows


class Collection(RustObject):
    """Signature files parsed into one host CSR + manifest by the native multi-threaded loader
    (smgpu_collection_*; no GPU involved).  `to_device()` uploads it as a SketchSet."""
    __dealloc_func__ = lib.smgpu_collection_free

    def __init__(self, paths, *, ksize=0, moltype=None, scaled=0, threads=0):
        arr, n = _path_array(paths)
        self._objptr = rustcall(lib.smgpu_collection_load, arr, n, int(ksize or 0),
                                moltype.encode() if moltype else None, int(scaled or 0), int(threads))

    def __len__(self):
        return self._methodcall(lib.smgpu_collection_len)

    @property
    def total_hashes(self):
        return self._methodcall(lib.smgpu_collection_total_hashes)

    @property
    def skipped(self):
        "sketches seen in the inputs that the selection left out"
        return self._methodcall(lib.smgpu_collection_skipped)

    @property
    def manifest_csv(self):
        return decode_str(self._methodcall(lib.smgpu_collection_manifest))

    @property
    def manifest(self):
        return _manifest_rows(self.manifest_csv)

    @property
    def offsets(self):
        ptr = self._methodcall(lib.smgpu_collection_offsets)
        return np.ctypeslib.as_array(ptr, shape=(len(self) + 1,)).copy()

    @property
    def hashes(self):
        n = self.total_hashes
        if not n:
            return np.zeros(0, dtype=np.uint64)
        return np.ctypeslib.as_array(self._methodcall(lib.smgpu_collection_hashes), shape=(n,)).copy()

    def to_device(self):
        return SketchSet._from_objptr(self._methodcall(lib.smgpu_sketchset_from_collection))


def score_hits(shared, sizes, n_query, *, do_containment=False, do_max_containment=False):
    """score[i] of a query of n_query hashes against a row of sizes[i] hashes sharing shared[i] with it: Jaccard by default, query
    containment or max containment on request -- the scores of JaccardSearch (search.py:88-160), 0 where the denominator is."""
    shared = np.asarray(shared).astype(np.float64)
    sizes = np.asarray(sizes).astype(np.float64)
    nq = float(n_query)
    if do_containment:
        return shared / nq if nq else np.zeros_like(shared)
    if do_max_containment:
        return np.divide(shared, np.minimum(sizes, nq), out=np.zeros_like(shared), where=np.minimum(sizes, nq) > 0)
    union = sizes + nq - shared
    return np.divide(shared, union, out=np.zeros_like(shared), where=union > 0)


def rank_scored(score, rows, *, threshold=0.0, best_only=False):
    "[(score, row)] best first, ties in the order given: the entries scoring >= threshold and above 0 (index/__init__.py:115-170)"
    keep = np.flatnonzero((score >= threshold) & (score > 0))
    order = keep[np.argsort(-score[keep], kind="stable")]
    hits = [(float(score[i]), int(rows[i])) for i in order]
    return hits[:1] if best_only else hits


def rank_search_hits(shared, sizes, n_query, *, threshold=0.0, do_containment=False, do_max_containment=False, best_only=False):
    """[(score, row)] best first from one overlap pass: shared[r] = |query ∩ row r|, sizes[r] = |row r|.  Jaccard by default,
    query containment or max containment on request -- the scores of JaccardSearch (search.py:88-160); rows scoring below
    the threshold or sharing nothing are dropped (index/__init__.py:115-170).  Shared by SketchSet.search (one GPU),
    SketchSet.search_many (the hits of one pass for many queries) and parallel.search_distributed (database sharded over the ranks)."""
    score = score_hits(shared, sizes, n_query, do_containment=do_containment, do_max_containment=do_max_containment)
    return rank_scored(score, np.arange(len(score)), threshold=threshold, best_only=best_only)


def many_need(sizes, threshold, *, do_containment=False, do_max_containment=False):
    """The integer filter the device applies for a search at `threshold`: need[q] for a query of sizes[q] hashes, never above the
    smallest common count that passes the float test of score_hits, never 0 (csrc/many_core.hpp: many_need)."""
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    out = np.ones(max(len(sizes), 1), dtype=np.uint32)
    mode = 1 if do_containment else 2 if do_max_containment else 0
    rustcall(lib.smgpu_many_need, mode, float(threshold), sizes.ctypes.data_as(C.c_void_p), len(sizes), out.ctypes.data_as(C.c_void_p))
    return out[:len(sizes)]


def prefetch_rows(shared, threshold_bp, scaled):
    "[(row, |intersect|)] in row order for the rows sharing at least threshold_bp with the query (search.py:956-976)"
    shared = np.asarray(shared)
    need = float(threshold_bp) / scaled if threshold_bp else 0.0
    return [(int(r), int(shared[r])) for r in np.flatnonzero((shared >= need) & (shared > 0))]


class SketchSet(RustObject):
    """n flat sketches packed as one device-resident CSR (smgpu_sketchset_*).

    Built from MinHash objects (`SketchSet(minhashes)`) or straight from files (`SketchSet.load(paths, ...)`:
    .sig / .sig.gz / .zip / directories / path lists, parsed by the native loader without creating a Python
    object per sketch).  A loaded set answers compare / search / gather by row number; `manifest[row]` says
    which signature that is, `signature(row)` materialises it.

    A set may carry abundances (`SketchSet(minhashes, track_abundance=True)`, `from_csr(..., abunds=)`): a uint64 column aligned
    with the hashes, every value at least 1.  See `track_abundance`, `abund_sums`, `flatten`, `inflate`, `filter_abund`, `merge`,
    `compare_angular`; `to_json`, `save` and SketchSetWriter write flat sets only."""
    __dealloc_func__ = lib.smgpu_sketchset_free
    _keep = ()
    _manifest = None

    def __init__(self, minhashes, track_abundance=False):
        """track_abundance=True: an abundance set -- every sketch must track abundance and share parameters; the set then carries a
        u64 abundance column beside its hashes (smgpu_sketchset_new_abund).  Every method that reads hashes only (compare, overlaps,
        search, gather, the *_many methods) sees such a set as its flattened self; subset, downsample, subtract and intersect
        carry the abundances, merge sums them, inflate / filter_abund / compare_angular / abund_sums use them.  The default keeps
        a flat set, of abundance sketches too."""
        self._keep = list(minhashes)
        ptrs, _alive = objptr_array(self._keep)
        self._objptr = rustcall(lib.smgpu_sketchset_new_abund if track_abundance else lib.smgpu_sketchset_new, ptrs, len(self._keep))
        if track_abundance:
            self._keep = ()                                             # (the set has host offsets and manifest rows of its own)

    @classmethod
    def load(cls, paths, *, ksize=0, moltype=None, scaled=0, threads=0):
        arr, n = _path_array(paths)
        return cls._from_objptr(rustcall(lib.smgpu_sketchset_load, arr, n, int(ksize or 0),
                                         moltype.encode() if moltype else None, int(scaled or 0), int(threads)))

    @classmethod
    def from_csr(cls, hashes, offsets, *, ksize, scaled=0, num=0, seed=42, moltype="DNA", names=None, filenames=None, abunds=None):
        """n flat sketches from device tensors (smgpu_sketchset_from_csr): row r = hashes[offsets[r]:offsets[r + 1]], ascending.
        hashes: int64 / uint64 device tensor (the bits are the hashes); offsets: int64 device tensor of n + 1 positions.  The rows
        are copied.  names / filenames: one string per row for the manifest.  abunds: an int64 / uint64 device tensor aligned with
        hashes makes an abundance set (smgpu_sketchset_from_csr_abund); an abundance of 0 is refused."""
        from .device import _ptr, _torch
        from .minhash import _get_max_hash_for_scaled
        torch = _torch()
        assert hashes.is_cuda and hashes.is_contiguous() and hashes.element_size() == 8
        assert offsets.dtype == torch.int64 and offsets.is_cuda and offsets.is_contiguous() and offsets.numel() >= 1
        _check_csr_abunds(abunds, hashes)
        n = offsets.numel() - 1

        def strings(values):
            if values is None:
                return None
            values = [v.encode("utf-8") if isinstance(v, str) else bytes(v) for v in values]
            if len(values) != n:
                raise ValueError("one string per row is needed")
            return (C.c_char_p * max(n, 1))(*values)
        hf = {"DNA": 1, "PROTEIN": 2, "DAYHOFF": 3, "HP": 4}[moltype.upper()]
        torch.cuda.current_stream().synchronize()                   # the library works on its own stream
        max_hash = _get_max_hash_for_scaled(int(scaled)) if scaled else 0
        if abunds is not None:
            return cls._from_objptr(rustcall(lib.smgpu_sketchset_from_csr_abund, _ptr(hashes), _ptr(abunds), _ptr(offsets), n, int(ksize), hf, int(seed),
                                             max_hash, int(num), strings(names), strings(filenames)))
        return cls._from_objptr(rustcall(lib.smgpu_sketchset_from_csr, _ptr(hashes), _ptr(offsets), n, int(ksize), hf, int(seed),
                                         max_hash, int(num), strings(names), strings(filenames)))

    @classmethod
    def sketch_records(cls, seq, starts, *, ksize, scaled, seed=42, moltype="DNA", is_protein=False, ends=None, track_abundance=False):
        """One flat scaled sketch per record of a device buffer, in one pass (smgpu_sketchset_sketch_records).  track_abundance=True:
        an abundance set -- a kept hash's abundance is the number of times its record holds it, as
        MinHash(track_abundance=True).add_sequence counts (smgpu_sketchset_sketch_records_abund and its residue sibling).

        seq: uint8 device tensor; starts: int64 device tensor of n_records + 1 ascending offsets, record r =
        seq[starts[r]:starts[r + 1]].  ksize 1 .. 88 (longer k-mers: sketch the records one by one).
        moltype protein / dayhoff / hp (smgpu_sketchset_sketch_residue_records): ksize counts residues, 1 .. 79; is_protein: the
        records are residues, otherwise DNA translated in six frames record by record; ends: int64 device tensor of n_records
        offsets, record r = seq[starts[r]:ends[r]] (None: records touch)."""
        from .device import _check_records, _ptr, _records_error, _torch
        torch = _torch()
        hf = _check_records(torch, seq, starts, moltype, is_protein, ends)
        torch.cuda.current_stream().synchronize()                   # the library works on its own stream
        lib.sourmash_err_clear()
        ab = int(bool(track_abundance))
        if hf == 1:
            ptr = lib.smgpu_sketchset_sketch_records_abund(_ptr(seq), seq.numel(), _ptr(starts), starts.numel() - 1, int(ksize), int(seed),
                                                           int(scaled), ab)
        else:
            ptr = lib.smgpu_sketchset_sketch_residue_records_abund(_ptr(seq), seq.numel(), _ptr(starts), _ptr(ends) if ends is not None else None,
                                                                   starts.numel() - 1, int(ksize), hf, int(not is_protein), int(seed), int(scaled), ab)
        code = lib.sourmash_err_get_last_code()
        if code:
            raise _records_error(code, decode_str(lib.sourmash_err_get_last_message()))
        return cls._from_objptr(ptr)

    @classmethod
    def sketch_file(cls, path, *, ksize=31, scaled=1000, seed=42, moltype="DNA", input_is_protein=False, track_abundance=False):
        """One flat scaled sketch per record of a FASTA / FASTQ file (plain or gzip): the device parses the file and
        sketches every record in one pass (smgpu_sketchset_sketch_file); manifest[row] carries the record's name and the
        file name.  What that path does not take (k > 88, a file above its size limit) is sketched record by record.
        track_abundance=True: an abundance set (manifest rows say with_abundance=True); the record-by-record way builds
        MinHash(track_abundance=True) objects and a SketchSet(..., track_abundance=True) of them.
        moltype protein / dayhoff / hp (smgpu_sketchset_sketch_residue_file): ksize counts residues, the one-pass path takes
        1 .. 79; input_is_protein: the records are residues, otherwise DNA translated in six frames."""
        from .device import _residue_hash_function
        from .sketch import _records_path_takes, _residue_records_path_takes, read_records
        path = os.fspath(path)
        hf = _residue_hash_function(moltype)
        if hf == 1 and input_is_protein:
            raise ValueError("input_is_protein goes with moltype protein, dayhoff or hp")
        ab = int(bool(track_abundance))
        if hf == 1 and _records_path_takes(path, [int(ksize)]):
            return cls._from_objptr(rustcall(lib.smgpu_sketchset_sketch_file_abund, os.fsencode(path), int(ksize), int(seed), int(scaled), ab))
        if hf != 1 and _residue_records_path_takes(path, [int(ksize)]):
            return cls._from_objptr(rustcall(lib.smgpu_sketchset_sketch_residue_file_abund, os.fsencode(path), int(ksize), hf,
                                             int(not input_is_protein), int(seed), int(scaled), ab))
        from .minhash import MinHash
        mhs, names = [], []
        mol = {2: dict(is_protein=True), 3: dict(dayhoff=True), 4: dict(hp=True)}.get(hf, {})
        for name, seq in read_records(path):
            mh = MinHash(0, int(ksize), scaled=int(scaled), seed=int(seed), track_abundance=bool(track_abundance), **mol)
            if input_is_protein:
                mh.add_protein(seq)
            else:
                mh.add_sequence(seq, True)
            mhs.append(mh)
            names.append(name)
        out = cls(mhs, track_abundance=bool(track_abundance))
        out.set_names(names, [path] * len(names))                   # (what to_json / save write; the manifest below says the same)
        sizes = out.sizes
        out._manifest = [dict(internal_location="", md5="", md5short="", ksize=int(ksize), moltype={1: "DNA", 2: "protein", 3: "dayhoff", 4: "hp"}[hf],
                              num=0, scaled=int(scaled), n_hashes=int(sizes[i]), with_abundance=bool(track_abundance), name=names[i], filename=path)
                         for i in range(len(names))]
        return out

    def __len__(self):
        return self._methodcall(lib.smgpu_sketchset_len)

    @property
    def total_hashes(self):
        return self._methodcall(lib.smgpu_sketchset_total_hashes)

    @property
    def manifest(self):
        if self._manifest is None:
            self._manifest = _manifest_rows(decode_str(self._methodcall(lib.smgpu_sketchset_manifest)))
        return self._manifest

    @property
    def skipped(self):
        "sketches seen in the inputs that the selection left out (a loaded set)"
        return self._methodcall(lib.smgpu_sketchset_skipped)

    @property
    def sizes(self):
        out = np.zeros(max(len(self), 1), dtype=np.uint64)
        self._methodcall(lib.smgpu_sketchset_sizes, out.ctypes.data_as(C.c_void_p))
        return out[:len(self)]

    @property
    def params(self):
        "(ksize, moltype, seed, scaled, num) shared by every row of a loaded set"
        k, hf, seed, mx, num = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._methodcall(lib.smgpu_sketchset_params, C.byref(k), C.byref(hf), C.byref(seed), C.byref(mx), C.byref(num))
        from .minhash import _get_scaled_for_max_hash
        moltype = {1: "DNA", 2: "protein", 3: "dayhoff", 4: "hp"}[hf.value]
        return k.value, moltype, seed.value, _get_scaled_for_max_hash(mx.value) if mx.value else 0, num.value

    @property
    def track_abundance(self):
        "does the set carry an abundance column beside its hashes?"
        return bool(lib.smgpu_sketchset_track_abundance(self._get_objptr()))

    @property
    def abund_sums(self):
        "MinHash.sum_abundances of every row as uint64 (wrapping), summed on the device (smgpu_sketchset_abund_sums)"
        _need_abundance_set(self.track_abundance, "abund_sums")
        out = np.zeros(max(len(self), 1), dtype=np.uint64)
        self._methodcall(lib.smgpu_sketchset_abund_sums, out.ctypes.data_as(C.c_void_p))
        return out[:len(self)]

    def minhash(self, row):
        "the sketch of a row; an abundance set gives abundance sketches"
        from .minhash import MinHash
        return MinHash._from_objptr(self._methodcall(lib.smgpu_sketchset_get, int(row)))

    def flatten(self):
        "a flat copy of the set (device-to-device): the hashes without the abundances; the manifest says with_abundance=False"
        return SketchSet._from_objptr(self._methodcall(lib.smgpu_sketchset_flatten))

    def inflate(self, other):
        """Every row's hashes that `other` holds, with `other`'s abundances (MinHash.inflate, `sig inflate`, and what -A does in
        `sig intersect` / `sig subtract`) -> an abundance set.  This set is flat (flatten() an abundance set first; the reference
        refuses the other order with the same words); `other` is an abundance MinHash, or an abundance SketchSet of one row or
        of len(self) rows (row by row).  Parameters must match as for intersect."""
        from .minhash import MinHash
        is_mh = isinstance(other, MinHash)
        if not is_mh and not isinstance(other, SketchSet):
            raise TypeError("the other side is a MinHash or a SketchSet")
        _check_inflate(self.track_abundance, other.track_abundance)
        if is_mh:
            return SketchSet._from_objptr(self._methodcall(lib.smgpu_sketchset_inflate_sketch, other._get_objptr()))
        _check_other_rows(len(self), len(other))
        return SketchSet._from_objptr(self._methodcall(lib.smgpu_sketchset_inflate, other._get_objptr()))

    def filter_abund(self, min_abundance=1, max_abundance=None):
        """Every row's hashes whose abundance a has min_abundance <= a and (max_abundance is None or a <= max_abundance), with
        their abundances (`sig filter`) -> an abundance set.  A flat set is a ValueError."""
        _need_abundance_set(self.track_abundance, "filter_abund")
        lo, hi = _abund_range(min_abundance, max_abundance)
        return SketchSet._from_objptr(self._methodcall(lib.smgpu_sketchset_filter_abund, lo, hi))

    def compare_angular(self):
        """-> f64 [n, n]: the angular similarity of every pair of rows, what compare_all_pairs(..., ignore_abundance=False) gives
        for the same sketches: the integer sums of the abundance kernels on the set's own buffers, then the host's formula.  A flat
        set is a ValueError."""
        _need_abundance_set(self.track_abundance, "compare_angular")
        n = len(self)
        out = np.zeros((n, n), dtype=np.float64)
        self._methodcall(lib.smgpu_sketchset_compare_angular, out.ctypes.data_as(C.c_void_p))
        return out

    def set_names(self, names=None, filenames=None):
        """One name / file name per row: what the set's signatures are written with (to_json, save, SketchSetWriter) and what its
        manifest rows say.  A set built from MinHash objects has none until they are given.  None leaves them as they are."""
        def strings(values):
            if values is None:
                return None
            values = [v.encode("utf-8") if isinstance(v, str) else bytes(v) for v in values]
            if len(values) != len(self):
                raise ValueError("one string per row of the set is needed")
            return (C.c_char_p * max(len(values), 1))(*values)
        self._methodcall(lib.smgpu_sketchset_set_names, strings(names), strings(filenames))
        if self._keep == ():
            self._manifest = None                                   # (a loaded set: read the rows again)

    def md5sums(self):
        "the md5sum of every row's sketch as hex strings, computed on the device (smgpu_sketchset_md5sums)"
        n = len(self)
        out = np.zeros(max(16 * n, 1), dtype=np.uint8)
        self._methodcall(lib.smgpu_sketchset_md5sums, out.ctypes.data_as(C.c_void_p))
        raw = out.tobytes()
        return [raw[16 * i:16 * i + 16].hex() for i in range(n)]

    def to_json(self, rows=None, compression=0):
        """The rows' signatures as the bytes save_signatures_to_json gives for [self.signature(r) for r in rows] (rows None: every
        row), written on the device (smgpu_sketchset_to_json).  compression > 0: the array as one gzip member."""
        size = C.c_size_t(0)
        if rows is None:
            raw = self._methodcall(lib.smgpu_sketchset_to_json, None, len(self), int(compression), C.byref(size))
        else:
            rows = np.ascontiguousarray(rows, dtype=np.uint64)
            raw = self._methodcall(lib.smgpu_sketchset_to_json, rows.ctypes.data_as(C.c_void_p), len(rows), int(compression), C.byref(size))
        try:
            return C.string_at(raw, size.value)
        finally:
            lib.nodegraph_buffer_free(raw, size.value)

    def save(self, path, *, compression=1):
        "write the set to `path`: .zip, .sig.gz (any .gz) or .sig (anything else), as SketchSetWriter does"
        with SketchSetWriter(path, compression=compression) as w:
            w.add(self)

    def subset(self, rows):
        "the given rows of a loaded set as a new set (device-side row gather; the manifest rows follow)"
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        return SketchSet._from_objptr(self._methodcall(lib.smgpu_sketchset_subset, rows.ctypes.data_as(C.c_void_p), len(rows)))

    def signature(self, row):
        "SourmashSignature of a row of a loaded set (name / filename from the manifest)"
        m = self.manifest[row]
        return SourmashSignature(self.minhash(row), name=m["name"], filename=m["filename"])

    def compare(self, *, jaccard=True):
        "-> (common u32 [n, n], jaccard f64 [n, n] or None) for the whole set"
        n = len(self)
        common = np.zeros((n, n), dtype=np.uint32)
        jac = np.zeros((n, n), dtype=np.float64) if jaccard else None
        self._methodcall(lib.smgpu_sketchset_compare, common.ctypes.data_as(C.c_void_p),
                         jac.ctypes.data_as(C.c_void_p) if jaccard else None)
        return common, jac

    def overlaps(self, query_mh):
        "|query ∩ row| for every row (one streaming pass over the CSR)"
        out = np.zeros(max(len(self), 1), dtype=np.uint64)
        self._methodcall(lib.smgpu_sketchset_overlaps, query_mh.flatten()._get_objptr(), out.ctypes.data_as(C.c_void_p))
        return out[:len(self)]

    def search(self, query_mh, *, threshold=0.0, do_containment=False, do_max_containment=False, best_only=False):
        """Rows scoring >= threshold against the query, best first -> [(score, row)].  Jaccard by default, query
        containment or max containment on request: the scores of JaccardSearch (search.py:88-160) from one overlap
        pass over the whole set."""
        if do_containment and do_max_containment:
            raise TypeError("'do_containment' and 'do_max_containment' cannot both be True")
        if (do_containment or do_max_containment) and not query_mh.scaled:
            raise TypeError("this search requires a scaled signature")
        return rank_search_hits(self.overlaps(query_mh), self.sizes, len(query_mh), threshold=threshold,
                                do_containment=do_containment, do_max_containment=do_max_containment, best_only=best_only)

    def prefetch(self, query_mh, threshold_bp=0):
        "Rows sharing at least threshold_bp with the query -> [(row, |intersect|)] in row order (search.py:956-976)."
        scaled = query_mh.scaled
        if not scaled:
            raise ValueError("prefetch requires scaled signatures")
        return prefetch_rows(self.overlaps(query_mh), threshold_bp, scaled)

    def gather(self, query_mh, threshold_bp=0):
        """Min-set-cover of the query by the rows of this set -> [(row, |intersect|)] in rank order; the whole
        loop runs on the GPU (GatherDatabases semantics, search.py:877-949, for equal scaled)."""
        scaled = query_mh.scaled
        if not scaled:
            raise ValueError("gather requires scaled signatures")
        thr = math.ceil(float(threshold_bp) / scaled) if threshold_bp else 0
        idx, isect = _DeviceCounter(self, query_mh.flatten()).gather(thr)
        return [(int(i), int(c)) for i, c in zip(idx, isect)]


    # ---- many queries in one pass over the set (csrc/overlap_many.hip) --------------------------------------------------------
    def _many_hits(self, queries, need):
        "the hits of `queries` (a SketchSet) against this set whose common count reaches need (an int, or one per query)"
        if not isinstance(queries, SketchSet):
            raise TypeError("the queries of a many-query search are a SketchSet")
        if np.ndim(need) == 0:
            need_arr, need_all = None, int(need)
            low = need_all < 1
        else:
            need_arr = np.ascontiguousarray(need, dtype=np.int64)
            if need_arr.shape != (len(queries),):
                raise ValueError("one count per query is needed")
            low = bool((need_arr < 1).any())
            need_arr, need_all = np.minimum(need_arr, 0xffffffff).astype(np.uint32), 1
        if low or need_all > 0xffffffff:
            raise ValueError("the common count a hit needs is at least 1")
        hits = _ManyHits._from_objptr(rustcall(lib.smgpu_sketchset_overlaps_many, self._get_objptr(), queries._get_objptr(),
                                               need_arr.ctypes.data_as(C.c_void_p) if need_arr is not None else None, need_all))
        hits._n_queries, hits._n_rows = len(queries), len(self)
        return hits

    def _sizes_at(self, scaled):
        "the rows' sizes once downsampled to `scaled`"
        from .minhash import _get_max_hash_for_scaled
        out = np.zeros(max(len(self), 1), dtype=np.uint64)
        self._methodcall(lib.smgpu_sketchset_sizes_at, _get_max_hash_for_scaled(int(scaled)), out.ctypes.data_as(C.c_void_p))
        return out[:len(self)]

    def overlaps_many(self, queries, min_common=1):
        """Every row of `queries` (a SketchSet) against every row of this set in one pass over it -> (query, row, common) arrays of
        the pairs sharing at least min_common hashes (an int, or one value per query; at least 1), ordered by (query, row).  Sets
        of different scaled meet at the coarser one."""
        hits = self._many_hits(queries, min_common)
        return hits.queries, hits.rows, hits.common

    def prefetch_many(self, queries, threshold_bp=0):
        "[self.prefetch(q, threshold_bp) for q in queries] from one pass over the set: per query [(row, |intersect|)] in row order"
        if not isinstance(queries, SketchSet):
            raise TypeError("the queries of a many-query search are a SketchSet")
        scaled = queries.params[3]
        if not scaled or not self.params[3]:
            raise ValueError("prefetch requires scaled signatures")
        need = float(threshold_bp) / scaled if threshold_bp else 0.0
        hits = self._many_hits(queries, max(1, int(math.ceil(need))))
        out = []
        for rows, common in hits.per_query(len(queries)):
            keep = (common >= need) & (common > 0)
            out.append([(int(r), int(c)) for r, c in zip(rows[keep], common[keep])])
        return out

    def search_many(self, queries, *, threshold=0.0, do_containment=False, do_max_containment=False, best_only=False):
        """[self.search(q, ...) for q in queries] from one pass over the set: per query [(score, row)] best first.  The device drops
        the pairs whose common count cannot reach the threshold (many_need); the float test and the ranking are the host's, by the
        code rank_search_hits uses.  Sets of different scaled are scored at the coarser one (both sizes downsampled)."""
        if do_containment and do_max_containment:
            raise TypeError("'do_containment' and 'do_max_containment' cannot both be True")
        if not isinstance(queries, SketchSet):
            raise TypeError("the queries of a many-query search are a SketchSet")
        q_scaled, scaled = queries.params[3], self.params[3]
        if (do_containment or do_max_containment) and not q_scaled:
            raise TypeError("this search requires a scaled signature")
        q_sizes = queries.sizes if q_scaled == scaled else queries._sizes_at(max(q_scaled, scaled))
        need = many_need(q_sizes, threshold, do_containment=do_containment, do_max_containment=do_max_containment)
        hits = self._many_hits(queries, need)
        q_sizes, row_sizes = hits.query_sizes, hits.row_sizes
        out = []
        for q, (rows, common) in enumerate(hits.per_query(len(queries))):
            score = score_hits(common, row_sizes[rows], int(q_sizes[q]), do_containment=do_containment, do_max_containment=do_max_containment)
            out.append(rank_scored(score, rows, threshold=threshold, best_only=best_only))
        return out

    # ---- gather of many queries in one call (csrc/gather_many.hip) -------------------------------------------------------------
    def _many_gather(self, queries, threshold_bp):
        if not isinstance(queries, SketchSet):
            raise TypeError("the queries of a many-query search are a SketchSet")
        # search.py:15-37: the loop stops below threshold_bp / scaled hashes, taken at the scaled the two sets meet at (a set that
        # is not scaled is refused by the call itself, in the order overlaps_many checks two sets)
        common_scaled = max(queries.params[3], self.params[3])
        thr = math.ceil(float(threshold_bp) / common_scaled) if threshold_bp and common_scaled else 0
        res = _ManyGather._from_objptr(rustcall(lib.smgpu_sketchset_gather_many, self._get_objptr(), queries._get_objptr(), int(thr)))
        res._n_queries = len(queries)
        return res

    def gather_many(self, queries, threshold_bp=0):
        """[self.gather(q, threshold_bp) for q in queries] from one call: per query [(row, |intersect|)] in rank order.  One pass over
        the set finds every query's candidates, then the min-set-cover loops of all queries run side by side on the GPU, a
        workgroup a query.  Sets of different scaled meet at the coarser one (both sides downsampled)."""
        return self._many_gather(queries, threshold_bp).per_query()


    # ---- the result rows of gather (csrc/gather_rows.hip) ------------------------------------------------------------------------
    def gather_stats_many(self, queries, threshold_bp=0, abunds=None, ignore_abundance=False):
        """gather_many, and for every pick the integers its result row is made of -> GatherStats.  One more pass over the resident
        sets: per pick |query ∩ row|, the query hashes it covered first (the rank's "remaining query ∩ match") and the sum of
        their abundances, and those abundances in hash order.  abunds: a flat uint64 array aligned with the queries' hashes (row
        after row, ascending within a row), or one array per query; None: every abundance is 1 and rows() gives the columns of
        an ignore-abundance gather.  Queries that are an abundance set bring their own: with abunds None their resident column is
        what the pass reads (no host array, no upload); ignore_abundance=True gives the all-ones rows instead."""
        if not isinstance(queries, SketchSet):
            raise TypeError("the queries of a many-query search are a SketchSet")
        if ignore_abundance:
            abunds = None
        common_scaled = max(queries.params[3], self.params[3])
        thr = math.ceil(float(threshold_bp) / common_scaled) if threshold_bp and common_scaled else 0
        if abunds is None and not ignore_abundance and queries.track_abundance:
            ptr = rustcall(lib.smgpu_sketchset_gather_rows_many_resident, self._get_objptr(), queries._get_objptr(), None, int(thr), 1)
            return GatherStats._from_handle(ptr, self, queries=queries, with_abundance=True, query_scaled=queries.params[3])
        flat = None
        if abunds is not None:
            if isinstance(abunds, (list, tuple)):
                if len(abunds) != len(queries):
                    raise ValueError("one abundance array per query is needed")
                sizes = queries.sizes
                if any(len(a) != int(n) for a, n in zip(abunds, sizes)):
                    raise ValueError("a query's abundances must be as many as its hashes")
                abunds = np.concatenate([np.asarray(a, dtype=np.uint64) for a in abunds]) if len(abunds) else np.zeros(0, dtype=np.uint64)
            flat = np.ascontiguousarray(abunds, dtype=np.uint64)
            if flat.shape != (queries.total_hashes,):
                raise ValueError("the abundances must be as many as the queries' hashes")
        ptr = rustcall(lib.smgpu_sketchset_gather_rows_many, self._get_objptr(), queries._get_objptr(),
                       flat.ctypes.data_as(C.c_void_p) if flat is not None and len(flat) else None, int(thr))
        return GatherStats._from_handle(ptr, self, queries=queries, with_abundance=abunds is not None, query_scaled=queries.params[3])

    def gather_stats(self, query_mh, threshold_bp=0, ignore_abundance=False):
        """gather(query_mh), and the integers of its result rows -> GatherStats of one query: the one-query gather, then the same
        pass.  The abundances are the sketch's own when it tracks them and ignore_abundance is not set."""
        scaled = query_mh.scaled
        if not scaled:
            raise ValueError("gather requires scaled signatures")
        with_abundance = bool(query_mh.track_abundance and not ignore_abundance)
        common_scaled = max(scaled, self.params[3])
        thr = math.ceil(float(threshold_bp) / common_scaled) if threshold_bp else 0
        mh = query_mh if with_abundance else query_mh.flatten()
        ptr = rustcall(lib.smgpu_sketchset_gather_rows, self._get_objptr(), mh._get_objptr(), int(thr))
        return GatherStats._from_handle(ptr, self, queries=None, with_abundance=with_abundance, query_scaled=scaled)


    # ---- set algebra on the resident CSR (csrc/setops.hip): every method returns a NEW set, this one is unchanged ------------------
    def merge(self, groups=None, *, min_rows=1, names=None, count_rows=False):
        """The rows merged by group -> a set of G rows: row g holds the hashes that at least min_rows rows of group g hold.
        groups: one integer per row, any order, values 0 .. G - 1 with G = max + 1 (None: all rows in one group).  min_rows=1 is
        the union (MinHash.merge, `sig merge --flatten`), min_rows="all" the intersection of a group's rows (`sig intersect`).  A
        group without rows, or of fewer rows than an integer min_rows, gives an empty row.  A num set gives the num smallest of
        the union, and takes min_rows=1 only.  names: one name per group.
        An abundance set gives an abundance set: a kept hash's abundance is the sum (uint64, wrapping) of the abundances of the
        group's rows that hold it (MinHash.merge, `sig merge`).  count_rows=True, on a flat set: an abundance set whose abundance
        is the number of rows of the group that hold the hash; on an abundance set it is a ValueError."""
        _check_count_rows(count_rows, self.track_abundance)
        g_arr, n_groups, need, need_all, name_arr = _merge_plan(len(self), self.params[4], groups, min_rows, names)
        return SketchSet._from_objptr(self._methodcall(lib.smgpu_sketchset_merge_groups_values, g_arr.ctypes.data_as(C.c_void_p) if g_arr is not None else None,
                                                       n_groups, need.ctypes.data_as(C.c_void_p) if need is not None else None, need_all, name_arr,
                                                       int(bool(count_rows))))

    def _filter(self, other, keep_present):
        from .minhash import MinHash
        if isinstance(other, MinHash):
            flat = other.flatten()                                      # (held until the call returns: a flattened copy is a new object)
            return SketchSet._from_objptr(self._methodcall(lib.smgpu_sketchset_filter_sketch, flat._get_objptr(), keep_present))
        if not isinstance(other, SketchSet):
            raise TypeError("the other side is a MinHash or a SketchSet")
        _check_other_rows(len(self), len(other))
        return SketchSet._from_objptr(self._methodcall(lib.smgpu_sketchset_filter, other._get_objptr(), keep_present))

    def subtract(self, other):
        """Every row without the hashes of `other` (MinHash.remove_many, `sig subtract`): a MinHash or a SketchSet of one row is
        taken from every row, a SketchSet of len(self) rows row by row.  Parameters must match (ksize, moltype, scaled, seed; the
        errors are count_common's): downsample first where the scaled differ."""
        return self._filter(other, 0)

    def intersect(self, other):
        "every row's hashes that `other` holds too (MinHash.intersection, `sig intersect`); `other` as for subtract"
        return self._filter(other, 1)

    def downsample(self, scaled):
        "every row cut to the hashes a sketch of `scaled` keeps (MinHash.downsample); a smaller scaled, or a num set, is a ValueError"
        from .minhash import _get_max_hash_for_scaled
        _check_downsample(self.params, scaled)
        return SketchSet._from_objptr(self._methodcall(lib.smgpu_sketchset_downsample, _get_max_hash_for_scaled(int(scaled))))


def _merge_plan(n_rows, num, groups, min_rows, names):
    """The arguments of SketchSet.merge checked and turned into what smgpu_sketchset_merge_groups takes -> (groups u32 or None,
    n_groups, need u32 per group or None, need_all, names array or None).  No device is needed."""
    if groups is None:
        g_arr, n_groups = None, 1
    else:
        g = np.asarray(groups)
        if g.ndim != 1 or len(g) != n_rows:
            raise ValueError("one group number per row of the set is needed")
        if len(g) and not np.issubdtype(g.dtype, np.integer):
            raise ValueError("group numbers are integers")
        g = g.astype(np.int64) if len(g) else np.zeros(0, dtype=np.int64)
        if len(g) and int(g.min()) < 0:
            raise ValueError("group numbers are not negative")
        n_groups = int(g.max()) + 1 if len(g) else 0
        if n_groups > 0xfffffffe:
            raise ValueError("group numbers fit 32 bits")
        g_arr = np.ascontiguousarray(g, dtype=np.uint32)
    if isinstance(min_rows, str):
        if min_rows != "all":
            raise ValueError('min_rows is a count, or "all"')
        need, need_all = None, 1
    else:
        if int(min_rows) != min_rows or int(min_rows) < 1:
            raise ValueError("min_rows is at least 1")
        need_all = 0
        need = None if int(min_rows) == 1 else np.full(max(n_groups, 1), min(int(min_rows), 0xffffffff), dtype=np.uint32)
    if num and (need_all or need is not None):
        raise ValueError("a num set merges to the union of its rows only (min_rows=1)")
    name_arr = None
    if names is not None:
        enc = [v.encode("utf-8") if isinstance(v, str) else bytes(v) for v in names]
        if len(enc) != n_groups:
            raise ValueError("one name per group is needed")
        name_arr = (C.c_char_p * max(n_groups, 1))(*enc)
    return g_arr, n_groups, need, need_all, name_arr


def _check_count_rows(count_rows, track_abundance):
    if count_rows and track_abundance:
        raise ValueError("count_rows counts the rows of a flat set: this set carries abundance and its merge sums them (flatten() first)")


def _need_abundance_set(track_abundance, what):
    if not track_abundance:
        raise ValueError(f"{what} needs a set that carries abundance (SketchSet(minhashes, track_abundance=True), from_csr(..., abunds=...))")


def _check_inflate(receiver_tracks, other_tracks):
    "the reference's order (minhash.py:1078-1091): the receiver is flat, the other side carries the abundances"
    if receiver_tracks or not other_tracks:
        raise ValueError("inflate operates on a flat MinHash and takes a MinHash object with track_abundance=True")


def _abund_range(min_abundance, max_abundance):
    "-> (lo, hi) as the C entry takes them: no upper bound is 2^64 - 1"
    lo = int(min_abundance)
    hi = 0xffffffffffffffff if max_abundance is None else int(max_abundance)
    if lo < 0 or hi < 0 or lo > 0xffffffffffffffff or hi > 0xffffffffffffffff:
        raise ValueError("abundance bounds are unsigned 64-bit integers")
    return lo, hi


def _check_csr_abunds(abunds, hashes):
    "from_csr: the abundance tensor is 64-bit integers, one per hash, on the device"
    if abunds is None:
        return
    if abunds.is_floating_point() or abunds.is_complex() or abunds.element_size() != 8:
        raise ValueError("the abundances are 64-bit integers (int64 / uint64: the bits are the values)")
    if abunds.dim() != 1 or abunds.numel() != hashes.numel():
        raise ValueError(f"the abundances must be as many as the hashes: {abunds.numel()} for {hashes.numel()}")
    if not abunds.is_cuda or not abunds.is_contiguous():
        raise ValueError("the abundances are a contiguous device tensor")


def _check_other_rows(n_rows, n_other):
    "subtract / intersect: the other set has one row, or one per row of this set"
    if n_other != 1 and n_other != n_rows:
        raise ValueError(f"the other set has {n_other} rows: one row, or the {n_rows} of this set, are needed")


def _check_downsample(params, scaled):
    "the errors of MinHash.downsample(scaled=...) for a set of these params (ksize, moltype, seed, scaled, num)"
    cur, num = params[3], params[4]
    if num or not cur:
        raise ValueError("cannot downsample a num MinHash using scaled")
    if cur > scaled:
        raise ValueError(f"new scaled {scaled} is lower than current sample scaled {cur}")


class _ManyGather(RustObject):
    "the picks of a many-query gather on the host (smgpu_manygather_*): offsets per query into rows / isect, in rank order"
    __dealloc_func__ = lib.smgpu_manygather_free
    _n_queries = 0

    def _array(self, func, n, ctype, dtype):
        if not n:
            return np.zeros(0, dtype=dtype)
        return np.ctypeslib.as_array(C.cast(func(self._get_objptr()), C.POINTER(ctype)), shape=(n,)).copy()

    @property
    def offsets(self):
        return self._array(lib.smgpu_manygather_offsets, self._n_queries + 1, C.c_uint64, np.uint64)

    scaled = property(lambda self: lib.smgpu_manygather_scaled(self._get_objptr()))

    @property
    def stats(self):
        """ms of the candidate pass, the fill, the sort and the rounds kernel (device), of the one-query way out and of the whole
        call (host); queries that took the way out; batches"""
        out = (C.c_double * 8)()
        lib.smgpu_manygather_stats(self._get_objptr(), out)
        return dict(zip(("candidates_ms", "fill_ms", "sort_ms", "rounds_ms", "way_out_ms", "call_ms", "way_out_queries", "batches"), out))

    def per_query(self):
        "[(row, |intersect|)] in rank order for query 0, 1, .."
        off = self.offsets
        total = int(off[-1]) if len(off) else 0
        rows = self._array(lib.smgpu_manygather_rows, total, C.c_uint32, np.uint32).tolist()
        isect = self._array(lib.smgpu_manygather_isect, total, C.c_uint32, np.uint32).tolist()
        return [list(zip(rows[int(off[q]):int(off[q + 1])], isect[int(off[q]):int(off[q + 1])])) for q in range(self._n_queries)]


class GatherStats:
    """The integers behind the rows of `sourmash gather` for the picks of one or many queries, as numpy arrays (what
    smgpu_sketchset_gather_rows_many / smgpu_sketchset_gather_rows leave on the host), and the rows themselves.

    offsets (queries + 1) cuts the per-pick arrays: pick_rows, isect (= the hashes the pick owns), orig_common, weighted;
    abund_offsets (picks + 1) cuts abund_values; query_sizes and total_weighted are per query, row_sizes per row of the set, all at
    `scaled`, the scaled the two sets meet at.  with_abundance: the queries' abundances were given."""
    FIELDS = ("offsets", "pick_rows", "isect", "orig_common", "weighted", "abund_offsets", "abund_values", "query_sizes", "row_sizes", "total_weighted")

    def __init__(self, *, offsets, pick_rows, isect, orig_common, weighted, abund_offsets, abund_values, query_sizes, row_sizes, total_weighted,
                 scaled, with_abundance, ksize=None, moltype=None, query_scaled=None, match_info=None, query_info=None, stats=None):
        self.offsets, self.abund_offsets = np.asarray(offsets, dtype=np.uint64), np.asarray(abund_offsets, dtype=np.uint64)
        self.pick_rows, self.isect, self.orig_common = (np.asarray(a, dtype=np.uint32) for a in (pick_rows, isect, orig_common))
        self.weighted, self.abund_values = np.asarray(weighted, dtype=np.uint64), np.asarray(abund_values, dtype=np.uint64)
        self.query_sizes, self.row_sizes, self.total_weighted = (np.asarray(a, dtype=np.uint64) for a in (query_sizes, row_sizes, total_weighted))
        self.scaled, self.with_abundance = int(scaled), bool(with_abundance)
        self.query_scaled = int(query_scaled) if query_scaled else int(scaled)
        self.ksize, self.moltype = ksize, moltype
        self.match_info, self.query_info = match_info, query_info
        self.stats = stats or {}
        self._db = self._queries = None

    @classmethod
    def _from_handle(cls, ptr, db, *, queries, with_abundance, query_scaled):
        try:
            m, n = lib.smgpu_gatherrows_queries(ptr), lib.smgpu_gatherrows_n_rows(ptr)

            def array(func, count, ctype, dtype):
                if not count:
                    return np.zeros(0, dtype=dtype)
                return np.ctypeslib.as_array(C.cast(func(ptr), C.POINTER(ctype)), shape=(count,)).copy()
            offsets = array(lib.smgpu_gatherrows_offsets, m + 1, C.c_uint64, np.uint64)
            picks = int(offsets[-1])
            abund_offsets = array(lib.smgpu_gatherrows_abund_offsets, picks + 1, C.c_uint64, np.uint64)
            stats = (C.c_double * 5)()
            lib.smgpu_gatherrows_stats(ptr, stats)
            ksize, moltype = db.params[0], db.params[1]
            out = cls(offsets=offsets, pick_rows=array(lib.smgpu_gatherrows_rows, picks, C.c_uint32, np.uint32),
                      isect=array(lib.smgpu_gatherrows_isect, picks, C.c_uint32, np.uint32),
                      orig_common=array(lib.smgpu_gatherrows_orig_common, picks, C.c_uint32, np.uint32),
                      weighted=array(lib.smgpu_gatherrows_weighted, picks, C.c_uint64, np.uint64), abund_offsets=abund_offsets,
                      abund_values=array(lib.smgpu_gatherrows_abund_values, int(abund_offsets[-1]), C.c_uint64, np.uint64),
                      query_sizes=array(lib.smgpu_gatherrows_query_sizes, m, C.c_uint64, np.uint64),
                      row_sizes=array(lib.smgpu_gatherrows_row_sizes, n, C.c_uint64, np.uint64),
                      total_weighted=array(lib.smgpu_gatherrows_total_weighted, m, C.c_uint64, np.uint64),
                      scaled=lib.smgpu_gatherrows_scaled(ptr), with_abundance=with_abundance, ksize=ksize, moltype=moltype, query_scaled=query_scaled,
                      stats=dict(zip(("gather_ms", "owner_ms", "tally_ms", "sort_ms", "call_ms"), stats)))
        finally:
            lib.smgpu_gatherrows_free(ptr)
        out._db, out._queries = db, queries
        return out

    def __len__(self):
        return len(self.offsets) - 1

    def per_query(self):
        "[(row, |intersect|)] in rank order for query 0, 1, ..: what gather_many returns"
        off, rows, isect = self.offsets.tolist(), self.pick_rows.tolist(), self.isect.tolist()
        return [list(zip(rows[off[q]:off[q + 1]], isect[off[q]:off[q + 1]])) for q in range(len(self))]

    def _set_info(self):
        "name / filename / md5 of the set's rows and of the query set's rows, from the manifests and md5sums"
        if self.match_info is None and self._db is not None:
            used = sorted(set(self.pick_rows.tolist()))
            if used and getattr(self._db, "_md5_of_rows", None) is None:
                self._db._md5_of_rows = self._db.md5sums()              # (the rows of a set do not change: kept for the next call)
            md5, man = (self._db._md5_of_rows, self._db.manifest) if used else ([], [])
            self.match_info = {r: dict(name=man[r]["name"], filename=man[r]["filename"], md5=md5[r]) for r in used}
        if self.query_info is None and self._queries is not None:
            md5, man = self._queries.md5sums(), self._queries.manifest
            self.query_info = [dict(query_name=man[q]["name"], query_filename=man[q]["filename"], query_md5=md5[q][:8]) for q in range(len(self))]

    def rows_of(self, q, with_abundance=None):
        """The rows of query q: a list of dicts with the columns of GatherResult.gather_write_cols, == to the gatherresultdict of the
        reference's loop round by round.  with_abundance: whether this query's abundances count (None: as the call was made).  Integer and ratio columns are the expressions of GatherResult.build_gather_result on the
        device's integers, the abundance statistics np.mean / np.median / np.std of the pick's abundances in hash order, the ANI
        columns distance_utils.containment_to_distance on the containments of (original query, match), None -- not written -- when
        either sketch is too small for its size to be trusted (MinHash.size_is_accurate)."""
        from .distance_utils import containment_to_distance, set_size_exact_prob
        from .minhash import MinHash
        self._set_info()
        if with_abundance is None:
            with_abundance = self.with_abundance
        S, off = self.scaled, self.offsets
        accurate = {}

        def size_is_accurate(n):
            "MinHash.size_is_accurate of a sketch of n hashes at the common scaled"
            if n not in accurate:
                accurate[n] = set_size_exact_prob(n * S, S, relative_error=0.20) >= 0.95
            return accurate[n]
        q_len, total_w = int(self.query_sizes[q]), int(self.total_weighted[q])
        qinfo = dict(self.query_info[q]) if self.query_info is not None else {}
        ksize, moltype = qinfo.pop("ksize", self.ksize), qinfo.pop("moltype", self.moltype)
        remaining, sum_found, out = q_len, 0, []
        for rank, p in enumerate(range(int(off[q]), int(off[q + 1]))):
            row, oc, u = int(self.pick_rows[p]), int(self.orig_common[p]), int(self.isect[p])
            r_len, w = int(self.row_sizes[row]), int(self.weighted[p])
            sum_found += w
            d = dict(self.match_info[row]) if self.match_info is not None else {}
            d.update(qinfo)
            d.update(intersect_bp=oc * S, f_orig_query=oc / q_len, f_match=MinHash._debias(u, r_len, S) if r_len else 0.0,
                     f_unique_to_query=u / q_len, f_match_orig=MinHash._debias(oc, r_len, S) if r_len else 0.0, unique_intersect_bp=u * S,
                     gather_result_rank=rank, remaining_bp=remaining * S - u * S, query_bp=q_len * self.query_scaled, ksize=ksize, moltype=moltype,
                     scaled=S, query_n_hashes=q_len, sum_weighted_found=sum_found, total_weighted_hashes=total_w)
            if with_abundance:
                values = self.abund_values[int(self.abund_offsets[p]):int(self.abund_offsets[p + 1])].tolist()
                d.update(average_abund=float(np.mean(values)), median_abund=float(np.median(values)), std_abund=float(np.std(values)),
                         query_abundance=True, n_unique_weighted_found=w, f_unique_weighted=w / total_w)
            else:
                d.update(f_unique_weighted=d["f_unique_to_query"], query_abundance=False)
            # the ANI columns of (original query, match): FracMinHashComparison.estimate_all_containment_ani on these numbers
            q_ani = containment_to_distance(MinHash._debias(oc, q_len, S) if q_len else 0.0, ksize, S, n_unique_kmers=q_len * S,
                                            confidence=0.95, estimate_ci=False, prob_threshold=1e-3)
            m_ani = containment_to_distance(MinHash._debias(oc, r_len, S) if r_len else 0.0, ksize, S, n_unique_kmers=r_len * S,
                                            confidence=0.95, estimate_ci=False, prob_threshold=1e-3)
            if not size_is_accurate(q_len) or not size_is_accurate(r_len):
                q_ani.size_is_inaccurate = m_ani.size_is_inaccurate = True      # (MinHash.containment_ani: no ANI from such a pair)
            pair = None if None in (q_ani.ani, m_ani.ani) else (q_ani.ani, m_ani.ani)
            d.update(query_containment_ani=q_ani.ani, match_containment_ani=m_ani.ani,
                     average_containment_ani=None if pair is None else (pair[0] + pair[1]) / 2,
                     max_containment_ani=None if pair is None else max(pair),
                     potential_false_negative=bool(q_ani.p_exceeds_threshold or m_ani.p_exceeds_threshold))
            out.append({k: v for k, v in d.items() if v is not None})
            remaining -= u
        return out

    def rows(self):
        "[self.rows_of(q)] for query 0, 1, .."
        return [self.rows_of(q) for q in range(len(self))]


class _ManyHits(RustObject):
    "the hits of a many-query pass on the host (smgpu_manyhits_*): arrays ordered by (query, row), sizes at the common scaled"
    __dealloc_func__ = lib.smgpu_manyhits_free

    def _array(self, func, n, dtype):
        if not n:
            return np.zeros(0, dtype=dtype)
        return np.ctypeslib.as_array(C.cast(func(self._get_objptr()), C.POINTER(C.c_uint32 if dtype == np.uint32 else C.c_uint64)), shape=(n,)).copy()

    def __len__(self):
        return lib.smgpu_manyhits_len(self._get_objptr())

    queries = property(lambda self: self._array(lib.smgpu_manyhits_queries, len(self), np.uint32))
    rows = property(lambda self: self._array(lib.smgpu_manyhits_rows, len(self), np.uint32))
    common = property(lambda self: self._array(lib.smgpu_manyhits_common, len(self), np.uint32))
    scaled = property(lambda self: lib.smgpu_manyhits_scaled(self._get_objptr()))

    def _sizes(self, func, n):
        return self._array(func, n, np.uint64)

    @property
    def query_sizes(self):
        return self._sizes(lib.smgpu_manyhits_query_sizes, self._n_queries)

    @property
    def row_sizes(self):
        return self._sizes(lib.smgpu_manyhits_row_sizes, self._n_rows)

    @property
    def stats(self):
        "ms of the index build, the passes, the final sort (device) and the whole call (host); reruns; passes over the collection"
        out = (C.c_double * 6)()
        lib.smgpu_manyhits_stats(self._get_objptr(), out)
        return dict(zip(("build_ms", "kernel_ms", "sort_ms", "call_ms", "reruns", "passes"), out))

    def per_query(self, m):
        "(rows, common) of query 0, 1, .. m - 1"
        queries, rows, common = self.queries, self.rows, self.common
        cut = np.searchsorted(queries, np.arange(m + 1))
        return [(rows[cut[q]:cut[q + 1]], common[cut[q]:cut[q + 1]]) for q in range(m)]


class _DeviceCounter(RustObject):
    "c[d] = |query ∩ D_d| on the GPU (smgpu_counter_*)."
    __dealloc_func__ = lib.smgpu_counter_free

    def __init__(self, sketchset, query_mh):
        self._set = sketchset
        self._objptr = rustcall(lib.smgpu_counter_new, sketchset._get_objptr(), query_mh._get_objptr())

    def values(self):
        out = np.zeros(max(len(self._set), 1), dtype=np.uint64)
        self._methodcall(lib.smgpu_counter_get, out.ctypes.data_as(C.c_void_p))
        return out[:len(self._set)]

    def best(self):
        "-> (index, count) of the largest counter (ties: lowest index) or None"
        idx, cnt = C.c_uint64(0), C.c_uint64(0)
        ok = self._methodcall(lib.smgpu_counter_best, C.byref(idx), C.byref(cnt))
        return (idx.value, cnt.value) if ok else None

    def consume(self, intersect_mh):
        self._methodcall(lib.smgpu_counter_consume, intersect_mh._get_objptr())

    def set(self, index, value):
        self._methodcall(lib.smgpu_counter_set, index, value)

    def gather(self, threshold_hashes=0):
        "Every remaining round of the min-set-cover loop on the GPU -> (winner indices, |intersect| per round)."
        n = max(len(self._set), 1)
        idx, isect = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        k = self._methodcall(lib.smgpu_counter_gather, int(threshold_hashes), idx.ctypes.data_as(C.c_void_p),
                             isect.ctypes.data_as(C.c_void_p), n)
        return idx[:k], isect[:k]


def _check_select_parameters(**kw):
    "types of the 'select' arguments (index/__init__.py:1229-1270)"
    extra = set(kw) - {"ksize", "num", "moltype", "scaled", "abund", "picklist", "containment"}
    if extra:
        raise ValueError(f"unknown 'select' parameters: {extra}")
    for key in ("ksize", "scaled", "num"):
        v = kw.get(key)
        if v is not None and not isinstance(v, int):
            raise ValueError(f"{key} value '{v}' must be an integer, is: {type(v)}")
    moltype = kw.get("moltype")
    if moltype is not None and moltype not in ("DNA", "protein", "dayhoff", "hp"):
        raise ValueError(f"unknown moltype: {moltype}")
    for key in ("containment", "abund"):
        v = kw.get(key)
        if v is not None and not isinstance(v, bool):
            raise ValueError(f"{key} value '{v}' must be a bool, is: {type(v)}")


class SketchSetWriter(RustObject):
    """Signature file written from the device (smgpu_sigwriter_*): the counterpart of SketchSet.load and of the reference's
    SaveSignaturesToLocation (save_load.py:406-540).  The suffix of `path` chooses the form: `.zip` (gzip members
    `signatures/<md5>.sig.gz` and `SOURMASH-MANIFEST.csv`), `.gz` (the JSON array as one gzip member), anything else the JSON
    array.  Several sets may be added (k = 21, 31, 51 of one file); the file appears when the writer is closed without an error.

        with SketchSetWriter("out.zip") as w:
            w.add(set21)
            w.add(set31)"""
    __dealloc_func__ = lib.smgpu_sigwriter_free

    def __init__(self, path, compression=1):
        self._objptr = rustcall(lib.smgpu_sigwriter_new, os.fsencode(os.fspath(path)), int(compression))
        self._closed = False

    def add(self, sketchset, names=None, filenames=None):
        "the rows of a SketchSet; names / filenames: one string per row, in place of the set's manifest rows"
        def strings(values):
            if values is None:
                return None
            values = [v.encode("utf-8") if isinstance(v, str) else bytes(v) for v in values]
            if len(values) != len(sketchset):
                raise ValueError("one string per row of the set is needed")
            return (C.c_char_p * max(len(values), 1))(*values)
        self._methodcall(lib.smgpu_sigwriter_add, sketchset._get_objptr(), strings(names), strings(filenames))

    def close(self):
        if not self._closed:
            self._closed = True
            self._methodcall(lib.smgpu_sigwriter_close)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        return False


def select_signature(ss, *, ksize=None, moltype=None, scaled=0, num=0, containment=False, abund=None, picklist=None):
    "does the signature meet the requirements? (index/__init__.py:349-394)"
    mh = ss.minhash
    if ksize and ksize != mh.ksize:
        return False
    if moltype and moltype != mh.moltype:
        return False
    if containment:                              # containment needs scaled sketches; similarity does not
        if not scaled:
            raise ValueError("'containment' requires 'scaled' in Index.select'")
        if not mh.scaled:
            return False
    if scaled and mh.num:                        # 'scaled' and 'num' exclude each other
        return False
    if num and (mh.scaled or num != mh.num):
        return False
    if abund and not mh.track_abundance:         # a sketch with abundances can always be flattened
        return False
    if picklist is not None and ss not in picklist:
        return False
    return True


def _zero_overlap_never_matches(search_fn, q_size):
    "true for the Jaccard / containment searches of search.py: no shared hash -> score 0 -> never passes"
    try:
        return search_fn.score_fn(q_size, 0, 1, q_size + 1) == 0 and not search_fn.passes(0)
    except Exception:                                        # noqa: BLE001  (an unusual search object: score every row)
        return False


class Index:
    """Base of every collection of signatures: selection, the signature walk, and search / prefetch / gather on top
    of one `find` (index/__init__.py:58-346).  `find` here scores the query against ALL signatures of the walk with one
    overlap kernel when they are scaled sketches; results and their order are those of the reference's per-signature loop."""
    is_database = False
    manifest = None                  # set by classes that select through a manifest

    def __len__(self):
        raise NotImplementedError

    @property
    def location(self):
        return None

    def signatures(self):
        raise NotImplementedError

    def signatures_with_location(self):
        for ss in self.signatures():
            yield ss, self.location

    def _signatures_with_internal(self):
        "(signature, internal location) for ALL signatures, selection ignored (used to build manifests)"
        raise NotImplementedError

    def insert(self, signature):
        raise NotImplementedError

    def save(self, path):
        raise NotImplementedError

    @classmethod
    def load(cls, location):
        raise NotImplementedError

    def select(self, **kwargs):
        raise NotImplementedError

    # ---- batched scoring --------------------------------------------------------------------------
    def _walk(self):
        """The signatures of the walk with their locations and sketches, and the exception that cut it short (or
        None).  The reference touches one signature at a time, so a signature that cannot be produced or read fails
        only when the walk reaches it: everything in front of it is still scored and yielded first."""
        items, pending = [], None
        it = iter(self.signatures_with_location())
        while True:
            try:
                ss, loc = next(it)
                mh = ss.minhash
            except StopIteration:
                break
            except Exception as exc:                         # noqa: BLE001  (re-raised by find at this position)
                pending = exc
                break
            items.append((ss, loc, mh))
        return items, pending

    def _subject_set(self, query_scaled, items):
        "subject sketches flattened and downsampled to the query's scaled when finer (find :125-131), and their CSR"
        subj = [flatten_and_downsample_scaled(mh, query_scaled) for _, _, mh in items]
        return (SketchSet(subj) if subj else None), subj

    def _score_shared(self, search_fn, query_mh, items, subj, shared):
        "the results of find for scaled sketches, from shared[i] = |query ∩ subject i|"
        skip_zero = _zero_overlap_never_matches(search_fn, len(query_mh))
        for i, ((ss, loc, _), subj_mh) in enumerate(zip(items, subj)):
            if skip_zero and not shared[i]:
                continue
            # the query is downsampled to the subject's scaled when the subject is coarser (:129-131)
            q_mh = query_mh if subj_mh.scaled <= query_mh.scaled else flatten_and_downsample_scaled(query_mh, subj_mh.scaled)
            q_size, s_size = len(q_mh), len(subj_mh)
            # plain |Q ∩ D| is unchanged by downsampling either side to the coarser scaled
            n_shared = int(shared[i])
            total = q_size + s_size - n_shared
            score = search_fn.score_fn(q_size, n_shared, s_size, total)
            if search_fn.passes(score) and search_fn.collect(score, ss):
                yield IndexSearchResult(score, ss, loc)

    def _find_many(self, search_fns, queries):
        """[list(self.find(search_fns[i], queries[i]))] for scaled queries of one scaled, from ONE pass over the subjects' device CSR
        (SketchSet.overlaps_many) in place of one pass per query."""
        queries = list(queries)
        mhs = []
        for search_fn, query in zip(search_fns, queries):
            search_fn.check_is_compatible(query)
            assert not query.minhash.track_abundance
            mhs.append(query.minhash)
        if not queries:
            return []
        scaled = mhs[0].scaled
        if not scaled or any(mh.scaled != scaled for mh in mhs):
            raise ValueError("a search of many queries takes scaled queries of one scaled")
        items, pending = self._walk()
        if not all(mh.scaled for _, _, mh in items):
            raise ValueError("a search of many queries takes scaled signatures")
        sset, subj = self._subject_set(scaled, items)
        out = []
        if sset is not None:
            hits = sset._many_hits(SketchSet([mh.flatten() for mh in mhs]), 1)
            per_query = hits.per_query(len(mhs))
        for i, (search_fn, mh) in enumerate(zip(search_fns, mhs)):
            shared = np.zeros(len(items), dtype=np.uint64)
            if sset is not None:
                rows, common = per_query[i]
                shared[rows] = common
            out.append(list(self._score_shared(search_fn, mh, items, subj, shared)))
        if pending is not None:
            raise pending
        return out

    def search_many(self, queries, *, threshold=None, do_containment=False, do_max_containment=False, best_only=False):
        "[self.search(q, ...) for q in queries]: the same result objects in the same order, from one pass over the collection"
        if threshold is None:
            raise TypeError("'search' requires 'threshold'")
        queries = list(queries)
        fns = [make_jaccard_search_query(do_containment=do_containment, do_max_containment=do_max_containment, best_only=best_only,
                                         threshold=float(threshold)) for _ in queries]
        out = self._find_many(fns, queries)
        for matches in out:
            matches.sort(key=lambda x: -x.score)
        return out

    def prefetch_many(self, queries, threshold_bp, **kwargs):
        "[list(self.prefetch(q, threshold_bp)) for q in queries], from one pass over the collection"
        if not self:
            raise ValueError("no signatures to search")
        queries = list(queries)
        fns = [make_containment_query(q.minhash, threshold_bp, best_only=kwargs.get("best_only", False)) for q in queries]
        return self._find_many(fns, queries)

    def find(self, search_fn, query, **kwargs):
        search_fn.check_is_compatible(query)
        query_mh = query.minhash
        assert not query_mh.track_abundance
        items, pending = self._walk()
        if query_mh.scaled and all(mh.scaled for _, _, mh in items):
            sset, subj = self._subject_set(query_mh.scaled, items)
            shared = sset.overlaps(query_mh) if sset is not None else []
            yield from self._score_shared(search_fn, query_mh, items, subj, shared)
        else:
            # num sketches (or mixed): per-pair GPU intersections, like the reference loop
            for ss, loc, mh in items:
                if query_mh.scaled:
                    subj_mh = flatten_and_downsample_scaled(mh, query_mh.scaled)
                    q_mh = flatten_and_downsample_scaled(query_mh, subj_mh.scaled)
                else:
                    subj_mh = flatten_and_downsample_num(mh, query_mh.num)
                    q_mh = flatten_and_downsample_num(query_mh, subj_mh.num)
                n_shared, total = q_mh.intersection_and_union_size(subj_mh)
                score = search_fn.score_fn(len(q_mh), n_shared, len(subj_mh), total)
                if search_fn.passes(score) and search_fn.collect(score, ss):
                    yield IndexSearchResult(score, ss, loc)
        if pending is not None:
            raise pending

    def search(self, query, *, threshold=None, do_containment=False, do_max_containment=False, best_only=False, **kw):
        if threshold is None:
            raise TypeError("'search' requires 'threshold'")
        search_obj = make_jaccard_search_query(do_containment=do_containment, do_max_containment=do_max_containment,
                                               best_only=best_only, threshold=float(threshold))
        matches = list(self.find(search_obj, query, **kw))
        matches.sort(key=lambda x: -x.score)
        return matches

    def search_abund(self, query, *, threshold=None, **kw):
        if not query.minhash.track_abundance:
            raise TypeError("'search_abund' requires query signature with abundance information")
        if threshold is None:
            raise TypeError("'search_abund' requires 'threshold'")
        out = []
        for ss, loc in self.signatures_with_location():
            if not ss.minhash.track_abundance:
                raise TypeError("'search_abund' requires subject signatures with abundance information")
            score = query.similarity(ss, downsample=True)
            if score >= float(threshold):
                out.append(IndexSearchResult(score, ss, loc))
        out.sort(key=lambda x: -x.score)
        return out

    def prefetch(self, query, threshold_bp, **kwargs):
        if not self:
            raise ValueError("no signatures to search")
        search_fn = make_containment_query(query.minhash, threshold_bp, best_only=kwargs.get("best_only", False))
        yield from self.find(search_fn, query, **kwargs)

    def best_containment(self, query, threshold_bp=None, **kwargs):
        results = sorted(self.prefetch(query, threshold_bp, best_only=True, **kwargs),
                         key=lambda x: (-x.score, x.signature.md5sum()))
        return results[0] if results else None

    def peek(self, query_mh, *, threshold_bp=0):
        try:
            result = self.best_containment(SourmashSignature(query_mh), threshold_bp=threshold_bp)
        except ValueError:
            result = None
        if not result:
            return []
        return [result, flatten_and_intersect_scaled(result.signature.minhash, query_mh)]

    def consume(self, intersect_mh):
        pass

    def counter_gather(self, query, threshold_bp, **kwargs):
        "Prefetch, then hand every match to a CounterGather in ONE batched add (index/__init__.py:302-320)."
        prefetch_query = query.to_mutable()
        prefetch_query.minhash = prefetch_query.minhash.flatten()
        counter = CounterGather(prefetch_query)
        matches = list(self.prefetch(prefetch_query, threshold_bp, **kwargs))
        counter.add_many([m.signature for m in matches], locations=[m.location for m in matches])
        return counter

    def gather(self, query, threshold_bp=None, **kwargs):
        "Best containment match only (index/__init__.py:272-300)."
        if not query.minhash.scaled:
            raise ValueError("gather requires scaled signatures")
        res = self.best_containment(query, threshold_bp=threshold_bp, **kwargs)
        return [res] if res else []


class LinearIndex(Index):
    "An in-memory list of signatures searched exhaustively -- on the GPU, all at once (index/__init__.py:397-453)."

    def __init__(self, _signatures=None, filename=None):
        self._signatures = list(_signatures) if _signatures else []
        self.filename = filename
        self._packed = None          # (query scaled, number of subjects) -> (SketchSet, prepared minhashes)

    @property
    def location(self):
        return self.filename

    def signatures(self):
        yield from self._signatures

    def __bool__(self):
        return bool(self._signatures)

    def __len__(self):
        return len(self._signatures)

    def insert(self, node):
        self._signatures.append(node)
        self._packed = None

    def save(self, path):
        "All signatures as one JSON file (index/__init__.py:427-429)."
        with open(path, "wb") as fp:
            save_signatures_to_json(self.signatures(), fp)

    @classmethod
    def load(cls, location, filename=None):
        "From a JSON signature file; raises when it cannot be parsed (index/__init__.py:431-439)."
        si = load_signatures_from_json(location, do_raise=True)
        return cls(si, filename=location if filename is None else filename)

    def select(self, **kwargs):
        """New LinearIndex with the signatures that match the requirements; never raises for 'nothing matches'
        (index/__init__.py:441-453 over select_signature :349-394, parameters checked as in :1229-1270)."""
        _check_select_parameters(**kwargs)
        return LinearIndex([ss for ss in self._signatures if select_signature(ss, **kwargs)], self.filename)

    def _subject_set(self, query_scaled, items):
        "the list only changes through insert(): keep the device CSR between queries of the same scaled"
        key = (query_scaled, len(items))
        if self._packed is None or self._packed[0] != key:
            self._packed = (key,) + Index._subject_set(self, query_scaled, items)
        return self._packed[1], self._packed[2]

    def _native_gather_inputs(self, queries, threshold_bp, abundance_queries):
        """What one native many-query gather works on -> (items of the walk, their SketchSet at the queries' scaled, the queries'
        sketches), or None when the per-query loop has to be taken: the queries are not all scaled and of one scaled (and flat,
        unless abundance_queries), or a query or subject differs in its parameters or is coarser.  What the loop raises on the host
        -- an empty index, an empty query, an unattainable threshold_bp, a subject that cannot be read -- is raised here for the
        first offending query, before any device work."""
        mhs = [q.minhash for q in queries]
        if not queries or not all(mh.scaled and (abundance_queries or not mh.track_abundance) for mh in mhs) \
                or any(mh.scaled != mhs[0].scaled for mh in mhs):
            return None
        scaled = mhs[0].scaled
        items, pending = self._walk()

        def meets(mh):
            "the sketch can stand in one set with the first query: the same parameters, and not coarser"
            return mh.scaled and mh.scaled <= scaled and (mh.ksize, mh.moltype, mh.seed) == (mhs[0].ksize, mhs[0].moltype, mhs[0].seed)
        if not all(meets(mh) for mh in mhs) or not all(meets(mh) for _, _, mh in items):
            return None                                             # (whatever a mismatch raises, the loop raises it)
        for i, (query, mh) in enumerate(zip(queries, mhs)):
            # what counter_gather checks on the host, in its order (the counter takes any scaled query): the index, then the
            # prefetch's search object, on the flattened query it works with
            if not self:
                raise ValueError("no signatures to search")
            if mh.track_abundance:
                mh = mh.flatten()
                query = query.to_mutable()
                query.minhash = mh
            make_containment_query(mh, threshold_bp, best_only=False).check_is_compatible(query)
            if i == 0 and pending is not None:
                raise pending                                       # (the walk of the first query's prefetch ends on it)
        sset, _ = self._subject_set(scaled, items)
        return items, sset, mhs

    def gather_many(self, queries, threshold_bp=0):
        """[self.counter_gather(q, threshold_bp).gather_all(threshold_bp) for q in queries]: per query [(md5, |intersect|)] in rank
        order.  One native call (SketchSet.gather_many over the subjects' device CSR) when the queries are flat, scaled and of one
        scaled and every subject is at that scaled once flattened and downsampled; otherwise that loop itself.  What the loop
        raises -- an empty index, an empty query, an unattainable threshold_bp -- is raised for the first offending query, before
        any device work."""
        queries = list(queries)
        native = self._native_gather_inputs(queries, threshold_bp, abundance_queries=False)
        if native is None:
            return [self.counter_gather(q, threshold_bp).gather_all(threshold_bp) for q in queries]
        items, sset, mhs = native
        # The prefetch inside counter_gather keeps a subject by a float containment test, the device by the integer count
        # ceil(threshold_bp / scaled).  Correctly rounded division by the same positive len(query) is monotone, so the two can only
        # disagree on a subject whose count is below the integer threshold: never picked, and it changes no other counter.  Subjects
        # with the same md5 are one entry of the counter; as rows the later one falls to 0 with the first and is never picked.
        picks = sset.gather_many(SketchSet([mh.flatten() for mh in mhs]), threshold_bp)
        md5 = {}
        out = []
        for rows in picks:
            for row, _ in rows:
                if row not in md5:
                    md5[row] = items[row][0].md5sum()
            out.append([(md5[row], n) for row, n in rows])
        return out

    def gather_results_many(self, queries, threshold_bp=0, *, ignore_abundance=False):
        """[[r.gatherresultdict for r in GatherDatabases(q, [self.counter_gather(q, threshold_bp)], threshold_bp=threshold_bp,
        ignore_abundance=ignore_abundance)] for q in queries]: per query the rows of `sourmash gather`, every column.  One native
        call (SketchSet.gather_stats_many over the subjects' device CSR) under the conditions of gather_many -- scaled queries of
        one scaled and one set of parameters, every subject at that scaled once flattened and downsampled -- and queries with
        abundances are taken there too; otherwise that loop itself, with whatever it raises, in its order.  noident_mh / ident_mh
        and estimate_ani_ci=True are not offered here: they stay with GatherDatabases."""
        from .search import GatherDatabases
        queries = list(queries)
        native = self._native_gather_inputs(queries, threshold_bp, abundance_queries=True)
        if native is None:
            return [[r.gatherresultdict for r in GatherDatabases(q, [self.counter_gather(q, threshold_bp)], threshold_bp=threshold_bp,
                                                                 ignore_abundance=ignore_abundance)] for q in queries]
        items, sset, mhs = native
        with_abundance = [bool(mh.track_abundance and not ignore_abundance) for mh in mhs]
        abunds = None
        if all(with_abundance):
            # every query brings abundances that count: an abundance set, whose resident column the pass reads where it lies
            stats = sset.gather_stats_many(SketchSet(mhs, track_abundance=True), threshold_bp)
        else:
            if any(with_abundance):
                # MinHash.hashes is ascending, as the set's rows are; a query whose abundances do not count carries ones
                abunds = [np.fromiter(mh.hashes.values(), dtype=np.uint64, count=len(mh)) if w else np.ones(len(mh), dtype=np.uint64)
                          for mh, w in zip(mhs, with_abundance)]
            stats = sset.gather_stats_many(SketchSet([mh.flatten() for mh in mhs]), threshold_bp, abunds=abunds)
        # Subjects with the same md5 are one entry of the loop's counter: it keeps the first one's place and the LAST one's
        # signature and location (CounterGather._register), so a picked row -- the first of its kind -- reports the last subject
        # of the walk with its md5.  The same md5 means the same hashes, hence the same size at the common scaled: only rows of
        # a picked row's size are asked for their md5.
        md5 = {}

        def md5_of(row):
            if row not in md5:
                md5[row] = items[row][0].md5sum()
            return md5[row]
        stats.match_info = {}
        for row in sorted(set(stats.pick_rows.tolist())):
            same_size = np.flatnonzero(stats.row_sizes == stats.row_sizes[row]).tolist()
            ss, loc, _ = items[max(j for j in same_size if md5_of(j) == md5_of(row))]
            stats.match_info[row] = dict(name=ss.name, filename=loc if loc is not None else ss.filename, md5=md5_of(row))
        stats.query_info = [dict(query_name=q.name, query_filename=q.filename, query_md5=q.md5sum()[:8], ksize=mh.ksize, moltype=mh.moltype)
                            for q, mh in zip(queries, mhs)]
        return [stats.rows_of(q, with_abundance=w) for q, w in enumerate(with_abundance)]


class CounterGather:
    """Track overlaps between a query and candidate matches for min-set-cover gather.

    Same protocol as the reference class (add / peek / consume, keyed by md5 with
    first-inserted winning ties); the counters live on the GPU.  `add_many` is the
    batch extension: all overlaps in one kernel.
    """

    def __init__(self, query):
        query_mh = query.minhash
        if not query_mh.scaled:
            raise ValueError("gather requires scaled signatures")
        self.orig_query_mh = query_mh.copy().flatten()
        self.scaled = query_mh.scaled
        self.siglist = {}            # md5 -> signature, insertion ordered
        self.locations = {}
        self.query_started = 0
        self._pending = []           # signatures added since the device state was last built
        self._host_counts = {}       # md5 -> overlap, until the device counter exists
        self._dev = None             # (_DeviceCounter, [md5 in CSR order])

    # ---- loading ---------------------------------------------------------------------------------
    def add(self, ss, *, location=None, require_overlap=True):
        "Add one potential match (overlap counted against the original query on the GPU)."
        if self.query_started:
            raise ValueError("cannot add more signatures to counter after peek/consume")
        overlap = self.orig_query_mh.count_common(ss.minhash, True)
        if overlap:
            self._register(ss, overlap, location)
        elif require_overlap:
            raise ValueError("no overlap between query and signature!?")

    def add_many(self, siglist, *, locations=None, require_overlap=False):
        "Batch extension: overlaps of every candidate in one kernel launch."
        if self.query_started:
            raise ValueError("cannot add more signatures to counter after peek/consume")
        siglist = list(siglist)
        if not siglist:
            return
        mhs = [ss.minhash.flatten() for ss in siglist]
        for mh in mhs:                                   # compatibility as count_common(downsample=True) would check
            if mh.ksize != self.orig_query_mh.ksize or mh.moltype != self.orig_query_mh.moltype \
                    or mh.seed != self.orig_query_mh.seed:
                self.orig_query_mh.count_common(mh, True)   # raises the reference's error
        overlaps = _DeviceCounter(SketchSet(mhs), self.orig_query_mh).values()
        for i, ss in enumerate(siglist):
            if overlaps[i]:
                self._register(ss, int(overlaps[i]), locations[i] if locations else None)
            elif require_overlap:
                raise ValueError("no overlap between query and signature!?")

    def _register(self, ss, overlap, location):
        md5 = ss.md5sum()
        if md5 not in self.siglist:
            self._pending.append(md5)
        self._host_counts[md5] = overlap
        self.siglist[md5] = ss
        self.locations[md5] = location
        self.downsample(ss.minhash.scaled)

    def downsample(self, scaled):
        if scaled > self.scaled:
            self.scaled = scaled
        return self.scaled

    def signatures(self):
        yield from self.siglist.values()

    @property
    def union_found(self):
        found_mh = self.orig_query_mh.copy_and_clear()
        for ss in self.siglist.values():
            found_mh.add_many(flatten_and_intersect_scaled(ss.minhash, self.orig_query_mh))
        return found_mh

    # ---- device state ---------------------------------------------------------------------------------
    def _device(self):
        if self._dev is None:
            order = list(self.siglist)
            mhs = [self.siglist[m].minhash.flatten() for m in order]
            dev = _DeviceCounter(SketchSet(mhs), self.orig_query_mh)
            # |Q ∩ D| computed in one launch equals the add-time overlaps (plain set intersections)
            self._dev = (dev, order)
        return self._dev

    @property
    def counter(self):
        "md5 -> remaining overlap: a collections.Counter snapshot of the device counters, zero entries dropped."
        if not self.siglist:
            return Counter()
        dev, order = self._device()
        vals = dev.values()
        return Counter({m: int(v) for m, v in zip(order, vals) if v})

    # ---- gather protocol ---------------------------------------------------------------------------------
    def peek(self, cur_query_mh, *, threshold_bp=0):
        "Best remaining match for the current query, without changing the counters."
        self.query_started = 1
        if not self.siglist:
            return []
        dev, order = self._device()
        scaled = self.downsample(cur_query_mh.scaled)
        cur_query_mh = cur_query_mh.downsample(scaled=scaled)
        if not cur_query_mh:
            return []
        if cur_query_mh.contained_by(self.orig_query_mh, downsample=True) < 1:
            raise ValueError("current query not a subset of original query")
        try:
            threshold, n_threshold_hashes = calc_threshold_from_bp(threshold_bp, scaled, len(cur_query_mh))
        except ValueError:
            return []
        best = dev.best()                               # highest count, ties to the first inserted
        if best is None:
            return []
        idx, match_size = best
        if match_size < n_threshold_hashes:
            return []
        md5 = order[idx]
        match = self.siglist[md5]
        cont = cur_query_mh.contained_by(match.minhash, downsample=True)
        assert cont and cont >= threshold
        match_mh = match.minhash.downsample(scaled=scaled).flatten()
        intersect_mh = cur_query_mh & match_mh
        return (IndexSearchResult(cont, match, self.locations[md5]), intersect_mh)

    def consume(self, intersect_mh):
        "Subtract |intersect ∩ D_d| from every live counter (one kernel)."
        self.query_started = 1
        if not intersect_mh or not self.siglist:
            return
        dev, _ = self._device()
        dev.consume(intersect_mh)

    # ---- batch extension: the whole min-set-cover loop ---------------------------------------------------
    def gather_all(self, threshold_bp=0):
        """Run gather to exhaustion; -> list of (md5, |intersect|) in rank order.  Same decisions as
        GatherDatabases over this single counter, without building result objects.  When every sketch shares
        the query's scaled the whole loop is one native call (smgpu_counter_gather); otherwise it goes round
        by round through peek/consume."""
        if not self.siglist:
            return []
        scaled = self.orig_query_mh.scaled
        if all(ss.minhash.scaled == scaled for ss in self.siglist.values()):
            self.query_started = 1
            dev, order = self._device()
            # search.py:15-37: stop below threshold_bp / scaled hashes; integer counts compare against its ceiling
            thr = math.ceil(float(threshold_bp) / scaled) if threshold_bp else 0
            idx, isect = dev.gather(thr)
            return [(order[int(i)], int(c)) for i, c in zip(idx, isect)]
        out = []
        query_mh = self.orig_query_mh.to_mutable()
        while query_mh:
            res = self.peek(query_mh, threshold_bp=threshold_bp)
            if not res:
                break
            sr, intersect_mh = res
            self.consume(intersect_mh)
            out.append((sr.signature.md5sum(), len(intersect_mh)))
            scaled = max(query_mh.scaled, sr.signature.minhash.scaled)
            query_mh = query_mh.downsample(scaled=scaled).to_mutable() if scaled != query_mh.scaled else query_mh
            query_mh.remove_many(sr.signature.minhash.downsample(scaled=scaled).flatten())
        return out
