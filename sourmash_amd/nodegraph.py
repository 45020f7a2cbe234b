"""Nodegraph: khmer's Bloom filter of k-mers, the structure behind the internal nodes of sourmash's SBT databases.

A graph holds ``n_tables`` bit tables of prime sizes (the largest primes below ``starting_size``); a hash sets one bit per
table, at hash mod size.  k-mers are hashed with khmer's two-bit code (the smaller of the forward and reverse-complement
words), and the ``.ng`` file format is khmer's.  The host container is ``csrc/nodegraph_host.hpp``.

The public surface is that of sourmash's ``sourmash.nodegraph`` (the same class, methods and module functions), plus bulk
input that runs on the GPU (``csrc/nodegraph.hip``): ``add_sequence`` (records queued and counted in one launch when the
graph is next read), ``add_file`` (FASTA / FASTQ, plain or gzip, through the streaming ingest), ``add_device`` (a
``torch.uint8`` tensor already in GPU memory), ``update_many`` / ``matches_many`` (many sketches in one launch).  Bulk k-mer
input takes ksize 1 .. 32 and folds lower case to upper case; ``count(str)`` stays strict, as khmer is.  Whatever the mix of
single and bulk calls, the tables and ``n_occupied()`` equal what the same calls give one by one.
"""
import ctypes as C
import struct
import sys
from tempfile import NamedTemporaryFile

import numpy as np

from ._lowlevel import lib
from .minhash import to_bytes, MinHash
from .utils import RustObject, rustcall

__all__ = ["Nodegraph", "extract_nodegraph_info", "calc_expected_collisions"]


class Nodegraph(RustObject):
    """Bloom filter over k-mers: ``Nodegraph(ksize, starting_size, n_tables)``."""

    __dealloc_func__ = lib.nodegraph_free

    def __init__(self, ksize, starting_size, n_tables):
        self._objptr = rustcall(lib.nodegraph_with_tables, ksize, int(starting_size), n_tables)

    # ---- persistence (khmer's layout; gzip accepted when reading) -------------------------------------------------------
    @staticmethod
    def load(filename):
        return Nodegraph._from_objptr(rustcall(lib.nodegraph_from_path, to_bytes(filename)))

    @staticmethod
    def from_buffer(buf):
        data = bytes(buf)
        return Nodegraph._from_objptr(rustcall(lib.nodegraph_from_buffer, data, len(data)))

    def save(self, filename):
        "The plain layout."
        self._methodcall(lib.nodegraph_save, to_bytes(filename))

    def to_bytes(self, compression=1):
        "The file layout: plain for compression 0, else gzip at that level (above 9: 9)."
        n = C.c_size_t(0)
        ptr = self._methodcall(lib.nodegraph_to_buffer, min(max(int(compression), 0), 255), C.byref(n))
        try:
            return C.string_at(ptr, n.value)
        finally:
            lib.nodegraph_buffer_free(C.cast(ptr, C.c_void_p), n.value)

    # ---- the reference's surface ----------------------------------------------------------------------------------------
    def update(self, other):
        if isinstance(other, Nodegraph):
            return self._methodcall(lib.nodegraph_update, other._get_objptr())
        elif isinstance(other, MinHash):
            return self._methodcall(lib.nodegraph_update_mh, other._get_objptr())
        else:
            raise TypeError("Must be a Nodegraph or MinHash")

    def count(self, h):
        "A str is a k-mer (upper-case ACGT only, any length); anything else a 64-bit hash.  True if a bit was new."
        if isinstance(h, str):
            return self._methodcall(lib.nodegraph_count_kmer, to_bytes(h))
        return self._methodcall(lib.nodegraph_count, h)

    def get(self, h):
        "1 if the k-mer (str) or hash is in every table, else 0."
        if isinstance(h, str):
            return self._methodcall(lib.nodegraph_get_kmer, to_bytes(h))
        return self._methodcall(lib.nodegraph_get, h)

    def n_occupied(self):
        "Bits of the first table that were turned on."
        return self._methodcall(lib.nodegraph_noccupied)

    def ksize(self):
        return self._methodcall(lib.nodegraph_ksize)

    def hashsizes(self):
        n = C.c_size_t(0)
        ptr = self._methodcall(lib.nodegraph_hashsizes, C.byref(n))
        try:
            return [ptr[i] for i in range(n.value)]
        finally:
            lib.kmerminhash_slice_free(ptr, n.value)

    @property
    def expected_collisions(self):
        return self._methodcall(lib.nodegraph_expected_collisions)

    def matches(self, mh):
        "How many hashes of the MinHash are in the graph."
        if not isinstance(mh, MinHash):
            raise ValueError("mh must be a MinHash")
        return self._methodcall(lib.nodegraph_matches, mh._get_objptr())

    def to_khmer_nodegraph(self):
        "The same graph as a khmer Nodegraph (khmer must be installed)."
        import khmer
        loader = getattr(khmer, "load_nodegraph", None) or khmer.Nodegraph.load
        with NamedTemporaryFile(suffix=".ng") as f:
            self.save(f.name)
            return loader(f.name)

    # ---- comparisons (sketch/nodegraph.rs; not in the reference's C interface) ---------------------------------------------
    def _pair(self, fn, other):
        if not isinstance(other, Nodegraph):
            raise TypeError("other must be a Nodegraph")
        return self._methodcall(fn, other._get_objptr())

    def similarity(self, other):
        "Summed intersections over summed unions of the zipped tables."
        return self._pair(lib.smgpu_nodegraph_similarity, other)

    def containment(self, other):
        "Summed intersections over this graph's summed set bits."
        return self._pair(lib.smgpu_nodegraph_containment, other)

    # ---- bulk input on the GPU ----------------------------------------------------------------------------------------------
    def add_sequence(self, sequence, force=False):
        """Count every k-mer of one record (lower case folded).  force=False: a byte outside ACGTacgt raises (naming the first
        k-mer holding one) after the k-mers before it were counted; force=True: such k-mers are skipped."""
        data = to_bytes(sequence)
        self._methodcall(lib.smgpu_nodegraph_add_sequence, data, len(data), force)

    def flush(self):
        "Count the queued records now (every read does it anyway)."
        self._methodcall(lib.smgpu_nodegraph_flush)

    def add_file(self, path):
        "Every record of a FASTA / FASTQ file (plain or gzip), bad k-mers skipped.  Returns (records, bases)."
        records = C.c_uint64(0)
        bases = self._methodcall(lib.smgpu_nodegraph_add_file, to_bytes(path), C.byref(records))
        return records.value, bases

    def add_device(self, tensor):
        "A torch.uint8 GPU tensor of ASCII DNA; records separated by any byte outside ACGTacgt (e.g. a newline)."
        import torch
        if not (isinstance(tensor, torch.Tensor) and tensor.dtype == torch.uint8 and tensor.is_cuda):
            raise TypeError("add_device takes a torch.uint8 tensor on the GPU")
        t = tensor.contiguous()
        stream = torch.cuda.current_stream(t.device).cuda_stream
        self._methodcall(lib.smgpu_nodegraph_add_device, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(stream))

    @staticmethod
    def _sketch_set(sketches):
        from .index import SketchSet
        if isinstance(sketches, SketchSet):
            return sketches
        sketches = list(sketches)
        for mh in sketches:
            if not isinstance(mh, MinHash):
                raise TypeError("update_many / matches_many take a SketchSet or MinHash objects")
        return SketchSet(sketches)

    def update_many(self, sketches):
        "update(mh) for every sketch of a SketchSet (or a list of MinHash), in one launch."
        s = self._sketch_set(sketches)
        self._methodcall(lib.smgpu_nodegraph_update_sketchset, s._get_objptr())

    def matches_many(self, sketches):
        "matches(mh) for every sketch of a SketchSet (or a list of MinHash), in one launch: a numpy uint64 array."
        s = self._sketch_set(sketches)
        out = np.zeros(len(s), dtype=np.uint64)
        if len(s):
            self._methodcall(lib.smgpu_nodegraph_matches_sketchset, s._get_objptr(),
                             out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return out


# khmer's header up to the first table's size: "OXLI", version, table type, ksize, n_tables, occupied, size of table 0
_HEADER = struct.Struct("<4sBBIBQQ")


def extract_nodegraph_info(filename):
    """(ksize, size of the first table rounded to hundreds, n_tables, format version, table type, occupied bins) from the
    header of a nodegraph file; ValueError if it is not one."""
    try:
        with open(filename, "rb") as f:
            head = f.read(_HEADER.size)
        magic, version, ht_type, ksize, n_tables, occupied, table_size = _HEADER.unpack(head)
    except (OSError, struct.error) as e:
        raise ValueError(f"Node graph '{filename}' is corrupt ") from e
    if magic != b"OXLI":
        raise ValueError(f"Node graph '{filename}' is corrupt (file type signature {magic!r})")
    return ksize, round(table_size, -2), n_tables, version, ht_type, occupied


def calc_expected_collisions(graph, force=False, max_false_pos=0.2):
    """The graph's expected false-positive rate.  Above max_false_pos a warning goes to stderr and, unless force is set,
    the program exits with status 1."""
    fp_all = graph.expected_collisions
    if fp_all > max_false_pos:
        sys.stderr.write(
            "**\n"
            "** ERROR: the graph structure is too small for this data set; increase its size.\n"
            "** Do not use these results!\n"
            f"** (estimated false positive rate {fp_all:.3f}; recommended at most {max_false_pos:.3f})\n"
            "**\n")
        if not force:
            raise SystemExit(1)
    return fp_all
