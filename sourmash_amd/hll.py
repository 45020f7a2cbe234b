"""HyperLogLog: an estimate of the number of distinct k-mers in a few KiB.

``HLL`` keeps 2^p one-byte registers (p from the requested relative error, 4 <= p <= 18; see ``csrc/hll_host.hpp``) and
answers cardinality, similarity, containment and intersection with maximum-likelihood estimators computed on the host.
Sequences reach the registers through the GPU kernel of ``csrc/hll.hip``: records passed to ``add_sequence`` are queued by the
library and hashed in one launch when the counter is next read, so a loop of short records costs no launch per call.

The public surface is that of sourmash's ``sourmash.hll.HLL`` (the same methods, exception types and messages), plus two
ways of feeding large inputs: ``add_file`` (FASTA / FASTQ, plain or gzip, through the streaming ingest) and ``add_device``
(a ``torch.uint8`` tensor already in GPU memory).
"""
import ctypes as C

from ._lowlevel import lib
from .minhash import to_bytes, MinHash
from .utils import RustObject, rustcall

__all__ = ["HLL"]

_NEEDS_HLL = "other must be a HyperLogLog"


class HLL(RustObject):
    """Distinct k-mer counter for DNA at one ksize (k-mers hashed canonically with MurmurHash3, seed 42)."""

    __dealloc_func__ = lib.hll_free

    def __init__(self, error_rate, ksize):
        # error 1301 (precision out of 4..18) surfaces as the mapped exception
        self._objptr = rustcall(lib.hll_with_error_rate, error_rate, ksize)

    # ---- what the counter is ----------------------------------------------------------------------------------------
    @property
    def ksize(self):
        return self._methodcall(lib.hll_ksize)

    @property
    def precision(self):
        "p: the counter holds 2^p registers"
        return self._methodcall(lib.smgpu_hll_precision)

    def registers(self):
        "A copy of the registers (bytes of length 2^p), queued records included."
        n = C.c_size_t(0)
        ptr = self._methodcall(lib.smgpu_hll_registers, C.byref(n))
        return C.string_at(ptr, n.value) if n.value else b""

    # ---- feeding it ---------------------------------------------------------------------------------------------------
    def add_sequence(self, sequence, force=False):
        """Count every k-mer of one record.  force=False: a byte outside ACGT raises (naming the first k-mer holding one)
        after the k-mers before it were counted; force=True: such k-mers are skipped."""
        data = to_bytes(sequence)
        self._methodcall(lib.hll_add_sequence, data, len(data), force)

    def add_kmer(self, kmer):
        "Count a single k-mer; its length must be the counter's ksize."
        k = self.ksize
        if len(kmer) == k:
            return self.add_sequence(kmer)
        raise ValueError(f"kmer to add is not {k} in length")

    def add(self, h):
        "A str is a k-mer; anything else is taken as a 64-bit hash value."
        if isinstance(h, str):
            return self.add_kmer(h)
        return self._methodcall(lib.hll_add_hash, h)

    count = add

    def get(self, h):
        raise NotImplementedError("HLL doesn't support membership query")

    def update(self, other):
        "Fold in another HLL (same ksize and size) or the hashes of a MinHash."
        if isinstance(other, HLL):
            fn = lib.hll_merge
        elif isinstance(other, MinHash):
            fn = lib.hll_update_mh
        else:
            raise TypeError("Must be a HyperLogLog or MinHash")
        self._methodcall(fn, other._get_objptr())

    # ---- estimates ----------------------------------------------------------------------------------------------------
    def cardinality(self):
        return self._methodcall(lib.hll_cardinality)

    __len__ = cardinality

    def _joint(self, fn, other):
        if not isinstance(other, HLL):
            raise TypeError(_NEEDS_HLL)
        return self._methodcall(fn, other._get_objptr())

    def similarity(self, other):
        "Estimated |A n B| / |A u B|."
        return self._joint(lib.hll_similarity, other)

    def containment(self, other):
        "Estimated |A n B| / |A|."
        return self._joint(lib.hll_containment, other)

    def intersection(self, other):
        "Estimated |A n B|."
        return self._joint(lib.hll_intersection_size, other)

    def matches(self, mh):
        "Estimated k-mers shared with the hashes of a MinHash (put in a counter of error rate 0.01)."
        if isinstance(mh, MinHash):
            return self._methodcall(lib.hll_matches, mh._get_objptr())
        raise ValueError("mh must be a MinHash")

    # ---- persistence: "HLL", version, p, q, ksize, registers (gzip accepted when reading) --------------------------------
    @classmethod
    def load(cls, filename):
        return cls._from_objptr(rustcall(lib.hll_from_path, to_bytes(filename)))

    @classmethod
    def from_buffer(cls, buf):
        data = bytes(buf)
        return cls._from_objptr(rustcall(lib.hll_from_buffer, data, len(data)))

    def save(self, filename):
        self._methodcall(lib.hll_save, to_bytes(filename))

    def to_bytes(self, compression=1):
        "The file layout, gzip-compressed (level 1 whatever `compression` says, as sourmash does)."
        n = C.c_size_t(0)
        ptr = self._methodcall(lib.hll_to_buffer, C.byref(n))
        try:
            return C.string_at(ptr, n.value)
        finally:
            lib.nodegraph_buffer_free(C.cast(ptr, C.c_void_p), n.value)

    # ---- bulk input -----------------------------------------------------------------------------------------------------
    def add_file(self, path):
        "Every record of a FASTA / FASTQ file (plain or gzip), bad k-mers skipped.  Returns (records, bases)."
        records = C.c_uint64(0)
        bases = self._methodcall(lib.smgpu_hll_add_file, to_bytes(path), C.byref(records))
        return records.value, bases

    def add_device(self, tensor):
        "A torch.uint8 GPU tensor of ASCII DNA; records separated by any byte outside ACGTacgt (e.g. a newline)."
        import torch
        if not (isinstance(tensor, torch.Tensor) and tensor.dtype == torch.uint8 and tensor.is_cuda):
            raise TypeError("add_device takes a torch.uint8 tensor on the GPU")
        t = tensor.contiguous()
        stream = torch.cuda.current_stream(t.device).cuda_stream
        self._methodcall(lib.smgpu_hll_add_device, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(stream))
