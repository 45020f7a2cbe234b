/*
 * sourmash_amd.h -- C-ABI of libsourmash_amd.so, the MI355X-native FracMinHash engine.
 *
 * PART 1 is a drop-in for the hot-path subset of the reference's cffi boundary
 * (reference header: include/sourmash.h, generated from the Rust shims under src/core/src/ffi/).
 * Every declaration has the reference's name, argument order, ownership rule
 * and error convention; the comment on each group cites the reference lines it
 * replaces.  A maintainer switches the path over by loading this library where
 * `sourmash._lowlevel.lib` is loaded today.
 *
 * PART 2 are additive batch entry points (prefix smgpu_) that collapse the
 * reference's per-record / per-pair / per-round Python loops into single calls
 * on device-resident data.  Plain pointers and sizes only -- no torch types.
 *
 * Error convention (src/core/src/ffi/utils.rs:17-19,58-83,195-207;
 * src/sourmash/utils.py:65-78): a fallible function stores its error in
 * thread-local state and returns an all-zero value; callers bracket calls with
 * sourmash_err_clear() / sourmash_err_get_last_code().  There is NO CPU
 * fallback: k-mer hashing and sketch intersection run on the GPU or fail with
 * SOURMASH_ERROR_CODE_INTERNAL.
 */
#ifndef SOURMASH_AMD_H_INCLUDED
#define SOURMASH_AMD_H_INCLUDED

#include <stdarg.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdlib.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ======================= PART 1: reference-compatible ABI ======================= */

/* include/sourmash.h:11-17 (src/core/src/ffi/mod.rs:33-68) */
/* (anonymous enum + integer typedef: identical ABI to the reference's `enum X {..}; typedef uint32_t X;`,
 * and also valid C++) */
enum {
  HASH_FUNCTIONS_MURMUR64_DNA = 1,
  HASH_FUNCTIONS_MURMUR64_PROTEIN = 2,
  HASH_FUNCTIONS_MURMUR64_DAYHOFF = 3,
  HASH_FUNCTIONS_MURMUR64_HP = 4,
};
typedef uint32_t HashFunctions;

/* include/sourmash.h:19-53 (src/core/src/errors.rs:101-143) -- values are ABI */
enum {
  SOURMASH_ERROR_CODE_NO_ERROR = 0,
  SOURMASH_ERROR_CODE_PANIC = 1,
  SOURMASH_ERROR_CODE_INTERNAL = 2,
  SOURMASH_ERROR_CODE_MSG = 3,
  SOURMASH_ERROR_CODE_UNKNOWN = 4,
  SOURMASH_ERROR_CODE_MISMATCH_K_SIZES = 101,
  SOURMASH_ERROR_CODE_MISMATCH_DNA_PROT = 102,
  SOURMASH_ERROR_CODE_MISMATCH_SCALED = 103,
  SOURMASH_ERROR_CODE_MISMATCH_SEED = 104,
  SOURMASH_ERROR_CODE_MISMATCH_SIGNATURE_TYPE = 105,
  SOURMASH_ERROR_CODE_NON_EMPTY_MIN_HASH = 106,
  SOURMASH_ERROR_CODE_MISMATCH_NUM = 107,
  SOURMASH_ERROR_CODE_NEEDS_ABUNDANCE_TRACKING = 108,
  SOURMASH_ERROR_CODE_CANNOT_UPSAMPLE_SCALED = 109,
  SOURMASH_ERROR_CODE_NO_MIN_HASH_FOUND = 110,
  SOURMASH_ERROR_CODE_EMPTY_SIGNATURE = 111,
  SOURMASH_ERROR_CODE_MULTIPLE_SKETCHES_FOUND = 112,
  SOURMASH_ERROR_CODE_INVALID_DNA = 1101,
  SOURMASH_ERROR_CODE_INVALID_PROT = 1102,
  SOURMASH_ERROR_CODE_INVALID_CODON_LENGTH = 1103,
  SOURMASH_ERROR_CODE_INVALID_HASH_FUNCTION = 1104,
  SOURMASH_ERROR_CODE_READ_DATA = 1201,
  SOURMASH_ERROR_CODE_STORAGE = 1202,
  SOURMASH_ERROR_CODE_HLL_PRECISION_BOUNDS = 1301,
  SOURMASH_ERROR_CODE_ANI_ESTIMATION_ERROR = 1401,
  SOURMASH_ERROR_CODE_IO = 100001,
  SOURMASH_ERROR_CODE_UTF8_ERROR = 100002,
  SOURMASH_ERROR_CODE_PARSE_INT = 100003,
  SOURMASH_ERROR_CODE_SERDE_ERROR = 100004,
  SOURMASH_ERROR_CODE_NIFFLER_ERROR = 100005,
  SOURMASH_ERROR_CODE_CSV_ERROR = 100006,
  SOURMASH_ERROR_CODE_ROCKS_DB_ERROR = 100007,
};
typedef uint32_t SourmashErrorCode;

/* opaque handles, include/sourmash.h:55-69: created by *_new / *_from_params,
 * owned by the caller, released by *_free (NULL tolerated, ffi/utils.rs:50-55) */
typedef struct SourmashComputeParameters SourmashComputeParameters;
typedef struct SourmashKmerMinHash SourmashKmerMinHash;
typedef struct SourmashSignature SourmashSignature;
typedef struct SourmashHyperLogLog SourmashHyperLogLog;
typedef struct SourmashNodegraph SourmashNodegraph;

/* include/sourmash.h:74-87 (ffi/utils.rs:209-316) */
typedef struct {
  char *data;
  uintptr_t len;
  bool owned;
} SourmashStr;

/* ---- library / errors: include/sourmash.h:416-467 (ffi/utils.rs:85-193) ---- */
void sourmash_init(void);
void sourmash_err_clear(void);
SourmashErrorCode sourmash_err_get_last_code(void);
SourmashStr sourmash_err_get_last_message(void);
SourmashStr sourmash_err_get_backtrace(void);
void sourmash_str_free(SourmashStr *s);
SourmashStr sourmash_str_from_cstr(const char *s);

/* ---- include/sourmash.h:133 (ffi/mod.rs:22-31; lib.rs:57-59): MurmurHash3_x64_128 h1 ---- */
uint64_t hash_murmur(const char *kmer, uint64_t seed);
/* include/sourmash.h:416-418,467 -- residue helpers of the protein / dayhoff / hp sketches */
char sourmash_aa_to_dayhoff(char aa);
char sourmash_aa_to_hp(char aa);
char sourmash_translate_codon(const char *codon);

/* ---- compute parameters: include/sourmash.h:89-131 (ffi/cmd/compute.rs:1-170) ---- */
SourmashComputeParameters *computeparams_new(void);
void computeparams_free(SourmashComputeParameters *ptr);
bool computeparams_dayhoff(const SourmashComputeParameters *ptr);
bool computeparams_dna(const SourmashComputeParameters *ptr);
bool computeparams_hp(const SourmashComputeParameters *ptr);
bool computeparams_protein(const SourmashComputeParameters *ptr);
bool computeparams_track_abundance(const SourmashComputeParameters *ptr);
const uint32_t *computeparams_ksizes(const SourmashComputeParameters *ptr, uintptr_t *size);
void computeparams_ksizes_free(uint32_t *ptr, uintptr_t insize);
uint32_t computeparams_num_hashes(const SourmashComputeParameters *ptr);
uint64_t computeparams_scaled(const SourmashComputeParameters *ptr);
uint64_t computeparams_seed(const SourmashComputeParameters *ptr);
void computeparams_set_dayhoff(SourmashComputeParameters *ptr, bool v);
void computeparams_set_dna(SourmashComputeParameters *ptr, bool v);
void computeparams_set_hp(SourmashComputeParameters *ptr, bool v);
void computeparams_set_protein(SourmashComputeParameters *ptr, bool v);
void computeparams_set_track_abundance(SourmashComputeParameters *ptr, bool v);
void computeparams_set_ksizes(SourmashComputeParameters *ptr, const uint32_t *ksizes_ptr, uintptr_t insize);
void computeparams_set_num_hashes(SourmashComputeParameters *ptr, uint32_t num);
void computeparams_set_scaled(SourmashComputeParameters *ptr, uint64_t scaled);
void computeparams_set_seed(SourmashComputeParameters *ptr, uint64_t new_seed);

/* ---- sketch object: include/sourmash.h:169-273 (ffi/minhash.rs:1-483) ---- */
SourmashKmerMinHash *kmerminhash_new(uint64_t scaled, uint32_t k, HashFunctions hash_function, uint64_t seed,
                                     bool track_abundance, uint32_t n);
void kmerminhash_free(SourmashKmerMinHash *ptr);
void kmerminhash_slice_free(uint64_t *ptr, uintptr_t insize);
/* HOT: sequence -> k-mers -> canonical -> murmur -> keep (signature.rs:38-58,246-306). NUL-terminated. */
void kmerminhash_add_sequence(SourmashKmerMinHash *ptr, const char *sequence, bool force);
const uint64_t *kmerminhash_seq_to_hashes(SourmashKmerMinHash *ptr, const char *sequence, uintptr_t insize,
                                          bool force, bool bad_kmers_as_zeroes, bool is_protein, uintptr_t *size);
void kmerminhash_add_hash(SourmashKmerMinHash *ptr, uint64_t h);
void kmerminhash_add_hash_with_abundance(SourmashKmerMinHash *ptr, uint64_t h, uint64_t abundance);
void kmerminhash_add_many(SourmashKmerMinHash *ptr, const uint64_t *hashes_ptr, uintptr_t insize);
void kmerminhash_add_from(SourmashKmerMinHash *ptr, const SourmashKmerMinHash *other);
void kmerminhash_add_word(SourmashKmerMinHash *ptr, const char *word);
void kmerminhash_add_protein(SourmashKmerMinHash *ptr, const char *sequence);   /* out of scope: raises */
void kmerminhash_remove_hash(SourmashKmerMinHash *ptr, uint64_t h);
void kmerminhash_remove_many(SourmashKmerMinHash *ptr, const uint64_t *hashes_ptr, uintptr_t insize);
void kmerminhash_remove_from(SourmashKmerMinHash *ptr, const SourmashKmerMinHash *other);
void kmerminhash_clear(SourmashKmerMinHash *ptr);
const uint64_t *kmerminhash_get_mins(const SourmashKmerMinHash *ptr, uintptr_t *size);
uintptr_t kmerminhash_get_mins_size(const SourmashKmerMinHash *ptr);
const uint64_t *kmerminhash_get_abunds(SourmashKmerMinHash *ptr, uintptr_t *size);
void kmerminhash_set_abundances(SourmashKmerMinHash *ptr, const uint64_t *hashes_ptr, const uint64_t *abunds_ptr,
                                uintptr_t insize, bool clear);
SourmashStr kmerminhash_md5sum(const SourmashKmerMinHash *ptr);
void kmerminhash_merge(SourmashKmerMinHash *ptr, const SourmashKmerMinHash *other);
bool kmerminhash_is_compatible(const SourmashKmerMinHash *ptr, const SourmashKmerMinHash *other);
/* HOT: sorted-u64 merge intersections (minhash.rs:539-631,635-702,915-953,1721-1807) */
uint64_t kmerminhash_count_common(const SourmashKmerMinHash *ptr, const SourmashKmerMinHash *other, bool downsample);
SourmashKmerMinHash *kmerminhash_intersection(const SourmashKmerMinHash *ptr, const SourmashKmerMinHash *other);
uint64_t kmerminhash_intersection_union_size(const SourmashKmerMinHash *ptr, const SourmashKmerMinHash *other,
                                             uint64_t *union_size);
double kmerminhash_jaccard(const SourmashKmerMinHash *ptr, const SourmashKmerMinHash *other);
double kmerminhash_similarity(const SourmashKmerMinHash *ptr, const SourmashKmerMinHash *other,
                              bool ignore_abundance, bool downsample);
double kmerminhash_angular_similarity(const SourmashKmerMinHash *ptr, const SourmashKmerMinHash *other);
uint32_t kmerminhash_num(const SourmashKmerMinHash *ptr);
uint32_t kmerminhash_ksize(const SourmashKmerMinHash *ptr);
uint64_t kmerminhash_seed(const SourmashKmerMinHash *ptr);
uint64_t kmerminhash_max_hash(const SourmashKmerMinHash *ptr);
HashFunctions kmerminhash_hash_function(const SourmashKmerMinHash *ptr);
void kmerminhash_hash_function_set(SourmashKmerMinHash *ptr, HashFunctions hash_function);
bool kmerminhash_is_protein(const SourmashKmerMinHash *ptr);
bool kmerminhash_dayhoff(const SourmashKmerMinHash *ptr);
bool kmerminhash_hp(const SourmashKmerMinHash *ptr);
bool kmerminhash_track_abundance(const SourmashKmerMinHash *ptr);
void kmerminhash_enable_abundance(SourmashKmerMinHash *ptr);
void kmerminhash_disable_abundance(SourmashKmerMinHash *ptr);

/* ---- signature container: include/sourmash.h:364-414 (ffi/signature.rs:1-344) ---- */
SourmashSignature *signature_new(void);
void signature_free(SourmashSignature *ptr);
SourmashSignature *signature_from_params(const SourmashComputeParameters *ptr);
uintptr_t signature_len(const SourmashSignature *ptr);
/* HOT: fans the record out over every sketch of the signature (signature.rs:661-677) */
void signature_add_sequence(SourmashSignature *ptr, const char *sequence, bool force);
void signature_add_protein(SourmashSignature *ptr, const char *sequence);       /* out of scope: raises */
void signature_set_name(SourmashSignature *ptr, const char *name);
void signature_set_filename(SourmashSignature *ptr, const char *name);
SourmashStr signature_get_name(const SourmashSignature *ptr);
SourmashStr signature_get_filename(const SourmashSignature *ptr);
SourmashStr signature_get_license(const SourmashSignature *ptr);
SourmashKmerMinHash *signature_first_mh(const SourmashSignature *ptr);
SourmashKmerMinHash **signature_get_mhs(const SourmashSignature *ptr, uintptr_t *size);
void signature_set_mh(SourmashSignature *ptr, const SourmashKmerMinHash *other);
void signature_push_mh(SourmashSignature *ptr, const SourmashKmerMinHash *other);
bool signature_eq(const SourmashSignature *ptr, const SourmashSignature *other);
SourmashStr signature_save_json(const SourmashSignature *ptr);
SourmashSignature **signatures_load_buffer(const char *ptr, uintptr_t insize, bool _ignore_md5sum, uintptr_t ksize,
                                           const char *select_moltype, uintptr_t *size);
SourmashSignature **signatures_load_path(const char *ptr, bool _ignore_md5sum, uintptr_t ksize,
                                         const char *select_moltype, uintptr_t *size);
const uint8_t *signatures_save_buffer(const SourmashSignature *const *ptr, uintptr_t size, uint8_t compression,
                                      uintptr_t *osize);
/* generic byte-buffer free (src/sourmash/signature.py:514 frees signatures_save_buffer output with it) */
void nodegraph_buffer_free(uint8_t *ptr, uintptr_t insize);

/* HyperLogLog (include/sourmash.h, src/core/src/ffi/hyperloglog.rs).  hll_to_buffer's buffer is freed with nodegraph_buffer_free. */
void hll_add_hash(SourmashHyperLogLog *ptr, uint64_t hash);
void hll_add_sequence(SourmashHyperLogLog *ptr, const char *sequence, uintptr_t insize, bool force);
uintptr_t hll_cardinality(const SourmashHyperLogLog *ptr);
double hll_containment(const SourmashHyperLogLog *ptr, const SourmashHyperLogLog *optr);
void hll_free(SourmashHyperLogLog *ptr);
SourmashHyperLogLog *hll_from_buffer(const char *ptr, uintptr_t insize);
SourmashHyperLogLog *hll_from_path(const char *filename);
uintptr_t hll_intersection_size(const SourmashHyperLogLog *ptr, const SourmashHyperLogLog *optr);
uintptr_t hll_ksize(const SourmashHyperLogLog *ptr);
uintptr_t hll_matches(const SourmashHyperLogLog *ptr, const SourmashKmerMinHash *mh_ptr);
void hll_merge(SourmashHyperLogLog *ptr, const SourmashHyperLogLog *optr);
SourmashHyperLogLog *hll_new(void);
void hll_save(const SourmashHyperLogLog *ptr, const char *filename);
double hll_similarity(const SourmashHyperLogLog *ptr, const SourmashHyperLogLog *optr);
const uint8_t *hll_to_buffer(const SourmashHyperLogLog *ptr, uintptr_t *size);
void hll_update_mh(SourmashHyperLogLog *ptr, const SourmashKmerMinHash *optr);
SourmashHyperLogLog *hll_with_error_rate(double error_rate, uintptr_t ksize);

/* Nodegraph, khmer's Bloom filter (include/sourmash.h, src/core/src/ffi/nodegraph.rs).  nodegraph_to_buffer's buffer is freed
 * with nodegraph_buffer_free, nodegraph_hashsizes' array with kmerminhash_slice_free. */
bool nodegraph_count(SourmashNodegraph *ptr, uint64_t h);
bool nodegraph_count_kmer(SourmashNodegraph *ptr, const char *kmer);
double nodegraph_expected_collisions(const SourmashNodegraph *ptr);
void nodegraph_free(SourmashNodegraph *ptr);
SourmashNodegraph *nodegraph_from_buffer(const char *ptr, uintptr_t insize);
SourmashNodegraph *nodegraph_from_path(const char *filename);
uintptr_t nodegraph_get(const SourmashNodegraph *ptr, uint64_t h);
uintptr_t nodegraph_get_kmer(const SourmashNodegraph *ptr, const char *kmer);
const uint64_t *nodegraph_hashsizes(const SourmashNodegraph *ptr, uintptr_t *size);
uintptr_t nodegraph_ksize(const SourmashNodegraph *ptr);
uintptr_t nodegraph_matches(const SourmashNodegraph *ptr, const SourmashKmerMinHash *mh_ptr);
SourmashNodegraph *nodegraph_new(void);
uintptr_t nodegraph_noccupied(const SourmashNodegraph *ptr);
uintptr_t nodegraph_ntables(const SourmashNodegraph *ptr);
void nodegraph_save(const SourmashNodegraph *ptr, const char *filename);
const uint8_t *nodegraph_to_buffer(const SourmashNodegraph *ptr, uint8_t compression, uintptr_t *size);
void nodegraph_update(SourmashNodegraph *ptr, const SourmashNodegraph *optr);
void nodegraph_update_mh(SourmashNodegraph *ptr, const SourmashKmerMinHash *optr);
SourmashNodegraph *nodegraph_with_tables(uintptr_t ksize, uintptr_t starting_size, uintptr_t n_tables);

/* ============================ PART 2: batch extensions ============================ */
/* Same conventions (TLS error, zero on failure).  "d_" pointers are device
 * pointers valid on the current HIP device; `stream` is a hipStream_t passed as
 * void* (NULL = the null stream).  None of the *_raw functions allocates or
 * synchronises unless stated. */

/* number of visible HIP devices (0 when none / no driver); never fails */
int32_t smgpu_device_count(void);
/* 1 if the k-mer / intersection kernels can run in this process */
bool smgpu_available(void);

/* Collapses the per-record loop of src/sourmash/command_sketch.py:746-768 +
 * src/core/src/signature.rs:38-58: sketch a whole buffer (records separated by any
 * byte outside ACGTacgt, e.g. '\n'; no NUL needed) into `ptr`. */
void smgpu_minhash_add_buffer(SourmashKmerMinHash *ptr, const char *buf, uintptr_t len, bool force);

/* The whole `sourmash sketch dna <file>` inner loop (command_sketch.py:697,746-768) in one call: a native
 * FASTA / FASTQ (plain or gzip) reader strips headers and line breaks, streams 64 MiB chunks through
 * pinned staging buffers to the GPU, and every sketch of the signature (all ksizes) is filled in the same
 * pass.  force=True semantics (bytes outside ACGTacgt drop the k-mers covering them).  Returns the
 * number of sequence bytes read; *n_records = number of records. */
/* Per-record sketching without a launch per record.  kmerminhash_add_sequence / signature_add_sequence (the reference's
 * loop: src/sourmash/command_sketch.py:746-768, src/core/src/signature.rs:38-58) validate the record, queue it in the
 * sketch and return; the queue goes through the sketch kernel in one launch when it reaches 32 MiB or when any accessor
 * looks at the sketch.  force = false still raises InvalidDNA from the offending call, after the k-mers in front of the
 * first bad one were queued (signature.rs:48-54).  smgpu_minhash_add_sequence_rc is add_sequence with the error code as
 * the return value (len bytes, a NUL ends the record early like the C string of the reference's entry point);
 * smgpu_minhash_flush settles the queue now; smgpu_minhash_pending_bytes tells how much is queued. */
uint32_t smgpu_minhash_add_sequence_rc(SourmashKmerMinHash *ptr, const char *sequence, uintptr_t len, bool force);
void smgpu_minhash_flush(SourmashKmerMinHash *ptr);
uint64_t smgpu_minhash_pending_bytes(const SourmashKmerMinHash *ptr);
uint64_t smgpu_signature_add_file(SourmashSignature *ptr, const char *path, uint64_t *n_records);
/* `sourmash sketch dna` over many files at once: n_threads workers (0 = min(16, host cores)), each with its own
 * stream, pinned ring and device buffers, one signature per file in input order (every ksize of `params` in it).
 * Returns an array of n signature handles (free each with signature_free and the array with nodegraph_buffer_free,
 * like signatures_load_buffer's). */
SourmashSignature **smgpu_sketch_files(const char *const *paths, uintptr_t n, const SourmashComputeParameters *params,
                                       uint32_t n_threads, uint64_t *total_bases);
uint64_t smgpu_minhash_add_file(SourmashKmerMinHash *ptr, const char *path, uint64_t *n_records);
/* The inflater behind the .gz ingest by itself (csrc/gunzip.hpp: the members' compressed bytes go to HBM, every deflate block of
 * a member is decoded at once, CRC-32 and length are checked against the trailer; what niffler / screed do on one host thread,
 * src/core/benches/compute.rs:35-38, src/sourmash/command_sketch.py:697).  n single-member gzip files, inflated in ONE batch;
 * their bytes come back to out[0, capacity) one behind the other, lens[i] = bytes of file i or UINT64_MAX when the device refused
 * it (several members, damaged, not gzip): such a file is the host inflater's.  stats (NULL or 16 doubles): [0] survivors of the
 * cheap header test, [1] candidates decoded, [2] runs on the chains, [3..8] milliseconds: scan, pass 1, link, pass 2, tails +
 * resolve + CRC, everything on the device; [9] H2D copy + file reads.  Returns the bytes written. */
uint64_t smgpu_gunzip_files(const char *const *paths, uintptr_t n, uint8_t *out, uint64_t capacity, uint64_t *lens, double *stats);
/* out[0]: signature documents smgpu_sketchset_load has parsed with the device doing inflate and number parsing (csrc/sigload.hpp)
 * since the library was loaded, out[1]: documents its host parser took (SMG_SIGLOAD_DEVICE=0 sends every document there). */
void smgpu_sigload_counters(uint64_t *out);
/* out[0]: gzip files the ingest inflated on the device since the library was loaded, out[1]: files it handed to the host inflater
 * after the device refused them. */
void smgpu_gunzip_counters(uint64_t *out);

/* Scratch size needed by smgpu_sketch_dna_raw for an output capacity: the unordered kept hashes, and the larger of the two
 * sorts' scratch (the uniform sort's regions, csrc/uniform_sort.hip; the general sort reuses them when it takes over). */
uint64_t smgpu_sketch_workspace_bytes(uint64_t out_capacity);
/* Device-resident sketching: d_seq[0,len) ASCII (any alignment) -> sorted unique
 * kept hashes (1 <= h <= max_hash; max_hash 0 = keep all) in d_out[0, n).
 * d_result (device, 2 x u64): [0] kept k-mer occurrences, [1] unique hashes n.
 * The kept count stays on the device: the sort for uniformly spread keys (csrc/uniform_sort.hip) reads it there, and the
 * call synchronises the stream once, behind the sort.  Kept hashes that do not spread like hashes (one k-mer repeated, a
 * short period) go through the general radix sort behind that, with a second synchronisation; the result is the same.
 * Returns n, or UINT64_MAX with an error set; if kept > out_capacity the error says so, d_result[0] holds the count, and
 * the caller retries with a larger buffer. */
uint64_t smgpu_sketch_dna_raw(const uint8_t *d_seq, uint64_t len, uint32_t ksize, uint64_t seed, uint64_t max_hash,
                              uint64_t *d_out, uint64_t out_capacity, uint64_t *d_result, void *d_workspace,
                              uint64_t workspace_bytes, void *stream);
/* ---- one sketch per record (csrc/sketch_records.hip; `sourmash sketch dna --singleton`, src/sourmash/command_sketch.py:712-739) ----
 * Records are described by d_starts[0 .. n_records], an ascending device array: record r is the bytes
 * [d_starts[r], d_starts[r + 1]) of d_seq, d_starts[n_records] <= len; records may touch without a separator byte.  A k-mer
 * counts for the record it lies in entirely; k-mers that span two records, or lie outside all of them, are dropped.
 * Scratch size of smgpu_sketch_records_raw for a capacity of kept (hash, position) pairs. */
uint64_t smgpu_sketch_records_workspace_bytes(uint64_t pair_capacity, uint64_t n_records);
/* d_seq[0,len) ASCII (any alignment) -> the CSR of its records: row r = the sorted distinct hashes (1 <= h <= max_hash;
 * max_hash 0 = keep all) of the canonical k-mers inside record r, in d_hashes[d_offsets[r], d_offsets[r + 1]); d_abunds
 * (NULL = flat) their multiplicities.  ksize 1 .. 88.  capacity: entries of d_hashes / d_abunds and kept pairs the workspace
 * holds; d_offsets: n_records + 1 entries.  d_result (device, 4 x u64): [0] kept k-mer occurrences, [1] entries, [3] non-zero
 * when the starts are refused.  Synchronises the stream twice (the sort needs the kept count).  Returns the entries, or
 * UINT64_MAX with an error set: starts not ascending or ending behind len; or more pairs kept than capacity -- the error says
 * so and names the count (also in d_result[0]), and the caller retries with a larger buffer. */
uint64_t smgpu_sketch_records_raw(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, uint64_t n_records,
                                  uint32_t ksize, uint64_t seed, uint64_t max_hash, uint64_t *d_hashes, uint64_t *d_abunds,
                                  uint64_t capacity, uint64_t *d_offsets, uint64_t *d_result, void *d_workspace,
                                  uint64_t workspace_bytes, void *stream);
/* Only its k-mer kernel (no assign, no sort): every kept hash appended unordered to d_hashes and the position of its k-mer's
 * first byte in d_seq to d_positions; the count is added to *d_count (device u64, caller zeroes).  Fully asynchronous. */
void smgpu_sketch_records_kernel_raw(const uint8_t *d_seq, uint64_t len, uint32_t ksize, uint64_t seed, uint64_t max_hash,
                                     uint64_t *d_hashes, uint64_t *d_positions, uint64_t capacity, uint64_t *d_count, void *stream);
/* The FASTA / FASTQ parser by itself (csrc/fastx.hip), for tests and for callers that hold file bytes in HBM: d_raw[0,len) is the
 * next piece of a FASTA (fastq == 0) or four-line FASTQ (fastq != 0) file.  The sequence bytes and one separator byte per record --
 * the first byte of its header line -- go to d_out in order (room for len bytes).  d_result (device, 2 x u64): [0] = bytes kept
 * of THIS piece, [1] += header lines of this piece (the caller zeroes it in front of the first piece).  d_carry (device, 4 bytes,
 * the caller's for the whole file): {1, 1, 0, 0} in front of a FASTA file's first piece, {3, 1, 0, 0} of a FASTQ file's; the
 * state behind the piece ({line state, ended on LF}) is left in d_carry[2,4) and, unless last_piece, copied to d_carry[0,2) for
 * the next piece.  An empty piece sets d_result[0] = 0 and touches nothing else.  d_record_starts (NULL: not wanted): entry j =
 * the offset in d_out just behind the j-th kept header byte of this piece, for j < record_capacity.  d_raw must be 16-byte
 * aligned: any other pointer is refused with an error before anything is launched.  Scratch is the library's.  Asynchronous. */
void smgpu_fastx_compact_raw(const uint8_t *d_raw, uint64_t len, int32_t fastq, uint8_t *d_carry, uint8_t *d_out, uint64_t *d_result,
                             uint64_t *d_record_starts, uint64_t record_capacity, int32_t last_piece, void *stream);
/* The signature JSON array parser by itself (csrc/sigjson.hip), for tests: d_text[0, text_len) is a block of JSON text in HBM,
 * docs (host) n_docs pairs {off, len} of documents inside it.  The span scan runs on all documents, the `mins` arrays of every
 * document with nothing odd become the jobs of ONE parse launch -- planned by the function the collection loader plans with
 * (csrc/sigjson_api.hpp: sj_plan) -- and their values go to d_values (device, value_capacity entries) side by side in job order.
 * To the host: spans_out, n_docs x 8 records {u64 begin, end; u32 n_values, kind (0 mins, 1 abundances), flags (1 odd), pad}, of
 * which the first doc_flags & 0xff are written; flags_out, n_docs x u32 (bit 31: the document is odd); parsed_out, one record
 * {u32 n_kept, flags (1: not plain ascending numbers)} per job, parsed_capacity records; counts_out[0] = jobs, [1] = values.
 * The parse kernel loads whole 16-byte lines: smgpu_sigjson_text_pad() bytes behind d_text[text_len) must be readable (the
 * device inflater's output has them).  Refused with an error before anything is launched: a null pointer, a document that
 * reaches outside the text.  An error after the span scan: more jobs or values than the capacities.  Synchronises the stream. */
uint64_t smgpu_sigjson_text_pad(void);
void smgpu_sigjson_parse_raw(const uint8_t *d_text, uint64_t text_len, const uint64_t *docs, uint32_t n_docs, uint64_t keep_max,
                             void *spans_out, uint32_t *flags_out, uint64_t *d_values, uint64_t value_capacity, void *parsed_out,
                             uint64_t parsed_capacity, uint64_t *counts_out, void *stream);
/* Every record of a FASTA / FASTQ file (plain or gzip, at most 2 GiB of text, resident as a whole) as a signature of its own,
 * holding every sketch of `params` (DNA, scaled, ksizes 1 .. 88): the device parses the file and reports where the records
 * start, one kernel pass per sketch covers all records.  Names are the header lines behind '>' / '@'.  *n = records.  Returns
 * an array of *n signature handles (ownership as for smgpu_sketch_files). */
SourmashSignature **smgpu_sketch_file_singleton(const char *path, const SourmashComputeParameters *params, uintptr_t *n);
/* The same for files sketched with protein / dayhoff / hp parameters (`sourmash sketch protein --singleton`, input_is_protein != 0:
 * records are residues; `sourmash sketch translate --singleton`, input_is_protein == 0: records are DNA, translated in six frames):
 * scaled, stored ksizes of 3 x (1 .. 79 residues).  A template that mixes molecule types runs one pass per sketch over the same
 * parsed buffer; a DNA sketch in it (translated input only) takes the pass of smgpu_sketch_file_singleton. */
SourmashSignature **smgpu_sketch_file_singleton_residues(const char *path, const SourmashComputeParameters *params,
                                                         int32_t input_is_protein, uintptr_t *n);
/* ---- one protein / dayhoff / hp sketch per record (csrc/protein_records.hip; src/core/src/signature.rs:257-261, 307-393) ----
 * Records with explicit ends: record r is the bytes [d_starts[r], d_ends[r]) of d_seq with d_starts[r] <= d_ends[r] <=
 * d_starts[r + 1]; d_ends NULL: d_ends[r] = d_starts[r + 1], records touch.  The bytes between d_ends[r] and d_starts[r + 1]
 * -- the byte a file parser leaves between two records -- belong to no record.  translate == 0: the records are residues, a
 * window of ksize residues counts for the record it lies in entirely.  translate != 0: the records are DNA, each translated in
 * six frames by itself (frames 0..2 forward and on the record's reverse complement, a trailing partial codon dropped, no
 * validity test; a record below 3 x ksize bases gives nothing).
 * Scratch size of smgpu_sketch_residue_records_raw for a capacity of kept (hash, position) pairs and a buffer of len bytes. */
uint64_t smgpu_sketch_residue_records_workspace_bytes(uint64_t pair_capacity, uint64_t n_records, uint64_t len, int32_t translate);
/* The contract of smgpu_sketch_records_raw -- the same d_result words, the same errors for refused starts, the same capacity
 * error -- for windows of ksize residues (1 .. 79) hashed as hash_function says (2 protein, 3 dayhoff, 4 hp).  One more error:
 * a d_ends[r] outside [d_starts[r], d_starts[r + 1]] (d_result[3] & 4).  d_workspace must be 8-byte aligned.  Synchronises the
 * stream three times (the records are checked before anything reads what they say). */
uint64_t smgpu_sketch_residue_records_raw(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, const uint64_t *d_ends,
                                          uint64_t n_records, uint32_t ksize, uint32_t hash_function, int32_t translate,
                                          uint64_t seed, uint64_t max_hash, uint64_t *d_hashes, uint64_t *d_abunds,
                                          uint64_t capacity, uint64_t *d_offsets, uint64_t *d_result, void *d_workspace,
                                          uint64_t workspace_bytes, void *stream);
/* Only its window kernel, for measurements: d_aa[0,n) is a residue buffer (8-byte aligned, readable in whole 8-byte words), every
 * kept hash of a window of ksize residues is appended unordered to d_hashes and the window's start to d_positions; the count is
 * added to *d_count (device u64, caller zeroes).  d_n (device u64, NULL: n) is the buffer's size where only the device knows it;
 * with it 0xFF bytes separate, as in the translated buffer.  d_positions NULL: the hash-only kernel of the record-by-record route
 * (0xFF bytes separate) on the same buffer.  Fully asynchronous. */
void smgpu_residue_records_kernel_raw(const uint8_t *d_aa, uint64_t n, const uint64_t *d_n, uint32_t ksize, uint64_t seed,
                                      uint64_t max_hash, uint64_t *d_hashes, uint64_t *d_positions, uint64_t capacity,
                                      uint64_t *d_count, void *stream);
/* Only the k-mer kernel (no sort): appends kept hashes unordered to d_out, adds the
 * count to *d_count (device u64, caller zeroes).  Fully asynchronous. */
void smgpu_sketch_dna_kernel_raw(const uint8_t *d_seq, uint64_t len, uint32_t ksize, uint64_t seed, uint64_t max_hash,
                                 uint64_t *d_out, uint64_t out_capacity, uint64_t *d_count, void *stream);
/* The same with a workgroup count: grid == 0 is the library's own choice, otherwise exactly `grid` workgroups (at most
 * 1048576), which take the tiles behind their first from the launch's ticket counter wherever there are more tiles than
 * workgroups.  For tests: many tiles per workgroup on a small input.  ksize <= 88; longer k-mers ignore `grid`. */
void smgpu_sketch_dna_kernel_grid_raw(const uint8_t *d_seq, uint64_t len, uint32_t ksize, uint64_t seed, uint64_t max_hash,
                                      uint64_t *d_out, uint64_t out_capacity, uint64_t *d_count, uint32_t grid, void *stream);
/* Union of hash vectors on the device (the `merge` of flat scaled sketches, src/core/src/sketch/minhash.rs:432-516, for
 * vectors already in HBM -- e.g. the all-gathered per-rank sketches): d_keys[0, n) in any order, duplicates allowed ->
 * the sorted distinct values in d_out[0, m) (capacity n); *d_n_out (device u64) = m.  d_keys is used as scratch.  The
 * workspace is smgpu_sketch_workspace_bytes(n) bytes.  Radix sort + run-length encode (csrc/device_sort.hip).
 * Synchronises the stream once.  Returns m, or UINT64_MAX with an error set. */
uint64_t smgpu_sort_unique_raw(uint64_t *d_keys, uint64_t n, uint64_t *d_out, uint64_t *d_n_out, void *d_workspace,
                               uint64_t workspace_bytes, void *stream);
/* The same for keys that are uniform on [0, thr] (hashes kept under a sketch's max_hash), with the number of keys on the device
 * (csrc/uniform_sort.hip): d_keys[0, min(*d_n, n_max)) -> the sorted distinct values in d_out[0, m) (capacity n_max), their
 * multiplicities in d_counts (NULL: not wanted); *d_result (device u64) = m.  Up to 16,384 keys one workgroup sorts whatever
 * they are; above, keys that do not spread uniformly are noticed on the device and go through the general radix sort, with the
 * same result.  The workspace is smgpu_sort_unique_uniform_workspace_bytes(n_max, counts wanted) bytes.  Synchronises the stream
 * once (twice when the general sort takes over).  Returns m, or UINT64_MAX with an error set. */
uint64_t smgpu_sort_unique_uniform_workspace_bytes(uint64_t n_max, int32_t counts);
uint64_t smgpu_sort_unique_uniform_raw(uint64_t *d_keys, const uint64_t *d_n, uint64_t n_max, uint64_t thr, uint64_t *d_out,
                                       uint64_t *d_counts, uint64_t *d_result, void *d_workspace, uint64_t workspace_bytes,
                                       void *stream);
/* out[0]: calls of smgpu_sketch_dna_raw / smgpu_sort_unique_uniform_raw since the library was loaded whose result the bucket
 * form of the uniform sort gave, out[1]: its one-workgroup form, out[2]: calls that fell back to the general sort. */
void smgpu_sort_counters(uint64_t *out);
/* The kernels of protein / dayhoff / hp sketches on device-resident input (src/core/src/signature.rs:307-393,
 * src/core/src/encodings.rs:103-368): the residues of a protein sequence -- or, translate = true, the six-frame translation of
 * DNA -- go to d_aa (capacity aa_capacity bytes: the residue count rounded up to 8 -- the window kernel reads whole aligned
 * 8-byte words; translated DNA needs 2 * len + 6 residues), every window of k_aa residues is hashed and
 * the hashes 1 <= h <= max_hash are appended unordered to d_out, their count added to *d_count (device u64, caller zeroes).
 * -> residues written to d_aa (DNA of fewer than three bases: the six separators, and no window is hashed).  Fully asynchronous.
 * hash_function: 2 protein, 3 dayhoff, 4 hp. */
uint64_t smgpu_sketch_residues_kernels_raw(const uint8_t *d_seq, uint64_t len, uint32_t k_aa, uint32_t hash_function, uint64_t seed,
                                           uint64_t max_hash, bool translate, uint8_t *d_aa, uint64_t aa_capacity, uint64_t *d_out,
                                           uint64_t out_capacity, uint64_t *d_count, void *stream);
/* Synthetic random DNA written straight into HBM (BASELINE config C2 generator). */
void smgpu_synth_dna_raw(uint8_t *d_out, uint64_t start, uint64_t n, uint64_t seed, uint64_t record_len, void *stream);

/* Collapses compare_all_pairs (src/sourmash/compare.py:14-64,328-358): CSR of n
 * sorted sketches on device -> u32 common[(row_hi-row_lo)][n] and/or f64
 * jaccard[(row_hi-row_lo)][n] for rows [row_lo,row_hi).  Either output may be NULL
 * (d_common is required as scratch if d_jaccard is given).  Asynchronous. */
void smgpu_compare_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, uint32_t n, uint32_t row_lo,
                       uint32_t row_hi, uint32_t *d_common, double *d_jaccard, void *stream);
/* Multi-GPU form of the same kernel (BASELINE config C4: row-block shard per GPU): this launch owns
 * the 16-row tiles rb_first, rb_first + rb_stride, ... (rb_count tiles) of the n x n problem and
 * computes their tiles on/above the diagonal into d_common[rb_count*16][n] (zero-initialised by the
 * caller).  After one all-gather of the shards, smgpu_symmetrize_raw mirrors the upper triangle of the
 * full matrix and smgpu_jaccard_raw converts counts (rows [row_lo,row_hi) of a full matrix slice that
 * starts at row_lo) to f64 Jaccard. */
void smgpu_compare_blocks_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, uint32_t n, uint32_t rb_first,
                              uint32_t rb_stride, uint32_t rb_count, uint32_t *d_common, void *stream);
void smgpu_symmetrize_raw(uint32_t *d_common, uint32_t n, void *stream);
void smgpu_jaccard_raw(const uint32_t *d_common, const uint64_t *d_offsets, uint32_t n, uint32_t row_lo,
                       uint32_t row_hi, double *d_jaccard, void *stream);
/* Indexed paths of the same comparison.  smgpu_bitindex_new groups every (hash, row) of the collection by hash (hash-space
 * buckets with LDS tables, csrc/dictindex.hip; a radix sort when a bucket holds more than 1,024 distinct hashes;
 * synchronises the stream once) and splits the hashes by how many sketches hold them: frequent ones become bit columns
 * (|A ∩ B| = popcount(A & B) over bit rows), rare ones inverted lists whose pairs are incremented directly.  A
 * collection drawn from one pool ends up all bit rows, a collection of unrelated genomes all inverted lists.
 * Returns NULL -- with no error set -- when the cost model prefers the merge kernel (smgpu_compare_*_raw).
 * smgpu_bitindex_compare_raw fills d_common[rb_count*16][n] for the owned 16-row tiles, ALL columns. */
typedef struct SmgpuBitIndex SmgpuBitIndex;
SmgpuBitIndex *smgpu_bitindex_new(const uint64_t *d_hashes, const uint64_t *d_offsets, uint32_t n, void *stream);
/* same with the knobs exposed: total_hashes = d_offsets[n] if the caller knows it (0: read back, one more
 * synchronisation); threshold > 0 forces the frequent/rare split instead of the cost model's (and then never returns NULL
 * unless the bit rows would exceed the memory cap); one_shot: the index will serve a single compare, so its own build
 * time counts against it. */
SmgpuBitIndex *smgpu_bitindex_new_ex(const uint64_t *d_hashes, const uint64_t *d_offsets, uint32_t n, uint64_t total_hashes,
                                     uint32_t threshold, bool one_shot, void *stream);
void smgpu_bitindex_free(SmgpuBitIndex *ptr);
uint64_t smgpu_bitindex_universe(const SmgpuBitIndex *ptr);
uint32_t smgpu_bitindex_builder(const SmgpuBitIndex *ptr);   /* which builder made it: 1 sort-free dictionary passes, 2 radix sort (diagnostic) */
/* how the index splits the collection: hashes held by more than `threshold` sketches are bit columns, the others
 * are inverted lists costing `rare_pairs` matrix increments per compare */
void smgpu_bitindex_stats(const SmgpuBitIndex *ptr, uint64_t *frequent_hashes, uint64_t *rare_pairs, uint32_t *threshold);
void smgpu_bitindex_compare_raw(const SmgpuBitIndex *ptr, uint32_t rb_first, uint32_t rb_stride, uint32_t rb_count,
                                uint32_t *d_common, void *stream);
/* The same for callers that mirror the triangle afterwards (smgpu_symmetrize_raw, as the all-pairs drivers do): only the
 * entries on or above the diagonal of the owned rows are computed (the counterpart of smgpu_compare_blocks_raw); what lies
 * below is left as it was.  Half the tiles of a world-size-1 launch. */
void smgpu_bitindex_compare_upper_raw(const SmgpuBitIndex *ptr, uint32_t rb_first, uint32_t rb_stride, uint32_t rb_count,
                                      uint32_t *d_common, void *stream);
/* Host float helper for the containment / ANI matrices of compare (src/sourmash/compare.py:67-187): out[i] =
 * pow(x[i], y[ny == 1 ? 0 : i]) with the host libm, i.e. the bits of the reference's per-pair Python `**`
 * (src/sourmash/minhash.py:832-834, src/sourmash/distance_utils.py:283).  n_threads = 0: every host core. */
void smgpu_host_pow_f64(const double *x, const double *y, uintptr_t ny, double *out, uintptr_t n, uint32_t n_threads);
/* Host helper of add_sequence(force = false): index of the first byte of seq[0, len) outside ACGTacgt (what makes a k-mer
 * invalid: src/core/src/encodings.rs:370-377 after the upper-casing of src/core/src/signature.rs:214), or UINTPTR_MAX
 * when there is none.  No device involved; exported so that the CPU test suite can pin the vectorised scan. */
uintptr_t smgpu_first_invalid_dna_byte(const char *seq, uintptr_t len);
/* n sketch handles -> n x n matrices on the host (either may be NULL): what src/sourmash/compare.py:326-358 walks pair by pair
 * through kmerminhash_similarity / kmerminhash_count_common (src/core/src/ffi/minhash.rs:409-457).  The sketches are packed into
 * pinned chunks by worker threads and travel as one H2D copy per chunk; the matrices come back through the same ring. */
void smgpu_compare_all_pairs(const SourmashKmerMinHash *const *mhs, uintptr_t n, uint32_t *common_out,
                             double *jaccard_out);
/* The same for a list with SEVERAL scaled values and downsample = true (compare.py:14-64; src/core/src/sketch/minhash.rs:682-702):
 * common_out[i][j] = |A ∩ B| with both sketches downsampled to the pair's coarser scaled -- a prefix of the finer row
 * (minhash.rs:777-798) -- and the row's own size on the diagonal.  class_of[i] = index of sketch i's scaled value in the ascending
 * list of the list's distinct values, class_max_hash[c] = max_hash of value c; sizes_out [n_classes][n] receives the size of
 * sketch i downsampled to value c (0 where c is finer than the sketch).  One upload, no downsampled host objects.  Errors: the
 * ksize / molecule / seed mismatch of the first sketch that does not match sketch 0. */
void smgpu_compare_all_pairs_mixed(const SourmashKmerMinHash *const *mhs, uintptr_t n, const uint32_t *class_of,
                                   const uint64_t *class_max_hash, uintptr_t n_classes, uint32_t *common_out, uint64_t *sizes_out);
/* Views for batched callers (src/sourmash/compare.py:326-358 reads `sig.minhash` per pair, and signature_first_mh
 * (src/core/src/ffi/signature.rs:167-182) CLONES the sketch every time): out_mhs[i] = the first sketch of sigs[i] as a BORROWED
 * handle -- valid while the signature lives and is not modified, never to be freed -- and params[i][8] = {ksize as stored,
 * hash_function, seed, max_hash, num, track_abundance, number of hashes, 0} in one call.  smgpu_minhashes_params: the same
 * parameter rows for sketch handles. */
void smgpu_signatures_sketch_views(const SourmashSignature *const *sigs, uintptr_t n, const SourmashKmerMinHash **out_mhs,
                                   uint64_t *params);
void smgpu_minhashes_params(const SourmashKmerMinHash *const *mhs, uintptr_t n, uint64_t *params);
/* Page-locked host memory (hipHostMalloc through the library's arena, which caches released blocks up to SMG_PINNED_CACHE_MAX
 * bytes): result matrices placed there are filled by ONE device-to-host copy at the link's rate.  smgpu_host_free takes only
 * pointers smgpu_host_alloc returned (others are ignored). */
void *smgpu_host_alloc(uintptr_t bytes);
void smgpu_host_free(void *ptr);
/* Bytes and nanoseconds the host-pointer entry points spent moving large pageable buffers (csrc/hostxfer.hpp) since the last reset:
 * out5 = {H2D bytes, D2H bytes, H2D ns, D2H ns, calls}.  Diagnostics for bench.py's API-level lines. */
void smgpu_xfer_stats(uint64_t *out5, bool reset);
/* The two directions of that path by themselves (tests): the n host pieces (pieces[i], lens[i] bytes, pageable or pinned, empty
 * ones allowed) are packed into one device buffer through the pinned ring, and that buffer comes back into out[0, out_bytes)
 * (out_bytes = the sum of lens) through the ring -- or directly when out is pinned (smgpu_host_alloc). */
void smgpu_xfer_roundtrip(const void *const *pieces, const uint64_t *lens, uintptr_t n, void *out, uint64_t out_bytes);
/* All pairs of BOTTOM-K (num) sketches in one launch (csrc/compare_ext.hip) -- what src/sourmash/compare.py:36-54 asks
 * kmerminhash_similarity for pair by pair: common_out[i][j] = |A ∩ B ∩ merged|, union_out[i][j] = |merged| with merged = the
 * num smallest hashes of A ∪ B, num taken from the sketch with the lower index (src/core/src/sketch/minhash.rs:593-621: the
 * merged sketch is built with self.num), jaccard_out = common / max(1, union) (minhash.rs:624-631), 1.0 on the diagonal.  n x n
 * host matrices, any may be NULL.  Errors: the compatibility error of the first sketch that does not match sketch 0. */
void smgpu_compare_num_all_pairs(const SourmashKmerMinHash *const *mhs, uintptr_t n, uint32_t *common_out, uint32_t *union_out,
                                 double *jaccard_out);
/* All pairs of ABUNDANCE-TRACKING sketches: sims_out[i][j] = angular similarity 1 - 2 acos(min(sum a_i b_j / (|a| |b|), 1)) / pi
 * (src/core/src/sketch/minhash.rs:635-680; 0 when a norm is 0; 1.0 on the diagonal as compare.py:33 has it).  The integer sums
 * come from one launch (prod_out[i][j] = sum over the common hashes of abund_i x abund_j, sumsq_out[i] = sum of squares; u64,
 * wrapping; optional), sqrt / acos from the host's libm.  Errors: compatibility as above; NeedsAbundanceTracking. */
void smgpu_compare_angular_all_pairs(const SourmashKmerMinHash *const *mhs, uintptr_t n, double *sims_out, uint64_t *prod_out,
                                     uint64_t *sumsq_out);
/* the host half of the above on its own: prod [n][n], sumsq [n] -> out [n][n] (n_threads 0: every host core) */
void smgpu_host_angular_f64(const uint64_t *prod, const uint64_t *sumsq, uintptr_t n, double *out, uint32_t n_threads);
/* The same kernels on caller-owned device buffers (CSR of sorted rows; d_nums[i] = num of sketch i; d_abunds parallel to
 * d_hashes; narrow = every abundance fits 32 bits).  Full n x n device matrices; d_union / d_jaccard may be NULL. */
void smgpu_compare_num_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, const uint32_t *d_nums, uint32_t n,
                           uint32_t *d_common, uint32_t *d_union, double *d_jaccard, void *stream);
void smgpu_compare_abund_raw(const uint64_t *d_hashes, const uint64_t *d_abunds, const uint64_t *d_offsets, uint32_t n, bool narrow,
                             uint32_t *d_common, uint64_t *d_prod, uint64_t *d_sumsq, void *stream);
/* The same with the number of hashes (= d_offsets[n]) given by the caller: only enqueues work.  The form above reads d_offsets[n]
 * back first and so blocks the caller until `stream` has drained. */
void smgpu_compare_abund_raw_n(const uint64_t *d_hashes, const uint64_t *d_abunds, const uint64_t *d_offsets, uint32_t n,
                               uint64_t total_hashes, bool narrow, uint32_t *d_common, uint64_t *d_prod, uint64_t *d_sumsq, void *stream);

/* Device-resident sketch collection + gather counters: the batched form of CounterGather
 * (src/sourmash/index/__init__.py:735-909).  A SketchSet is a CSR of n sorted sketches in HBM;
 * a Counter holds c[d] = |Q ∩ D_d| for every member d (CounterGather.add, :783-789), finds the
 * best match with the reference tie-break (highest count, then first inserted = lowest index;
 * :856-857) and applies consume (c[d] -= |I ∩ D_d| for every live d; :897-909) in one kernel. */
typedef struct SmgpuSketchSet SmgpuSketchSet;
typedef struct SmgpuCounter SmgpuCounter;
SmgpuSketchSet *smgpu_sketchset_new(const SourmashKmerMinHash *const *mhs, uintptr_t n);
void smgpu_sketchset_free(SmgpuSketchSet *ptr);
uintptr_t smgpu_sketchset_len(const SmgpuSketchSet *ptr);
/* Bulk loading: signature files -> one CSR in HBM, with no per-sketch host object.  Replaces the per-signature
 * loops of src/sourmash/save_load.py:218-234,448-549 / src/core/src/signature.rs:569-659 for the collection side
 * of compare / search / gather.  `paths`: .sig, .sig.gz, .zip (members chosen through SOURMASH-MANIFEST.csv when
 * present, src/sourmash/manifest.py:15-387), directories (walked for *.sig / *.sig.gz) or text files listing one
 * path per line.  Selection: ksize (0 = any), moltype ("DNA", "protein", "dayhoff", "hp"; NULL = any), scaled
 * (0 = as stored; otherwise sketches with scaled <= this, downsampled to it).  Rows keep the input order; all
 * selected sketches must share ksize / moltype / seed / scaled (the reference's compatibility errors otherwise).
 * n_threads = 0 uses every host core. */
typedef struct SmgpuCollection SmgpuCollection;
/* The host half on its own (no GPU needed): the CSR and manifest of what sketchset_load would put in HBM. */
SmgpuCollection *smgpu_collection_load(const char *const *paths, uintptr_t n_paths, uint32_t ksize, const char *moltype,
                                       uint64_t scaled, uint32_t n_threads);
void smgpu_collection_free(SmgpuCollection *ptr);
uintptr_t smgpu_collection_len(const SmgpuCollection *ptr);
uint64_t smgpu_collection_total_hashes(const SmgpuCollection *ptr);
uint64_t smgpu_collection_skipped(const SmgpuCollection *ptr);
const uint64_t *smgpu_collection_hashes(const SmgpuCollection *ptr);   /* borrowed, valid until free */
const uint64_t *smgpu_collection_offsets(const SmgpuCollection *ptr);  /* borrowed, len + 1 entries */
SourmashStr smgpu_collection_manifest(const SmgpuCollection *ptr);
void smgpu_collection_params(const SmgpuCollection *ptr, uint32_t *ksize, uint32_t *hash_function, uint64_t *seed,
                             uint64_t *max_hash, uint64_t *num);
SmgpuSketchSet *smgpu_sketchset_from_collection(const SmgpuCollection *ptr);
SmgpuSketchSet *smgpu_sketchset_load(const char *const *paths, uintptr_t n_paths, uint32_t ksize, const char *moltype,
                                     uint64_t scaled, uint32_t n_threads);
/* The records of a device buffer (smgpu_sketch_records_raw describes them) as a set that owns its CSR: flat scaled DNA
 * sketches, ksize 1 .. 88.  The pair buffer is sized from len / scaled; when repetitive input exceeds the estimate the call
 * is repeated once with the count.  Work is enqueued on the library's stream: the caller's writes to d_seq / d_starts must
 * have completed. */
SmgpuSketchSet *smgpu_sketchset_sketch_records(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, uint64_t n_records,
                                               uint32_t ksize, uint64_t seed, uint64_t scaled);
/* The records of a FASTA / FASTQ file (plain or gzip, at most 2 GiB of text) as such a set; the manifest rows carry each
 * record's name and the file name. */
SmgpuSketchSet *smgpu_sketchset_sketch_file(const char *path, uint32_t ksize, uint64_t seed, uint64_t scaled);
/* The same for protein / dayhoff / hp sketches (smgpu_sketch_residue_records_raw describes records, ksize -- in residues, 1 .. 79
 * -- hash_function and translate): the set carries hash_function, its manifest rows say protein / dayhoff / hp. */
SmgpuSketchSet *smgpu_sketchset_sketch_residue_records(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts,
                                                       const uint64_t *d_ends, uint64_t n_records, uint32_t ksize,
                                                       uint32_t hash_function, int32_t translate, uint64_t seed, uint64_t scaled);
/* The records of a FASTA / FASTQ file as such a set: a record ends in front of the next record's header line. */
SmgpuSketchSet *smgpu_sketchset_sketch_residue_file(const char *path, uint32_t ksize, uint32_t hash_function, int32_t translate,
                                                    uint64_t seed, uint64_t scaled);
/* ---- a sketch's k-mers in sequences (csrc/sketch_find.hip; `sourmash sig kmers`, src/sourmash/sig/__main__.py:1087-1310) ----
 * The way back from a sketch to the sequences it came from: every position of a buffer or a file whose k-mer hashes into a
 * query, by record.  The query is the union of n compatible flat scaled DNA sketches, merged as the reference merges them
 * (:1113-1135: the first one's copy_and_clear, abundances off, merge of each -- an incompatible sketch raises what
 * kmerminhash_merge raises).  Refused with an error: no sketch, no hash, a num sketch, a protein / dayhoff / hp sketch.  The
 * handle is made on the host; its hashes and their bucket directory go to the device when it is first used there. */
typedef struct SmgpuKmerQuery SmgpuKmerQuery;
typedef struct SmgpuKmerMatches SmgpuKmerMatches;
SmgpuKmerQuery *smgpu_kmerquery_new(const SourmashKmerMinHash *const *mhs, uintptr_t n);
void smgpu_kmerquery_free(SmgpuKmerQuery *ptr);
uint64_t smgpu_kmerquery_len(const SmgpuKmerQuery *ptr);
/* Scratch size of smgpu_find_kmers_raw for a capacity of matched (hash, position) pairs. */
uint64_t smgpu_find_kmers_workspace_bytes(uint64_t pair_capacity, uint64_t n_records);
/* d_seq[0,len) ASCII (any alignment), records as for smgpu_sketch_records_raw -> one row per position i whose k-mer
 * d_seq[i, i + k) holds only ACGTacgt, lies inside one record and whose canonical hash is a member of the query; a k-mer that
 * occurs at several positions, or on both strands, is a row at each.  Rows are ordered by position, so by record:
 * d_positions (absolute in d_seq), d_hashes, d_kmers (NULL: not wanted; row * k bytes, the window as it stands, upper-cased);
 * the rows of record r are [d_offsets[r], d_offsets[r + 1]).  The query's ksize must be 1 .. 88.  capacity: rows the three
 * arrays hold and matched pairs the workspace holds; d_offsets: n_records + 1 entries.  d_result (device, 4 x u64): [0]
 * matched pairs, [1] rows, [3] non-zero when the starts are refused.  Synchronises the stream three times: refused starts
 * launch nothing behind the check, and the sort needs the matched count.  Returns the rows, or
 * UINT64_MAX with an error set: starts not ascending or ending behind len; ksize above 88; or more pairs matched than
 * capacity -- the error says so and names the count (also in d_result[0]), and the caller retries with a larger buffer. */
uint64_t smgpu_find_kmers_raw(const SmgpuKmerQuery *query, const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts,
                              uint64_t n_records, uint64_t *d_positions, uint64_t *d_hashes, uint8_t *d_kmers,
                              uint64_t capacity, uint64_t *d_offsets, uint64_t *d_result, void *d_workspace,
                              uint64_t workspace_bytes, void *stream);
/* Only its k-mer kernel (no assign, no sort): every matched hash appended unordered to d_hashes and the position of its
 * k-mer's first byte in d_seq to d_positions; the count is added to *d_count (device u64, caller zeroes).  grid == 0 is the
 * library's own number of workgroups, otherwise exactly `grid` (at most 1048576; for tests: many tiles per workgroup on a
 * small input).  Asynchronous once the query is on the device. */
void smgpu_find_kmers_kernel_raw(const SmgpuKmerQuery *query, const uint8_t *d_seq, uint64_t len, uint64_t *d_hashes,
                                 uint64_t *d_positions, uint64_t capacity, uint64_t *d_count, uint32_t grid, void *stream);
/* The records of a FASTA / FASTQ file (plain or gzip, at most 2 GiB of text; the files smgpu_sketchset_sketch_file takes)
 * searched in one pass.  The accessors borrow from the handle: offsets (n_records + 1), positions (relative to the row's
 * record), hashes, kmers (n_rows * ksize bytes); a record's name; the sequence of a record that has rows (NULL otherwise). */
SmgpuKmerMatches *smgpu_find_kmers_file(const SmgpuKmerQuery *query, const char *path);
void smgpu_kmermatches_free(SmgpuKmerMatches *ptr);
uint64_t smgpu_kmermatches_n_records(const SmgpuKmerMatches *ptr);
uint64_t smgpu_kmermatches_n_rows(const SmgpuKmerMatches *ptr);
uint64_t smgpu_kmermatches_n_bases(const SmgpuKmerMatches *ptr);
const uint64_t *smgpu_kmermatches_offsets(const SmgpuKmerMatches *ptr);
const uint64_t *smgpu_kmermatches_positions(const SmgpuKmerMatches *ptr);
const uint64_t *smgpu_kmermatches_hashes(const SmgpuKmerMatches *ptr);
const uint8_t *smgpu_kmermatches_kmers(const SmgpuKmerMatches *ptr);
const uint64_t *smgpu_kmermatches_record_lengths(const SmgpuKmerMatches *ptr);
SourmashStr smgpu_kmermatches_record_name(const SmgpuKmerMatches *ptr, uint64_t record);
const uint8_t *smgpu_kmermatches_record_sequence(const SmgpuKmerMatches *ptr, uint64_t record, uint64_t *len);
/* rows[0..n) of a loaded set as a new set: row gather on the device, manifest rows follow.  Replaces the object loop of
 * Index.counter_gather (src/sourmash/index/__init__.py:302-320: `for result in self.prefetch(...): counter.add(
 * result.signature, ...)`): the rows that pass the prefetch become the counter's database without leaving HBM. */
SmgpuSketchSet *smgpu_sketchset_subset(const SmgpuSketchSet *set, const uint64_t *rows, uintptr_t n);
/* A set from a CSR in device memory (row r = d_hashes[d_offsets[r] .. d_offsets[r + 1]) ascending; n + 1 offsets): the rows are
 * copied.  ksize in residues of the molecule; names / filenames: NULL or one C string per row for the manifest. */
SmgpuSketchSet *smgpu_sketchset_from_csr(const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n, uint32_t ksize,
                                         uint32_t hash_function, uint64_t seed, uint64_t max_hash, uint64_t num,
                                         const char *const *names, const char *const *filenames);
/* names / filenames: NULL (left as they are) or one C string per row: the names the set's manifest rows carry and its signatures
 * are written with (a set built from sketch handles has none until they are given). */
void smgpu_sketchset_set_names(SmgpuSketchSet *set, const char *const *names, const char *const *filenames);
/* The signature writer: a set's rows as signature JSON, MD5 identities and gzip members, produced on the device (csrc/sigwrite.hpp).
 * md5sums: out[16 r .. 16 r + 16) = the MD5 of row r (the `md5sum` of its sketch).
 * to_json: the JSON array of the rows' signatures (rows NULL: all n rows of the set), byte for byte what signatures_save_buffer gives
 * for the same signatures at compression 0; above 0 the array as one gzip member.  Freed with nodegraph_buffer_free. */
void smgpu_sketchset_md5sums(const SmgpuSketchSet *set, uint8_t *out);
const uint8_t *smgpu_sketchset_to_json(const SmgpuSketchSet *set, const uint64_t *rows, uintptr_t n, uint8_t compression, uintptr_t *size);
/* A file written from the device; the suffix of the path chooses the form: .zip (gzip members signatures/<md5>.sig.gz, stored, and
 * SOURMASH-MANIFEST.csv last), .gz (the JSON array as one gzip member), anything else the JSON array.  Several sets may be added;
 * names / filenames: NULL or one C string per row.  The file exists once close has returned without an error, and not otherwise. */
typedef struct SmgpuSigWriter SmgpuSigWriter;
SmgpuSigWriter *smgpu_sigwriter_new(const char *path, uint8_t compression);
void smgpu_sigwriter_add(SmgpuSigWriter *writer, const SmgpuSketchSet *set, const char *const *names, const char *const *filenames);
void smgpu_sigwriter_close(SmgpuSigWriter *writer);
void smgpu_sigwriter_free(SmgpuSigWriter *writer);
/* out[0 .. 7): ms in lengths, md5, text, crc, pack, device-to-host copies, file writes since the last reset; out[7 .. 12): rows,
 * hashes, bytes of text, bytes written, rows whose MD5 the host computed. */
void smgpu_sigwrite_stats(double *out, int32_t reset);
/* The writer's kernels on caller-owned device buffers.  md5: 16 bytes a row into d_md5, rows whose message exceeds long_row_bound
 * bytes on the host (0: the library's bound) -> rows the host did.  json: the rows' documents into d_text (per_doc: one `[{...}]` per
 * row on 16-byte lines; else one array), params = ksize, hash_function, seed, max_hash, num, docs_out = offset, length per row
 * -> bytes of text.  deflate: every document (offset, length; offsets multiples of 16, d_text itself 16-byte aligned) of d_text as a gzip member in d_out,
 * compression 0 stored blocks, else literal-only Huffman blocks packed `chunk` bytes a workgroup (0: the default) -> bytes of output.
 * json and deflate write nothing when the result exceeds the capacity. */
uint64_t smgpu_sigwrite_md5_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n_rows, uint32_t ksize, uint64_t long_row_bound,
                                uint8_t *d_md5, void *stream);
uint64_t smgpu_sigwrite_json_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n_rows, const uint64_t *params,
                                 const char *const *names, const char *const *filenames, int32_t per_doc, uint8_t *d_text, uint64_t capacity,
                                 uint64_t *docs_out, void *stream);
uint64_t smgpu_deflate_literals_raw(const uint8_t *d_text, uint64_t text_len, const uint64_t *docs, uint32_t n_docs, uint8_t compression,
                                    uint32_t chunk, uint8_t *d_out, uint64_t capacity, uint64_t *members_out, void *stream);

uint64_t smgpu_sketchset_total_hashes(const SmgpuSketchSet *ptr);
uint64_t smgpu_sketchset_skipped(const SmgpuSketchSet *ptr);
/* One manifest row per CSR row, in the reference's CSV manifest format (manifest.py:29-41,128-146). */
SourmashStr smgpu_sketchset_manifest(const SmgpuSketchSet *ptr);
void smgpu_sketchset_params(const SmgpuSketchSet *ptr, uint32_t *ksize, uint32_t *hash_function, uint64_t *seed,
                            uint64_t *max_hash, uint64_t *num);
void smgpu_sketchset_sizes(const SmgpuSketchSet *ptr, uint64_t *sizes_out);
SourmashKmerMinHash *smgpu_sketchset_get(const SmgpuSketchSet *ptr, uint64_t index);
void smgpu_sketchset_device_csr(const SmgpuSketchSet *ptr, const uint64_t **d_hashes, const uint64_t **d_offsets);
/* counts_out[row] = |query ∩ row| for every row of the set (Index.find's shared sizes, index/__init__.py:115-170) */
void smgpu_sketchset_overlaps(const SmgpuSketchSet *ptr, const SourmashKmerMinHash *query, uint64_t *counts_out);
/* n x n matrices of a loaded set on the host (either may be NULL); same kernels as smgpu_compare_all_pairs. */
void smgpu_sketchset_compare(const SmgpuSketchSet *ptr, uint32_t *common_out, double *jaccard_out);
/* ---- many queries against a collection in one pass over it (csrc/overlap_many.hip, csrc/many_core.hpp) ----
 * The reference searches many against many with a loop of Index.search / Index.prefetch around the collection
 * (src/sourmash/index/__init__.py:115-170, 202-256).  Here the queries' hashes are merged into one index on the device and the
 * collection is read once: the hits -- the (query, row) pairs whose common count reaches the query's `need` -- leave as triples
 * ordered by (query, row).  When the two sets differ in scaled every pair is taken at the coarser one (minhash.rs:539-548).
 * geometry: lanes of a workgroup, the default queries per pass, and the most a caller may ask for.
 * need: the integer filter of a search at `threshold` for queries of the given sizes (mode 0 Jaccard, 1 containment, 2 max
 * containment): never above the smallest count that passes the float test, never 0.  Host only. */
typedef struct SmgpuManyHits SmgpuManyHits;
void smgpu_many_geometry(uint32_t *workgroup, uint32_t *q_block, uint32_t *q_block_max);
void smgpu_many_need(uint32_t mode, double threshold, const uint64_t *sizes, uint64_t m, uint32_t *need_out);
uint64_t smgpu_many_overlap_workspace_bytes(uint64_t m, uint64_t q_total, uint64_t capacity);
/* Both CSRs in device memory: the queries (m rows, d_qoffsets m + 1 entries, q_total hashes in all) and the collection (n_rows
 * rows); rows ascending.  d_need: one u32 >= 1 per query; cutoff: only hashes <= cutoff count (the smaller max_hash of the two
 * sets; UINT64_MAX: all).  q_block: queries counted per pass over the collection (0: the default); grid: workgroups of a pass (0:
 * the library's number).  The hits go to d_queries / d_rows / d_common (capacity entries each), ordered by (query, row).  d_result
 * (device, 4 x u64): [0] the true number of hits, [1] distinct query hashes <= cutoff, [2] passes.  Returns the number of hits;
 * when it exceeds the capacity the arrays hold the first `capacity` hits found, unordered, nothing is written behind them, and the
 * caller runs again with room.  Synchronises the stream.  UINT64_MAX with an error set: a refused argument, or no device. */
uint64_t smgpu_many_overlap_raw(const uint64_t *d_qhashes, const uint64_t *d_qoffsets, uint64_t m, uint64_t q_total,
                                const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n_rows, const uint32_t *d_need,
                                uint64_t cutoff, uint32_t q_block, uint32_t grid, uint32_t *d_queries, uint32_t *d_rows,
                                uint32_t *d_common, uint64_t capacity, uint64_t *d_result, void *d_workspace,
                                uint64_t workspace_bytes, void *stream);
/* d_sizes[r] = hashes of row r that are <= cutoff: a set's sizes at the common scaled.  Asynchronous on `stream`. */
void smgpu_many_sizes_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n, uint64_t cutoff, uint64_t *d_sizes,
                          void *stream);
/* The same for a resident set, into a host array (max_hash 0: the full sizes). */
void smgpu_sketchset_sizes_at(const SmgpuSketchSet *set, uint64_t max_hash, uint64_t *sizes_out);
/* Every row of `queries` against every row of `db`.  need: one count per query (NULL: need_all for each); never 0.  The sets must
 * be compatible in the reference's order (check_compatible, minhash.rs:886-912: ksize, hash function, seed) and scaled; num sets
 * are refused.  The capacity is the library's choice; a result that does not fit is computed once more with room.  The getters
 * borrow from the handle: len hits (queries, rows, common), the sizes of every query and every row at the common scaled, that
 * scaled; stats: out[0 .. 3) ms of the index build, the passes and the final sort (device), [3] ms of the whole call (host), [4]
 * reruns, [5] passes over the collection. */
SmgpuManyHits *smgpu_sketchset_overlaps_many(const SmgpuSketchSet *db, const SmgpuSketchSet *queries, const uint32_t *need,
                                             uint32_t need_all);
void smgpu_manyhits_free(SmgpuManyHits *ptr);
uint64_t smgpu_manyhits_len(const SmgpuManyHits *ptr);
const uint32_t *smgpu_manyhits_queries(const SmgpuManyHits *ptr);
const uint32_t *smgpu_manyhits_rows(const SmgpuManyHits *ptr);
const uint32_t *smgpu_manyhits_common(const SmgpuManyHits *ptr);
const uint64_t *smgpu_manyhits_query_sizes(const SmgpuManyHits *ptr);
const uint64_t *smgpu_manyhits_row_sizes(const SmgpuManyHits *ptr);
uint64_t smgpu_manyhits_scaled(const SmgpuManyHits *ptr);
void smgpu_manyhits_stats(const SmgpuManyHits *ptr, double *out6);
/* Test support: the capacity smgpu_sketchset_overlaps_many first tries (0: its own choice), to see the second run. */
void smgpu_many_set_first_capacity(uint64_t capacity);

/* ---- gather of many queries against a collection in one call (csrc/gather_many.hip, csrc/gather_many_core.hpp) ----
 * The reference decomposes many queries against one collection with a loop of GatherDatabases (src/sourmash/search.py:877-949
 * over CounterGather, src/sourmash/index/__init__.py:735-909).  Here the many-queries pass above finds every query's candidates
 * (the rows sharing at least max(1, threshold) hashes with it) and one kernel then runs the min-set-cover loops side by side: a
 * workgroup a query, the counters of its candidates and its uncovered hashes in LDS.  Per query: the largest counter wins a
 * round (ties: the lowest row), the loop ends at a best counter of 0 or below threshold_hashes, the round's intersect is what
 * the winner holds of the still-uncovered hashes, and every counter drops by what it shares with that.  Sets of different
 * scaled meet at the coarser one.
 * geometry: lanes of a workgroup, and the default caps: the most hashes (<= cutoff) and the most candidates a query may have to
 * run in that kernel.  workspace_bytes: for m queries with n_hits hits whose common counts sum to total_common. */
void smgpu_gather_many_geometry(uint32_t *workgroup, uint32_t *max_query_hashes, uint32_t *max_candidates);
uint64_t smgpu_gather_many_workspace_bytes(uint64_t m, uint64_t n_hits, uint64_t total_common);
/* Both CSRs in device memory as for smgpu_many_overlap_raw, and the hits that call produced for them, ordered by (query, row);
 * d_hit_common must be the true common counts at `cutoff` (checked: a row that shares another number of hashes with its query
 * is an error).  The picks of query q go to [first hit of q, + d_out_rounds[q]) of d_out_rows / d_out_isect, in rank order;
 * the slots behind them are left untouched.  A query with more than max_query_hashes hashes <= cutoff or more than
 * max_candidates hits is not run: d_status[q] = 1 and nothing else is written for it (d_status[q] = 0 for the others).  Caps of
 * 0 mean the defaults; grid: workgroups of the launches (0: the library's numbers).  Returns the total number of rounds.
 * Synchronises the stream.  UINT64_MAX with an error set: a refused argument (caps beyond what LDS holds, grid above 1048576, a
 * null pointer, a workspace smaller than smgpu_gather_many_workspace_bytes says, 2^32 rows or hits), or no device. */
uint64_t smgpu_gather_many_raw(const uint64_t *d_qhashes, const uint64_t *d_qoffsets, uint64_t m,
                               const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n_rows,
                               const uint32_t *d_hit_queries, const uint32_t *d_hit_rows, const uint32_t *d_hit_common,
                               uint64_t n_hits, uint64_t cutoff, uint64_t threshold_hashes,
                               uint32_t max_query_hashes, uint32_t max_candidates, uint32_t grid,
                               uint32_t *d_out_rows, uint32_t *d_out_isect, uint32_t *d_out_rounds, uint32_t *d_status,
                               void *d_workspace, uint64_t workspace_bytes, void *stream);
/* [gather(query q of `queries`) against `db` for every q]: compatibility as for smgpu_sketchset_overlaps_many.  Queries are run
 * in contiguous batches whose forward lists stay under a budget; a query beyond a cap runs through the one-query path
 * (smgpu_counter_new / smgpu_counter_gather on the resident buffers), so the answer is always complete.  The getters borrow from
 * the handle: offsets (m + 1 entries) into rows / isect, the picks of a query in rank order, and the common scaled; stats:
 * out[0 .. 4) ms of the candidate pass, the fill, the sort and the rounds kernel (device), [4] ms of the one-query way out and
 * [5] of the whole call (host), [6] queries that took the way out, [7] batches. */
typedef struct SmgpuManyGather SmgpuManyGather;
SmgpuManyGather *smgpu_sketchset_gather_many(const SmgpuSketchSet *db, const SmgpuSketchSet *queries, uint64_t threshold_hashes);
void            smgpu_manygather_free(SmgpuManyGather *ptr);
const uint64_t *smgpu_manygather_offsets(const SmgpuManyGather *ptr);   /* m + 1 */
const uint32_t *smgpu_manygather_rows(const SmgpuManyGather *ptr);
const uint32_t *smgpu_manygather_isect(const SmgpuManyGather *ptr);
uint64_t        smgpu_manygather_scaled(const SmgpuManyGather *ptr);
void            smgpu_manygather_stats(const SmgpuManyGather *ptr, double *out8);
/* Test support: the caps and the batch budget smgpu_sketchset_gather_many works with (0: the default of each). */
void smgpu_gather_many_set_limits(uint32_t max_query_hashes, uint32_t max_candidates, uint64_t batch_common);
/* ---- the result rows of gather for many queries (csrc/gather_rows.hip, csrc/gather_rows_core.hpp) ----
 * The reference builds a gather row per round from MinHash objects and a {hash: abundance} dictionary (GatherDatabases,
 * src/sourmash/search.py:877-949; GatherResult.build_gather_result :480-505).  Every number of such a row is a function of a few
 * integers per pick and the abundances of the query hashes the pick covered first; one pass over resident data gives them for the
 * picks of every query.  The picks of query q are d_pick_rows[d_pick_offsets[q], d_pick_offsets[q + 1]) in rank order.  The OWNER
 * of a query hash is the lowest rank among its query's picks whose row holds it: "remaining query ∩ match" of that round.
 * Everything is taken at `cutoff` (the smaller max_hash of the two sets).  Per pick: orig_common = |query ∩ row|, unique = hashes
 * it owns, weighted = the sum of their abundances, and abund_values[abund_offsets[p], abund_offsets[p + 1]) their abundances in
 * ascending hash order.  Per query: query_sizes = hashes <= cutoff, total_weighted = the sum of their abundances.
 * workspace_bytes: for m queries of q_total hashes in all with n_picks picks (UINT64_MAX with an error set: 2^32 of either). */
uint64_t smgpu_gather_rows_workspace_bytes(uint64_t m, uint64_t q_total, uint64_t n_picks);
/* Everything in device memory.  d_qoffsets (m + 1) are positions in d_qhashes[0, q_total); d_qabunds is aligned with d_qhashes
 * (NULL: every abundance is 1).  Outputs: d_owner (q_total; the owning rank, 0xffffffff for none), d_orig_common / d_unique /
 * d_weighted (n_picks), d_abund_offsets (n_picks + 1), d_abund_values (room for q_total), d_query_sizes / d_total_weighted (m).
 * grid: workgroups of the launches (0: the library's numbers).  Returns the number of owned hashes (= d_abund_offsets[n_picks]).
 * Synchronises the stream.  UINT64_MAX with an error set: a refused argument (a null pointer, a workspace smaller than
 * smgpu_gather_rows_workspace_bytes says, grid above 1048576, 2^32 queries, query hashes, rows or picks, a pick row >= n_rows,
 * offsets that descend or leave their arrays), or no device. */
uint64_t smgpu_gather_rows_raw(const uint64_t *d_qhashes, const uint64_t *d_qabunds, const uint64_t *d_qoffsets, uint64_t m, uint64_t q_total,
                               const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n_rows,
                               const uint64_t *d_pick_offsets, const uint32_t *d_pick_rows, uint64_t n_picks,
                               uint64_t cutoff, uint32_t grid,
                               uint32_t *d_owner, uint32_t *d_orig_common, uint32_t *d_unique, uint64_t *d_weighted,
                               uint64_t *d_abund_offsets, uint64_t *d_abund_values, uint64_t *d_query_sizes, uint64_t *d_total_weighted,
                               void *d_workspace, uint64_t workspace_bytes, void *stream);
/* smgpu_sketchset_gather_many, then the pass above on the same resident buffers; compatibility as for
 * smgpu_sketchset_overlaps_many.  abunds: host array aligned with the queries' hashes (all of them, in row order), or NULL.  The
 * pass is checked against the gather: a pick that owns another number of hashes than the gather reported is an error.
 * smgpu_sketchset_gather_rows: one query through the one-query gather (smgpu_counter_new / smgpu_counter_gather on the resident
 * set), abundances from the sketch when it tracks them.  The getters borrow from the handle: offsets (queries + 1) into the
 * per-pick arrays rows / isect / orig_common / weighted; abund_offsets (picks + 1) into abund_values; query_sizes and
 * total_weighted per query, row_sizes per row of the set, all at the common scaled; stats: out[0] ms of the gather (host),
 * [1 .. 4) of the owner pass, the tally pass and the pair sort (device), [4] of the whole call (host). */
typedef struct SmgpuGatherRows SmgpuGatherRows;
SmgpuGatherRows *smgpu_sketchset_gather_rows_many(const SmgpuSketchSet *db, const SmgpuSketchSet *queries, const uint64_t *abunds,
                                                  uint64_t threshold_hashes);
SmgpuGatherRows *smgpu_sketchset_gather_rows(const SmgpuSketchSet *db, const SourmashKmerMinHash *query, uint64_t threshold_hashes);
void            smgpu_gatherrows_free(SmgpuGatherRows *ptr);
uint64_t        smgpu_gatherrows_queries(const SmgpuGatherRows *ptr);
uint64_t        smgpu_gatherrows_n_rows(const SmgpuGatherRows *ptr);
const uint64_t *smgpu_gatherrows_offsets(const SmgpuGatherRows *ptr);
const uint32_t *smgpu_gatherrows_rows(const SmgpuGatherRows *ptr);
const uint32_t *smgpu_gatherrows_isect(const SmgpuGatherRows *ptr);
const uint32_t *smgpu_gatherrows_orig_common(const SmgpuGatherRows *ptr);
const uint64_t *smgpu_gatherrows_weighted(const SmgpuGatherRows *ptr);
const uint64_t *smgpu_gatherrows_abund_offsets(const SmgpuGatherRows *ptr);
const uint64_t *smgpu_gatherrows_abund_values(const SmgpuGatherRows *ptr);
const uint64_t *smgpu_gatherrows_query_sizes(const SmgpuGatherRows *ptr);
const uint64_t *smgpu_gatherrows_row_sizes(const SmgpuGatherRows *ptr);
const uint64_t *smgpu_gatherrows_total_weighted(const SmgpuGatherRows *ptr);
uint64_t        smgpu_gatherrows_scaled(const SmgpuGatherRows *ptr);
void            smgpu_gatherrows_stats(const SmgpuGatherRows *ptr, double *out5);
SmgpuCounter *smgpu_counter_new(const SmgpuSketchSet *set, const SourmashKmerMinHash *query);
void smgpu_counter_free(SmgpuCounter *ptr);
void smgpu_counter_get(const SmgpuCounter *ptr, uint64_t *counts_out);
void smgpu_counter_set(SmgpuCounter *ptr, uint64_t index, uint64_t value);
bool smgpu_counter_best(const SmgpuCounter *ptr, uint64_t *index, uint64_t *count);
void smgpu_counter_consume(SmgpuCounter *ptr, const SourmashKmerMinHash *intersect);
/* The whole min-set-cover loop of GatherDatabases (src/sourmash/search.py:877-949) from the counter's current
 * state, every round on the GPU: winner index (order of smgpu_sketchset_new) and |intersect| per round into the
 * host arrays; -> number of rounds.  threshold_hashes = ceil(threshold_bp / scaled) (search.py:15-37). */
uint64_t smgpu_counter_gather(SmgpuCounter *ptr, uint64_t threshold_hashes, uint64_t *out_index, uint64_t *out_isect,
                              uint64_t cap);

/* The same loop over caller-owned device buffers (query: sorted unique u64; database: CSR shard whose rows have
 * global indices index_base, index_base+1, ...).  new_raw inverts the shard against the query once (query hash ->
 * rows holding it), so a round costs |I| postings walks instead of a pass over the database.
 *   single GPU:  begin, run.
 *   sharded:     begin, then per exchange  topk_export_raw (this shard's k best rows as records
 *                [key, bound, len, hashes...] of `stride` u64 words, key = (count << 32) | ~global index, bound = the
 *                best key the shard keeps back) -> ONE all-gather of the records -> cands_load_raw on every rank
 *                (at most 64 records in all) -> replay_raw(rounds): each round takes the best candidate, which is
 *                the global arg-max as long as its key is not below any kept-back key (counters only decrease), and
 *                applies it to the local postings and to the candidates' counters; rounds turn into no-ops once that
 *                test fails (the next exchange decides) or a stop rule fired.  poll every few exchanges.  Nothing
 *                between two polls needs the host; every rank replays the same rounds.
 *                Replaces the per-round walk of CounterGather.peek / consume, src/sourmash/index/__init__.py:817-909. */
typedef struct SmgpuGather SmgpuGather;
SmgpuGather *smgpu_gather_new_raw(const uint64_t *d_query, uint64_t nq, const uint64_t *d_hashes,
                                  const uint64_t *d_offsets, uint64_t ndb, uint64_t index_base, void *stream);
void smgpu_gather_free(SmgpuGather *ptr);
uint64_t smgpu_gather_postings(const SmgpuGather *ptr);
/* What the build and the last smgpu_gather_run cost, so that one benchmark line separates kernels from host effects
 * (waits for the build's kernels): out[0] build kernel span in ms (HIP events on the build's stream), out[1] build host
 * wall clock ms (the smgpu_gather_new_raw call), out[2] ms inside the driver's allocator during the build (0 once the
 * arena is warm), out[3] driver allocations made, out[4] host synchronisations of the build, out[5] ms the host waited in
 * them, out[6] GPU span in ms of the last run's rounds (events around the loop), out[7] host wall clock ms of that run,
 * out[8] times the resident loop kernel gave up because its grid was not resident as a whole (another kernel or process held
 * CUs) and the two-kernel rounds / the record protocol took over from the untouched state. */
void smgpu_gather_stats(SmgpuGather *ptr, double *out9);
/* The library's device arena (csrc/arena.hpp): every index / scratch block comes from it and is cached on release.
 * out[0] driver allocations, out[1] driver frees, out[2] ns inside the driver, out[3] reuse hits, out[4] live bytes,
 * out[5] cached bytes, out[6] peak bytes held, out[7] reuses that waited on another stream's event. */
void smgpu_arena_stats(uint64_t *out8);
void smgpu_arena_trim(uint64_t keep_bytes);     /* give cached blocks back to the driver (0: all of them) */
/* The gzip reader of the ingest path on its own (host threads, no device): inflates `path`, returns the decompressed length,
 * the CRC-32 of the bytes it produced and whether the many-thread form (csrc/pargz.hpp: block starts found by search,
 * window references resolved afterwards) carried the whole file; up to `cap` bytes are copied to `out` (may be NULL).
 * threads 0: the CPUs this process may use; span_bytes 0: 1 MiB of compressed data per work unit.
 * Replaces the single zlib stream behind screed / niffler (src/sourmash/command_sketch.py:697, src/core/benches/compute.rs:35-38). */
uint64_t smgpu_gunzip_file(const char *path, uint32_t threads, uint64_t span_bytes, uint8_t *out, uint64_t cap, uint32_t *crc32_out,
                           bool *parallel_used);
/* The 15-bit code the reader's marker bytes carry for window position `p` (an involution on 0..32767): the 128 codes whose two
 * marker bytes coincide -- and so read like a data byte >= 0x80 -- belong to positions 0..127 (tests/test_pargz_cpu.py). */
uint32_t smgpu_gunzip_position_code(uint32_t p);
void smgpu_gather_counters_get(const SmgpuGather *ptr, uint64_t *counts_out, void *stream);
void smgpu_gather_begin(SmgpuGather *ptr, uint64_t threshold_hashes, uint64_t max_rounds, void *stream);
uint64_t smgpu_gather_run(SmgpuGather *ptr, uint64_t *out_index, uint64_t *out_isect, uint64_t cap, void *stream);
/* Several ranks, one shard each, running the SAME rounds inside their resident loop kernels: the local winners meet in
 * host-visible memory every rank can reach (POSIX shared memory registered with HIP when the ranks are processes on one node;
 * private pinned memory when one process drives all of them), the best is the round's winner everywhere and its query
 * positions travel through the same memory -- no host collective inside the loop.  xchg_new: shm_name NULL/"" = private
 * memory; else rank 0 creates (create = true) and the others open it after a barrier.  rowcap >= the longest row of any shard
 * (smgpu_gather_longest_row, MAX over ranks).  launch_shared enqueues the armed loop (after smgpu_gather_begin) and returns
 * false when this index cannot run the resident loop (every rank must check smgpu_gather_loop_eligible first and all agree);
 * run_id: the same on every rank, different from the previous run on this memory; n_wg: workgroups (0 = one per CU).
 * smgpu_gather_results then waits and reads the picks (identical on every rank).  Replaces the per-round walk of
 * CounterGather.peek / consume across shards, src/sourmash/index/__init__.py:817-909. */
typedef struct SmgpuGatherXchg SmgpuGatherXchg;
SmgpuGatherXchg *smgpu_gather_xchg_new(const char *shm_name, uint32_t world, uint64_t rowcap, bool create);
void smgpu_gather_xchg_free(SmgpuGatherXchg *ptr);
bool smgpu_gather_loop_eligible(const SmgpuGather *ptr, uint32_t n_wg);
/* (one process driving several ranks: reserve every rank's loop memory BEFORE the first launch -- an allocation may synchronise
 *  the device while a loop that already runs waits for its peers) */
void smgpu_gather_loop_reserve(SmgpuGather *ptr, uint32_t n_wg, uint64_t rowcap, void *stream);
/* The exchange in DEVICE memory instead (BASELINE north_star: the gather exchange "over xGMI"): rank `rank` allocates ITS area
 * (fine-grained device memory), exports it (handle_out: smgpu_gather_xchg_ipc_handle_size() bytes, a hipIpcMemHandle_t), the
 * handles travel by one all-gather, and every rank opens its peers' (world <= 16, the ranks of one node).  A rank's loop kernel
 * writes its own area and polls the others'.  smgpu_gather_launch_shared takes either kind. */
SmgpuGatherXchg *smgpu_gather_xchg_new_device(uint32_t world, uint32_t rank, uint64_t rowcap);
uintptr_t smgpu_gather_xchg_ipc_handle_size(void);
void smgpu_gather_xchg_ipc_export(const SmgpuGatherXchg *xchg, uint8_t *handle_out);
void smgpu_gather_xchg_ipc_open(SmgpuGatherXchg *xchg, uint32_t peer_rank, const uint8_t *handle);
bool smgpu_gather_xchg_is_device(const SmgpuGatherXchg *xchg);
bool smgpu_gather_launch_shared(SmgpuGather *ptr, SmgpuGatherXchg *xchg, uint32_t rank, uint32_t run_id, uint32_t n_wg, void *stream);
/* Test support: `n_wg` workgroups that keep `lds_bytes` of LDS each and spin for `micros` microseconds on `stream` -- "somebody
 * else's kernel holds CUs of this device" (the resident gather loop must step aside for the two-kernel rounds, not fail). */
void smgpu_debug_hold_cus(uint32_t n_wg, uint32_t lds_bytes, uint64_t micros, void *stream);
/* Test support: d_pos_out[i] = position of d_probes[i] in the sorted distinct query d_query[0 .. nq) (nq >= 1), or 0xffffffff when it
 * is not there, through the query index of the overlap and gather passes.  form 0: the table lookup, 1: the bucket-record lookup,
 * 2: the record lookup in its two-step form (load, then match).  Stream-ordered; scratch comes from the arena. */
void smgpu_debug_qindex_find(const uint64_t *d_query, uint64_t nq, const uint64_t *d_probes, uint64_t n, int32_t form,
                             uint32_t *d_pos_out, void *stream);
uint64_t smgpu_gather_longest_row(const SmgpuGather *ptr);   /* hashes in the shard's longest row: stride >= 3 + the longest row of any shard */
void smgpu_gather_topk_export_raw(SmgpuGather *ptr, uint64_t *d_records, uint32_t k, uint64_t stride, void *stream);
void smgpu_gather_cands_load_raw(SmgpuGather *ptr, const uint64_t *d_records, uint32_t n_records, uint64_t stride,
                                 void *stream);
void smgpu_gather_replay_raw(SmgpuGather *ptr, uint32_t rounds, void *stream);
uint64_t smgpu_gather_poll(SmgpuGather *ptr, bool *done, void *stream);
uint64_t smgpu_gather_results(SmgpuGather *ptr, uint64_t *out_index, uint64_t *out_isect, uint64_t cap, void *stream);

/* Gather primitives (src/sourmash/index/__init__.py:735-909):
 *   overlap:  d_overlap[d] = |Q ∩ D_d| (op 0, CounterGather.add) or
 *             d_overlap[d] -= |Q ∩ D_d| saturating (op 1, CounterGather.consume)
 *   argmax:   *d_best = max(*d_best, (count << 32) | ~(index_base + d)): highest count,
 *             ties to the lowest index (Counter.most_common order) -- one u64 MAX
 *             all-reduce across GPUs picks the global winner.
 *   intersect: sorted list Q ∩ R into d_out, size into *d_n (device u64). */
void smgpu_overlap_raw(const uint64_t *d_query, uint64_t nq, const uint64_t *d_hashes, const uint64_t *d_offsets,
                       uint64_t ndb, uint64_t *d_overlap, int32_t op, void *stream);
void smgpu_argmax_raw(const uint64_t *d_overlap, uint64_t ndb, uint64_t index_base, uint64_t *d_best, void *stream);
uint64_t smgpu_intersect_workspace_bytes(uint64_t n);
void smgpu_intersect_raw(const uint64_t *d_a, uint64_t na, const uint64_t *d_b, uint64_t nb, uint64_t *d_out,
                         uint64_t *d_n, void *d_workspace, uint64_t workspace_bytes, void *stream);
/* query <- query minus match (src/sourmash/search.py:915-919): sorted set difference */
void smgpu_subtract_raw(const uint64_t *d_a, uint64_t na, const uint64_t *d_b, uint64_t nb, uint64_t *d_out,
                        uint64_t *d_n, void *d_workspace, uint64_t workspace_bytes, void *stream);

/* ---- HyperLogLog extensions (csrc/hll.hip) ---- */
/* Hash the records queued by hll_add_sequence into the registers now (every reader does it anyway). */
void smgpu_hll_flush(SourmashHyperLogLog *ptr);
/* The 2^p registers (one byte each, owned by the handle, valid until its next change); *size = 2^p. */
const uint8_t *smgpu_hll_registers(const SourmashHyperLogLog *ptr, uintptr_t *size);
uint32_t smgpu_hll_precision(const SourmashHyperLogLog *ptr);
/* Every record of a FASTA / FASTQ file (plain or gzip) into the registers through the streaming ingest (force = true
 * semantics: bad k-mers are skipped).  *n_records (may be NULL) = records read; returns the bases read. */
uint64_t smgpu_hll_add_file(SourmashHyperLogLog *ptr, const char *path, uint64_t *n_records);
/* d_seq[0,len) already on the device (records separated by a byte outside ACGTacgt, e.g. '\n') into the registers;
 * `stream` is the stream that wrote d_seq.  Synchronises. */
void smgpu_hll_add_device(SourmashHyperLogLog *ptr, const uint8_t *d_seq, uint64_t len, void *stream);
/* The kernel alone: d_regs[2^p] (device u32, one per register) updated with every canonical k-mer hash != 0 (seed 42) of
 * d_seq[0,len); p in 4 .. 18.  Asynchronous on `stream`. */
void smgpu_hll_dna_raw(const uint8_t *d_seq, uint64_t len, uint32_t ksize, uint32_t p, uint32_t *d_regs, void *stream);

/* ---- Nodegraph extensions (csrc/nodegraph.hip) ---- */
/* The bulk k-mer calls take ksize 1 .. 32 and fold lower case to upper case; a bulk call on another ksize is an error.  The
 * tables and n_occupied after any mix of single and bulk calls equal what the same calls give one by one on the host. */
/* add_sequence: the records are queued and counted when the graph is next read (force = false: InvalidDNA naming the first
 * bad k-mer after the k-mers before it were counted; force = true: bad k-mers are skipped). */
void smgpu_nodegraph_add_sequence(SourmashNodegraph *ptr, const char *sequence, uintptr_t insize, bool force);
/* Count the queued records now (every reader does it anyway). */
void smgpu_nodegraph_flush(SourmashNodegraph *ptr);
/* Every record of a FASTA / FASTQ file (plain or gzip) through the streaming ingest (force = true semantics).  *n_records
 * (may be NULL) = records read; returns the bases read. */
uint64_t smgpu_nodegraph_add_file(SourmashNodegraph *ptr, const char *path, uint64_t *n_records);
/* d_seq[0,len) already on the device (records separated by any byte outside ACGTacgt); `stream` wrote d_seq.  Synchronises. */
void smgpu_nodegraph_add_device(SourmashNodegraph *ptr, const uint8_t *d_seq, uint64_t len, void *stream);
/* nodegraph_update_mh of every row of a SketchSet, in one launch over its resident CSR. */
void smgpu_nodegraph_update_sketchset(SourmashNodegraph *ptr, const SmgpuSketchSet *set);
/* out[r] = nodegraph_matches of row r of a SketchSet (out: one uint64_t per row). */
void smgpu_nodegraph_matches_sketchset(const SourmashNodegraph *ptr, const SmgpuSketchSet *set, uint64_t *out);
/* Summed intersections over summed unions of the zipped tables / summed intersections over this graph's set bits. */
double smgpu_nodegraph_similarity(const SourmashNodegraph *ptr, const SourmashNodegraph *optr);
double smgpu_nodegraph_containment(const SourmashNodegraph *ptr, const SourmashNodegraph *optr);
/* The table sizes nodegraph_with_tables(_, starting_size, n_tables) would make, without making the tables: the first
 * min(n, cap) into out; returns n. */
uintptr_t smgpu_nodegraph_table_sizes(uintptr_t starting_size, uintptr_t n_tables, uint64_t *out, uintptr_t cap);

/* ---- set algebra on resident collections: merge by group, intersect, subtract, downsample (csrc/setops.hip, csrc/setops_core.hpp) ----
 * Flat sets as `sig merge --flatten`, `sig intersect` and `sig subtract` work; what a set that carries abundances adds is said
 * under "abundance sets" below.  Every set-level entry returns a NEW set
 * (freed with smgpu_sketchset_free) with the receiver's parameters, host offsets and manifest rows; the receiver is unchanged.
 * geometry: lanes of a workgroup, the partner hashes the row-wise filter stages in LDS, and the row length above which the filter
 * splits a row over workgroups.  key_form: the pair form of the merge for a set of `max_hash` (0: num) merged into n_groups rows --
 * the bits of a hash and of a group number, and whether both share one 64-bit key.  Host only. */
void smgpu_setops_geometry(uint32_t *workgroup, uint32_t *lds_partner, uint64_t *split);
void smgpu_setops_key_form(uint64_t max_hash, uint64_t n_groups, uint32_t *hbits, uint32_t *gbits, uint32_t *packed);
/* The CSR in device memory (d_offsets: n + 1 positions in d_hashes spanning `total` hashes; rows ascending) merged into n_groups
 * rows: row g = the hashes that at least need-of-g rows of group g hold.  d_groups: one group number < n_groups per row (NULL:
 * all rows in group 0); d_need: one count per group (NULL: 1, the union), need_all != 0: the group's row count (the
 * intersection).  max_hash: of the sketches (0 for num sketches); num != 0: rows are cut to their num smallest hashes (union
 * only).  d_out_hashes: room for `total`; d_out_offsets: n_groups + 1; d_result: 2 x uint64_t ([0] the result's hashes, [1]
 * distinct (group, hash) pairs).  Returns the result's hashes.  Synchronises the stream.  UINT64_MAX with an error set: a refused
 * argument, or no device. */
uint64_t smgpu_setops_merge_workspace_bytes(uint64_t total, uint64_t n_groups);
uint64_t smgpu_setops_merge_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n, uint64_t total, const uint32_t *d_groups,
                                uint64_t n_groups, const uint32_t *d_need, uint32_t need_all, uint64_t max_hash, uint64_t num,
                                uint64_t *d_out_hashes, uint64_t *d_out_offsets, uint64_t *d_result, void *d_workspace,
                                uint64_t workspace_bytes, void *stream);
/* Row r of the result = the hashes of row r that are (keep_present != 0: intersect) or are not (0: subtract) in the other
 * sketch.  d_other_offsets NULL: one sketch d_other_hashes[0, other_len), ascending, against every row; otherwise a second CSR of
 * n rows, row r against row r (other_len is not read; the workspace takes other_len = 0).  grid: workgroups (0: the library's
 * number).  d_out_offsets: n + 1, always written; d_out_hashes: `capacity` hashes -- when the result is longer nothing is written
 * to it and the caller runs again with room.  d_result: 2 x uint64_t.  Returns the result's hashes.  Synchronises the stream. */
uint64_t smgpu_setops_filter_workspace_bytes(uint64_t n, uint64_t total, uint64_t other_len);
uint64_t smgpu_setops_filter_raw(const uint64_t *d_hashes, const uint64_t *d_offsets, uint64_t n, uint64_t total,
                                 const uint64_t *d_other_hashes, const uint64_t *d_other_offsets, uint64_t other_len,
                                 uint32_t keep_present, uint32_t grid, uint64_t *d_out_hashes, uint64_t capacity,
                                 uint64_t *d_out_offsets, uint64_t *d_result, void *d_workspace, uint64_t workspace_bytes, void *stream);
/* groups: one number < n_groups per row of the set (NULL: one group); need: one count per group (NULL: 1), need_all != 0: the
 * group's row count; names: NULL or one C string per group.  A num set takes the union only (MISMATCH_NUM otherwise). */
SmgpuSketchSet *smgpu_sketchset_merge_groups(const SmgpuSketchSet *set, const uint32_t *groups, uint64_t n_groups, const uint32_t *need,
                                             uint32_t need_all, const char *const *names);
/* other: a set of one row (against every row) or of as many rows as `set` (row by row); parameters must match in the
 * reference's order (ksize, hash function, scaled, seed).  Names and file names follow the receiver's rows. */
SmgpuSketchSet *smgpu_sketchset_filter(const SmgpuSketchSet *set, const SmgpuSketchSet *other, uint32_t keep_present);
SmgpuSketchSet *smgpu_sketchset_filter_sketch(const SmgpuSketchSet *set, const SourmashKmerMinHash *mh, uint32_t keep_present);
/* Every row cut to its hashes <= max_hash; a larger max_hash than the set's is CANNOT_UPSAMPLE_SCALED. */
SmgpuSketchSet *smgpu_sketchset_downsample(const SmgpuSketchSet *set, uint64_t max_hash);

/* ---- abundance sets: a resident collection with a u64 abundance column aligned with its hashes (csrc/capi_abund_set.cpp,
 * csrc/abund_set.hip, and the value-moving forms of csrc/setops.hip).  Every stored abundance is at least 1.  Every entry that
 * reads hashes and offsets only (compare, overlaps, search, gather, the many-query entries, Nodegraph, find, md5sums) sees an
 * abundance set as its flattened self.  subset, downsample and smgpu_sketchset_filter* carry the receiver's abundances with the
 * kept hashes (the other side's stay ignored); smgpu_sketchset_merge_groups sums them per kept hash (wrapping u64);
 * smgpu_sketchset_get gives abundance sketches; smgpu_sketchset_to_json and smgpu_sigwriter_add refuse the set.
 * new_abund: every sketch must track abundance (NEEDS_ABUNDANCE_TRACKING) and share parameters (the reference's mismatch errors).
 * from_csr_abund: smgpu_sketchset_from_csr with d_abunds aligned with d_hashes; a 0 in it is refused with the first such position. */
SmgpuSketchSet *smgpu_sketchset_new_abund(const SourmashKmerMinHash *const *mhs, uintptr_t n);
SmgpuSketchSet *smgpu_sketchset_from_csr_abund(const uint64_t *d_hashes, const uint64_t *d_abunds, const uint64_t *d_offsets, uint64_t n,
                                               uint32_t ksize, uint32_t hash_function, uint64_t seed, uint64_t max_hash, uint64_t num,
                                               const char *const *names, const char *const *filenames);
/* smgpu_sketchset_sketch_records / _sketch_file / _sketch_residue_records / _sketch_residue_file with track_abundance != 0: the
 * result is an abundance set, a kept hash's abundance the number of times the record holds it (both strands counted as one
 * k-mer, as add_sequence counts); manifest rows say with_abundance = 1.  track_abundance = 0: the flat entries themselves. */
SmgpuSketchSet *smgpu_sketchset_sketch_records_abund(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, uint64_t n_records,
                                                     uint32_t ksize, uint64_t seed, uint64_t scaled, uint32_t track_abundance);
SmgpuSketchSet *smgpu_sketchset_sketch_file_abund(const char *path, uint32_t ksize, uint64_t seed, uint64_t scaled, uint32_t track_abundance);
SmgpuSketchSet *smgpu_sketchset_sketch_residue_records_abund(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, const uint64_t *d_ends,
                                                             uint64_t n_records, uint32_t ksize, uint32_t hash_function, int32_t translate,
                                                             uint64_t seed, uint64_t scaled, uint32_t track_abundance);
SmgpuSketchSet *smgpu_sketchset_sketch_residue_file_abund(const char *path, uint32_t ksize, uint32_t hash_function, int32_t translate,
                                                          uint64_t seed, uint64_t scaled, uint32_t track_abundance);
/* 1 for an abundance set; the largest stored abundance (a bound after a filter; UINT64_MAX after a summing merge). */
uint32_t smgpu_sketchset_track_abundance(const SmgpuSketchSet *set);
uint64_t smgpu_sketchset_abund_max(const SmgpuSketchSet *set);
/* The column where it lies, borrowed: valid while the set lives; NULL for a flat set. */
void smgpu_sketchset_device_abunds(const SmgpuSketchSet *set, const uint64_t **d_abunds);
/* out[r] = the sum of row r's abundances, wrapping u64 (MinHash.sum_abundances), computed on the device. */
void smgpu_sketchset_abund_sums(const SmgpuSketchSet *set, uint64_t *out);
/* A flat copy (device-to-device); manifest rows say with_abundance = 0. */
SmgpuSketchSet *smgpu_sketchset_flatten(const SmgpuSketchSet *set);
/* sig inflate: `set` is flat, `other` carries abundance (one row against every row, or as many rows as `set`, row by row; or one
 * sketch).  A hash is kept when the other side holds it and takes the other side's abundance.  Parameters as for
 * smgpu_sketchset_filter. */
SmgpuSketchSet *smgpu_sketchset_inflate(const SmgpuSketchSet *set, const SmgpuSketchSet *other);
SmgpuSketchSet *smgpu_sketchset_inflate_sketch(const SmgpuSketchSet *set, const SourmashKmerMinHash *mh);
/* sig filter: the hashes whose abundance a satisfies min_abundance <= a <= max_abundance (UINT64_MAX: no upper bound), with
 * their abundances.  A flat set is NEEDS_ABUNDANCE_TRACKING. */
SmgpuSketchSet *smgpu_sketchset_filter_abund(const SmgpuSketchSet *set, uint64_t min_abundance, uint64_t max_abundance);
/* smgpu_sketchset_merge_groups with count_rows != 0: `set` is flat and the result carries, as abundance, the number of rows of
 * the group that hold the hash.  count_rows = 0: smgpu_sketchset_merge_groups itself. */
SmgpuSketchSet *smgpu_sketchset_merge_groups_values(const SmgpuSketchSet *set, const uint32_t *groups, uint64_t n_groups, const uint32_t *need,
                                                    uint32_t need_all, const char *const *names, uint32_t count_rows);
/* sims_out: n x n doubles, the angular similarity of every pair of rows (smgpu_compare_abund_raw_n on the set's own buffers,
 * narrow when every abundance is below 2^32, then smgpu_host_angular_f64).  A flat set is NEEDS_ABUNDANCE_TRACKING. */
void smgpu_sketchset_compare_angular(const SmgpuSketchSet *set, double *sims_out);
/* smgpu_sketchset_gather_rows_many; use_resident != 0: `queries` is an abundance set and its own column is the pass's
 * abundances (abunds must be NULL): no host array, no upload. */
SmgpuGatherRows *smgpu_sketchset_gather_rows_many_resident(const SmgpuSketchSet *db, const SmgpuSketchSet *queries, const uint64_t *abunds,
                                                           uint64_t threshold_hashes, uint32_t use_resident);
/* The value-moving forms on caller-owned buffers.  filter: smgpu_setops_filter_raw (its workspace function serves) with `values`:
 * 0 flat; 1 carry -- d_abunds is aligned with d_hashes and a kept hash keeps its own; 2 take -- d_other_abunds is aligned with
 * d_other_hashes, keep_present is 1, a kept hash takes the other's at the found position; 3 range -- no other sketch, a hash is
 * kept when range_lo <= its abundance <= range_hi.  d_out_abunds: `capacity` values beside d_out_hashes.
 * merge: smgpu_setops_merge_raw with `values`: 0 flat; 1 sum -- d_out_abunds gets the wrapping u64 sum of the abundances of the
 * group's rows that hold the hash; 2 count -- their number (d_abunds is not read).  With values the workspace is
 * smgpu_setops_merge_values_workspace_bytes'. */
uint64_t smgpu_setops_filter_values_raw(const uint64_t *d_hashes, const uint64_t *d_abunds, const uint64_t *d_offsets, uint64_t n, uint64_t total,
                                        const uint64_t *d_other_hashes, const uint64_t *d_other_abunds, const uint64_t *d_other_offsets,
                                        uint64_t other_len, uint32_t keep_present, uint32_t values, uint64_t range_lo, uint64_t range_hi,
                                        uint32_t grid, uint64_t *d_out_hashes, uint64_t *d_out_abunds, uint64_t capacity,
                                        uint64_t *d_out_offsets, uint64_t *d_result, void *d_workspace, uint64_t workspace_bytes, void *stream);
uint64_t smgpu_setops_merge_values_workspace_bytes(uint64_t total, uint64_t n_groups);
uint64_t smgpu_setops_merge_values_raw(const uint64_t *d_hashes, const uint64_t *d_abunds, const uint64_t *d_offsets, uint64_t n, uint64_t total,
                                       const uint32_t *d_groups, uint64_t n_groups, const uint32_t *d_need, uint32_t need_all,
                                       uint64_t max_hash, uint64_t num, uint32_t values, uint64_t *d_out_hashes, uint64_t *d_out_abunds,
                                       uint64_t *d_out_offsets, uint64_t *d_result, void *d_workspace, uint64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SOURMASH_AMD_H_INCLUDED */
