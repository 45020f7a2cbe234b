// Internal C++ interface between the HIP translation units and the C-ABI layer.
// Everything here takes raw device pointers and a stream; what a launch needs besides comes from the arena in stream order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "find_core.hpp"
#include "qindex_core.hpp"

namespace smg {

// x rounded up to the 256-byte granule the workspaces are carved in
inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }
// workgroups for n items at `per` items each: at least one, at most `cap` (the kernels stride over the rest)
inline unsigned grid_for(uint64_t n, unsigned per, unsigned cap) {
    const uint64_t b = (n + per - 1) / per;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- sketch.hip ---------------------------------------------------------------
// Append every hash h of a canonical DNA k-mer of d_seq[0,len) with 1 <= h <= thr
// to d_out (unordered, duplicates kept); *d_count += number appended (keeps
// counting past `cap`, entries past cap are dropped).  d_seq may have any alignment
// (an unaligned start costs nothing: the kernel realigns and blanks the prefix).  Any byte outside ACGTacgt kills the k-mers covering it.
hipError_t sketch_dna_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, uint64_t seed, uint64_t thr,
                             uint64_t* d_out, unsigned long long* d_count, uint64_t cap, hipStream_t stream);
// The same with `grid` workgroups exactly (0: the launcher's own number) where k <= 88; longer k-mers take their own kernel's grid.
hipError_t sketch_dna_launch_grid(const uint8_t* d_seq, uint64_t len, uint32_t k, uint64_t seed, uint64_t thr,
                                  uint64_t* d_out, unsigned long long* d_count, uint64_t cap, uint32_t grid, hipStream_t stream);
// d_out[i] = hash of the canonical k-mer starting at i for i in [0, n_kmers) (0 for k-mers
// covering a byte outside ACGTacgt).  d_out must be zeroed by the caller.
// k-mers longer than the register-window kernel holds (sketch_words.hip): k = 129 .. sketch_dna_max_k(), any k >= 16 accepted
// several ksizes of one stretch in one pass (sketch_multi.hip): the standard ksize sets only
struct SketchMultiOut { uint64_t thr; uint64_t* out; unsigned long long* count; uint64_t cap; };
bool sketch_dna_multi_supported(const uint32_t* ks, int n);
hipError_t sketch_dna_multi_launch(const uint8_t* d_new, uint64_t n_new, const uint32_t* ks, int n, uint64_t seed, const SketchMultiOut* outs,
                                   hipStream_t stream);
hipError_t sketch_dna_words_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, uint64_t seed, uint64_t thr, uint64_t* d_out,
                                   unsigned long long* d_count, uint64_t cap, bool dense, hipStream_t stream);
uint32_t sketch_dna_max_k();
hipError_t kmer_hashes_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, uint64_t seed, uint64_t* d_out,
                              uint64_t n_kmers, hipStream_t stream);
// *d_first = min(*d_first, position of the first byte outside ACGTacgt)
hipError_t first_invalid_launch(const uint8_t* d_seq, uint64_t len, unsigned long long* d_first, hipStream_t stream);

// ---- hll.hip (HyperLogLog registers: one u32 per register, 2^p of them, p in 4 .. 18) ------------------
// every canonical DNA k-mer hash h != 0 (seed 42) of d_seq[0,len): d_regs[h & (2^p-1)] = max(.., clz64(h >> p) + 1 - p).
// Any alignment; bytes outside ACGTacgt kill the k-mers covering them.  k > 88 takes scratch from the library's arena.
hipError_t hll_dna_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, uint32_t p, uint32_t* d_regs, hipStream_t stream);
// the same update for every hash of d_hashes[0,n) (skip_zero: hashes equal to 0 are left out)
hipError_t hll_hashes_launch(const uint64_t* d_hashes, uint64_t n, uint32_t p, uint32_t* d_regs, bool skip_zero, hipStream_t stream);
// d_out[i] = (uint8_t)d_regs[i]
hipError_t hll_pack_launch(const uint32_t* d_regs, uint32_t n, uint8_t* d_out, hipStream_t stream);

// ---- nodegraph.hip (Bloom filter tables: one u32 word array, fixedbitset layout) ----------------------------------------
// table t: `size` bits from word `off` of the array; magic = ng_magic(size) (nodegraph_core.hpp)
struct NgTable { uint64_t size, magic, off; };
// a graph's device mirror: tabs[n_tables] and words[n_words] on the device, t0_words = table 0's words (it starts at word 0),
// *occ += table-0 bits turned from 0 to 1
struct NgDev {
    const NgTable* tabs = nullptr;
    uint32_t n_tables = 0;
    uint32_t* words = nullptr;
    uint64_t n_words = 0;
    uint64_t t0_words = 0;
    unsigned long long* occ = nullptr;
};
// every k-mer (1 <= k <= 32) of d_seq[0,len) whose bytes are all in ACGTacgt sets bit min(fwd, rev two-bit word) mod size of
// every table.  Any alignment.  Asynchronous on `stream`.
hipError_t nodegraph_dna_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, const NgDev& g, hipStream_t stream);
// every hash of d_hashes[0,n) sets its bits
hipError_t nodegraph_hashes_launch(const uint64_t* d_hashes, uint64_t n, const NgDev& g, hipStream_t stream);
// d_out[r] = hashes of CSR row r (d_hashes[d_offsets[r] .. d_offsets[r+1])) found in every table (read-only)
hipError_t nodegraph_matches_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n_rows, const NgDev& g,
                                    uint64_t* d_out, hipStream_t stream);

// ---- protein.hip (protein / dayhoff / hp sketches) ---------------------------------------------
// d_aa[i] = alphabet(upper(d_seq[i]))  (hash_function 2 protein, 3 dayhoff, 4 hp)
hipError_t residues_launch(const uint8_t* d_seq, uint64_t len, uint32_t hash_function, uint8_t* d_aa, hipStream_t stream);
// six-frame translation of DNA: segments frame0 fwd, frame0 rc, frame1 fwd, ... each followed by a 0xFF separator;
// d_aa must hold translated_bytes(len) bytes
uint64_t translated_bytes(uint64_t len);
hipError_t translate_launch(const uint8_t* d_seq, uint64_t len, uint32_t hash_function, uint8_t* d_aa, hipStream_t stream);
// hashes of the windows of k residues that do not touch a separator: appended (1 <= h <= thr; *d_count += n) or,
// dense, d_out[i] = hash of the window starting at i (d_out pre-zeroed, cap = number of entries)
hipError_t residue_windows_launch(const uint8_t* d_aa, uint64_t n, uint32_t k, uint64_t seed, uint64_t thr, uint64_t* d_out,
                                  unsigned long long* d_count, uint64_t cap, bool dense, hipStream_t stream);

// ---- device_sort.hip ------------------------------------------------------------
size_t sort_unique_temp_bytes(uint64_t n);
// many small lists sorted as one (device_sort.hip): dst[seg.dst + i] = src[seg.src + i] | (list number << hbits)
struct TagSegment { uint64_t src, dst, n; };
hipError_t tag_gather_launch(const uint64_t* d_src, const TagSegment* d_segs, uint32_t n_segs, uint64_t* d_dst, int hbits, hipStream_t stream);
// keys[0,n) -> sorted unique in out[0,*d_n_out); if d_counts != nullptr also the
// multiplicity of every unique key.  keys is clobbered.  `bits` = significant key bits.
hipError_t sort_unique(uint64_t* d_keys, uint64_t n, uint64_t* d_out, uint64_t* d_counts, uint64_t* d_n_out,
                       void* d_temp, size_t temp_bytes, int bits, hipStream_t stream);

// ---- uniform_sort.hip (uniform_sort_core.hpp: the plan and its rules) ---------------------------------------------------------------
// The same result for keys that are uniform on [0, thr], without a size on the host: d_keys[0, min(*d_n, n_max)) -> sorted unique
// in d_out[0, *d_n_out), multiplicities in d_counts (may be null).  Grids come from n_max; nothing synchronises; d_keys is not
// modified.  *d_fellback = 0 when the result stands, 1 when the keys did not spread as planned (or the plan declines n_max / thr /
// temp_bytes): then nothing else is valid and the caller runs sort_unique on the untouched d_keys.
hipError_t sort_unique_uniform(const uint64_t* d_keys, const unsigned long long* d_n, uint64_t n_max, uint64_t thr, uint64_t* d_out,
                               uint64_t* d_counts, uint64_t* d_n_out, uint32_t* d_fellback, void* d_temp, size_t temp_bytes,
                               hipStream_t stream);
// workspace of that call; and a bound of it over every thr
size_t sort_unique_uniform_temp_bytes(uint64_t n_max, uint64_t thr, bool counts);
size_t sort_unique_uniform_temp_bound(uint64_t n_max, bool counts);
// the form the call takes (UsForm: 0 declines, 1 one workgroup, 2 / 3 one / two scatter passes)
uint32_t sort_unique_uniform_form(uint64_t n_max, uint64_t thr, size_t temp_bytes, bool counts);
// d_report[0 .. 3) = {*d_n, *d_n_out, *d_fellback}: what the host wants to know of such a call, in one place for one copy
hipError_t sort_report_launch(const unsigned long long* d_n, const uint64_t* d_n_out, const uint32_t* d_fellback, uint64_t* d_report,
                              hipStream_t stream);

// (key, value) pairs sorted by the low `bits` bits of the key (stable), and runs of equal (a, b) pairs with their lengths
size_t sort_pairs_temp_bytes(uint64_t n);
hipError_t sort_pairs(const uint64_t* d_keys_in, uint64_t* d_keys_out, const uint64_t* d_vals_in, uint64_t* d_vals_out, uint64_t n,
                      int bits, void* d_temp, size_t temp_bytes, hipStream_t stream, int begin_bit = 0);     // (orders by bits [begin_bit, begin_bit + bits))
size_t rle_pairs_temp_bytes(uint64_t n);
hipError_t rle_pairs(const uint64_t* d_a, const uint64_t* d_b, uint64_t n, uint64_t* d_out_a, uint64_t* d_out_b, uint64_t* d_counts,
                     uint64_t* d_n_out, void* d_temp, size_t temp_bytes, hipStream_t stream);

// ---- sketch_records.hip (one sketch per record of a buffer: CSR rows) -----------------------------------------------------
// Every hash h of a canonical DNA k-mer (1 <= k <= 88) of d_seq[0,len) with 1 <= h <= thr appended to d_hash, the position of the
// k-mer's first byte to d_pos (unordered); *d_count += pairs (keeps counting past `cap`, pairs past cap are dropped).
hipError_t records_pairs_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, uint64_t seed, uint64_t thr, uint64_t* d_hash,
                                uint64_t* d_pos, unsigned long long* d_count, uint64_t cap, hipStream_t stream);
// *d_bad |= 1 if d_starts[0 .. n_records] is not ascending, |= 2 if d_starts[n_records] > len
hipError_t records_check_starts_launch(const uint64_t* d_starts, uint64_t n_records, uint64_t len, unsigned long long* d_bad,
                                       hipStream_t stream);
size_t records_csr_temp_bytes(uint64_t n_pairs);
// n_pairs (hash, position) pairs -> the CSR of the records d_starts describes (records_core.hpp: rec_assign): row r = sorted
// distinct hashes of the k-mers inside record r, d_abunds (may be null) their multiplicities, d_offsets[0 .. n_records],
// *d_n_out = entries.  The pair arrays are clobbered.  Asynchronous: no size is read back.
hipError_t records_csr_launch(uint64_t* d_pair_hash, uint64_t* d_pair_pos, uint64_t n_pairs, const uint64_t* d_starts, uint64_t n_records,
                              uint32_t k, uint64_t max_hash, uint64_t* d_hashes, uint64_t* d_abunds, uint64_t* d_offsets, uint64_t* d_n_out,
                              void* d_temp, size_t temp_bytes, hipStream_t stream);

// the same for records with explicit ends (records_core.hpp: rec_assign_ends): record r = [d_starts[r], d_ends[r]), d_ends null
// = records touch.  `k` and the positions are in the units of the buffer the pairs came from (residues for the residue passes).
hipError_t records_csr_ends_launch(uint64_t* d_pair_hash, uint64_t* d_pair_pos, uint64_t n_pairs, const uint64_t* d_starts, const uint64_t* d_ends,
                                   uint64_t n_records, uint32_t k, uint64_t max_hash, uint64_t* d_hashes, uint64_t* d_abunds, uint64_t* d_offsets,
                                   uint64_t* d_n_out, void* d_temp, size_t temp_bytes, hipStream_t stream);
// *d_bad |= 4 if some d_ends[r] lies outside [d_starts[r], d_starts[r + 1]] (the starts are checked by records_check_starts_launch)
hipError_t records_check_ends_launch(const uint64_t* d_starts, const uint64_t* d_ends, uint64_t n_records, unsigned long long* d_bad,
                                     hipStream_t stream);
// the ends of a parsed file's records: d_ends[r] = d_starts[r + 1] - 1, the header byte fastx.hip keeps, for every record but the last
hipError_t records_file_ends_launch(const uint64_t* d_starts, uint64_t n_records, uint64_t* d_ends, hipStream_t stream);

// ---- protein_records.hip (one protein / dayhoff / hp sketch per record: the residue side of sketch_records.hip) -------------------
// Every hash h of a window of k residues (1 <= k <= 79) of d_aa, with 1 <= h <= thr, appended to d_hash and the window's start to
// d_pos (unordered); *d_count += pairs (keeps counting past `cap`, pairs past cap are dropped).  d_aa: 8-byte aligned, readable
// in whole 8-byte words.  d_n not null: the translated buffer -- its size is *d_n (a size only the device knows), never above
// n_bound, and windows touching a 0xFF do not exist.  d_n null: residues of protein input, n_bound of them, no separators.
hipError_t residue_pairs_launch(const uint8_t* d_aa, uint64_t n_bound, const uint64_t* d_n, uint32_t k, uint64_t seed, uint64_t thr,
                                uint64_t* d_hash, uint64_t* d_pos, unsigned long long* d_count, uint64_t cap, hipStream_t stream);
// Six-frame translation of every record [d_starts[r], d_ends[r]) (d_ends null: records touch) of d_seq[0,len) into a block of its
// own of d_aa (translate_records_core.hpp): d_block_starts[0 .. n_records] the blocks' starts, the last one the bytes written.
// d_aa: 8-byte aligned, room for translated_records_bytes_bound(len, n_records) + 8 bytes.  The records must have been checked.
uint64_t translated_records_bytes_bound(uint64_t len, uint64_t n_records);
size_t translate_records_temp_bytes(uint64_t n_records);
hipError_t translate_records_launch(const uint8_t* d_seq, uint64_t len, const uint64_t* d_starts, const uint64_t* d_ends, uint64_t n_records,
                                    uint32_t hash_function, uint64_t* d_block_starts, uint8_t* d_aa, void* d_temp, size_t temp_bytes,
                                    hipStream_t stream);

// ---- sketch_find.hip (a query sketch's k-mers in a buffer: rows of (position, hash), by record) ----------------------------------
// d_dir[b] = first index of the sorted d_q[0,n) with d_q[i] >> shift >= b, for b = 0 .. n_buckets (find_core.hpp)
hipError_t find_dir_launch(const uint64_t* d_q, uint64_t n, uint32_t shift, uint64_t n_buckets, uint32_t* d_dir, hipStream_t stream);
// Every k-mer (1 <= k <= 88) of d_seq[0,len) whose canonical hash is a member of the query: the hash appended to d_hash, the
// position of the k-mer's first byte to d_pos (unordered); *d_count += pairs (keeps counting past `cap`, pairs past cap are
// dropped).  grid: 0, the launcher's own number of workgroups, or exactly that many.
hipError_t find_pairs_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, uint64_t seed, const FindQuery& query, uint64_t* d_hash,
                             uint64_t* d_pos, unsigned long long* d_count, uint64_t cap, uint32_t grid, hipStream_t stream);
size_t find_rows_temp_bytes(uint64_t n_pairs);
// n_pairs matched (hash, position) pairs -> rows ordered by position, without the pairs whose k-mer lies in no record
// (records_core.hpp: rec_assign): d_positions / d_hashes (room for n_pairs), d_kmers (may be null; n_pairs * k bytes) the k-mers'
// upper-cased text, d_offsets[0 .. n_records] the first row of every record, *d_n_out = rows.  The pair arrays are clobbered.
// Asynchronous: no size is read back.
hipError_t find_rows_launch(const uint8_t* d_seq, uint64_t len, uint64_t* d_pair_hash, uint64_t* d_pair_pos, uint64_t n_pairs,
                            const uint64_t* d_starts, uint64_t n_records, uint32_t k, uint64_t* d_positions, uint64_t* d_hashes,
                            uint8_t* d_kmers, uint64_t* d_offsets, uint64_t* d_n_out, void* d_temp, size_t temp_bytes, hipStream_t stream);

// ---- overlap_many.hip (m queries against every row of a CSR collection in one pass; many_core.hpp holds its rules) -------------
// Both CSRs on the device: the queries (m rows, q_total hashes in all) and the collection (n_rows rows).  d_need[q] >= 1: the count
// a pair of query q must reach to be reported; cutoff: only hashes <= cutoff count (rows are ascending and end there).  q_block:
// queries counted per pass over the collection (0: MANY_Q_BLOCK); grid: workgroups of the pass (0: the launcher's own number).
// The hits (query, row, count) leave in d_queries / d_rows / d_common, at most `capacity` of them, ordered by (query, row);
// d_result (4 x u64): [0] the true number of hits, [1] distinct query hashes <= cutoff, [2] passes over the collection.
struct ManyArgs {
    const uint64_t *d_qhashes, *d_qoffsets;
    uint64_t m, q_total;
    const uint64_t *d_hashes, *d_offsets;
    uint64_t n_rows;
    const uint32_t* d_need;
    uint64_t cutoff;
    uint32_t q_block, grid;
    uint32_t *d_queries, *d_rows, *d_common;
    uint64_t capacity;
    uint64_t* d_result;
    void* d_workspace;
    uint64_t workspace_bytes;
};
size_t many_overlap_workspace_bytes(uint64_t m, uint64_t q_total, uint64_t capacity);
uint32_t many_overlap_passes(uint64_t m, uint32_t q_block);
// Synchronises the stream (the index geometry and the hit count are read back).  *hits = d_result[0]; when it exceeds the capacity
// the first `capacity` hits found stand unordered in the arrays and nothing lies behind them.  ms3 (may be null): milliseconds of
// the index build, the passes, and the final sort.
hipError_t many_overlap_run(const ManyArgs& args, uint64_t* hits, float* ms3, hipStream_t stream);
// d_sizes[r] = hashes of row r that are <= cutoff (a set's sizes at the common scaled)
hipError_t many_sizes_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint64_t n, uint64_t cutoff, uint64_t* d_sizes, hipStream_t stream);

// ---- gather_many.hip (the min-set-cover loop for many small queries, one workgroup a query; gather_many_core.hpp holds its rules) ----
// The queries [q_base, q_base + m) of a call: d_qoffsets points at THEIR m + 1 offsets (into d_qhashes), the hits are those of
// many_overlap_run for them -- ordered by (query, row), query numbers starting at q_base -- and d_out_rounds / d_status have one
// entry per query of the range.  The picks of a query go to the slots of its own hits in d_out_rows / d_out_isect, in rank order:
// [its first hit, + d_out_rounds[q]).  d_status[q] = 1: the query is beyond a cap and nothing was written for it.  Caps of 0 mean
// the defaults; grid: workgroups of the fill and the rounds (0: the launcher's own numbers).
struct GatherManyArgs {
    const uint64_t *d_qhashes, *d_qoffsets;
    uint64_t m;
    uint32_t q_base;
    const uint64_t *d_hashes, *d_offsets;
    uint64_t n_rows;
    const uint32_t *d_hit_queries, *d_hit_rows, *d_hit_common;
    uint64_t n_hits;
    uint64_t cutoff, threshold_hashes;
    uint32_t max_query_hashes, max_candidates, grid;
    uint32_t *d_out_rows, *d_out_isect, *d_out_rounds, *d_status;
    void* d_workspace;
    uint64_t workspace_bytes;
};
// what a run can find wrong with its input beside a HIP error: the forward CSR did not come out as long as the hits' common counts
// say (the hits are not those of these sets), 2^32 entries or more, or a workspace smaller than the entries need
enum GatherManyTrouble : uint32_t { GM_OK = 0, GM_FILL_MISMATCH = 1, GM_TOO_MANY_ENTRIES = 2, GM_WORKSPACE_TOO_SMALL = 3 };
// total_common: the sum of the hits' common counts over the queries within the caps (the entries of the forward CSR)
size_t gather_many_workspace_bytes(uint64_t m, uint64_t n_hits, uint64_t total_common);
// Synchronises the stream.  *total_rounds = picks of all queries that ran; ms3 (may be null): milliseconds of the fill (with the
// scan in front of it), the sort, and the rounds.  hipErrorInvalidValue: an argument smgpu_gather_many_raw refuses.
hipError_t gather_many_run(const GatherManyArgs& args, uint64_t* total_rounds, uint32_t* trouble, float* ms3, hipStream_t stream);
// Per query of a whole call (q_base = 0): d_qlo[0 .. m] its first hit, d_qn its hashes <= cutoff, d_status as above, d_sums the sum
// of common over its hits.  Asynchronous.
hipError_t gather_many_plan(const uint64_t* d_qhashes, const uint64_t* d_qoffsets, uint64_t m, const uint32_t* d_hit_queries,
                            const uint32_t* d_hit_common, uint64_t n_hits, uint64_t cutoff, uint32_t max_query_hashes, uint32_t max_candidates,
                            uint32_t* d_qlo, uint32_t* d_qn, uint32_t* d_status, uint64_t* d_sums, hipStream_t stream);

// ---- gather_rows.hip (from the picks of gather to the integers of its result rows; gather_rows_core.hpp holds its rules) ----------
// Both CSRs on the device; d_qoffsets (m + 1) are positions in d_qhashes[0, q_total), d_qabunds (may be null: every abundance is 1)
// is aligned with d_qhashes.  The picks of query q are d_pick_rows[d_pick_offsets[q], d_pick_offsets[q + 1]) in rank order.
// Outputs: d_owner (q_total: the rank that owns the hash, or GM_NONE), d_orig_common / d_unique / d_weighted (n_picks),
// d_abund_offsets (n_picks + 1), d_abund_values (room for q_total), d_query_sizes / d_total_weighted (m).
struct GatherRowsArgs {
    const uint64_t *d_qhashes, *d_qabunds, *d_qoffsets;
    uint64_t m, q_total;
    const uint64_t *d_hashes, *d_offsets;
    uint64_t n_rows;
    const uint64_t* d_pick_offsets;
    const uint32_t* d_pick_rows;
    uint64_t n_picks;
    uint64_t cutoff;
    uint32_t grid;
    uint32_t *d_owner, *d_orig_common, *d_unique;
    uint64_t *d_weighted, *d_abund_offsets, *d_abund_values, *d_query_sizes, *d_total_weighted;
    void* d_workspace;
    uint64_t workspace_bytes;
};
size_t gather_rows_workspace_bytes(uint64_t m, uint64_t q_total, uint64_t n_picks);
// Synchronises the stream.  *n_owned = query hashes that a pick owns (the entries of d_abund_values); *trouble: 0, or the bits of
// gather_rows_core.hpp (GR_BAD_*) -- then the outputs hold nothing; ms3 (may be null): milliseconds of the owner pass, the tally
// pass and the pair sort.  hipErrorInvalidValue: an argument smgpu_gather_rows_raw refuses.
hipError_t gather_rows_run(const GatherRowsArgs& args, uint64_t* n_owned, uint32_t* trouble, float* ms3, hipStream_t stream);

// ---- setops.hip (set algebra on a CSR collection: merge by group, intersect, subtract; setops_core.hpp holds its rules) -----------
// Merge: the CSR of n rows (d_offsets: n + 1 positions in d_hashes, `total` hashes between the first and the last) -> a CSR of
// n_groups rows, row g = the hashes that at least need-of-g rows of group g hold, ascending.  d_groups: the group of every row,
// < n_groups (null: every row in group 0); d_need: one count per group (null: 1), or with need_all != 0 the group's row count.
// max_hash: of the set (0 for num sets; it chooses the key form); num != 0: every result row is cut to its num smallest.
// d_out_hashes: room for `total`; d_out_offsets: n_groups + 1; d_result (2 x u64): [0] hashes of the result, [1] distinct
// (group, hash) pairs.
struct SetopsMergeArgs {
    const uint64_t *d_hashes, *d_offsets;
    uint64_t n, total;
    const uint32_t* d_groups;
    uint64_t n_groups;
    const uint32_t* d_need;
    uint32_t need_all;
    uint64_t max_hash, num;
    uint64_t *d_out_hashes, *d_out_offsets, *d_result;
    void* d_workspace;
    uint64_t workspace_bytes;
    // values (setops_core.hpp: SetopsMergeValues).  SUM: d_abunds is aligned with d_hashes and d_out_abunds (room for `total`)
    // gets, beside every kept hash, the wrapping u64 sum of the abundances of the group's rows that hold it; COUNT: d_out_abunds
    // gets the number of those rows and d_abunds is not read.  The workspace is setops_merge_values_workspace_bytes' then.
    uint32_t values = 0;
    const uint64_t* d_abunds = nullptr;
    uint64_t* d_out_abunds = nullptr;
};
size_t setops_merge_workspace_bytes(uint64_t total, uint64_t n_groups);
size_t setops_merge_values_workspace_bytes(uint64_t total, uint64_t n_groups);
// Synchronises the stream.  hipErrorInvalidValue: an argument smgpu_setops_merge_raw refuses.
hipError_t setops_merge_run(const SetopsMergeArgs& args, uint64_t* total_out, hipStream_t stream);
// Filter: row r of the result = the hashes of row r that are (keep_present != 0) or are not members of the other sketch.
// d_other_offsets null: ONE sketch, d_other_hashes[0, other_len) ascending, for every row (looked up through a query index built by
// the call); otherwise the second set's CSR, n rows, row r for row r.  grid: workgroups (0: the launcher's own number).
// d_out_offsets: n + 1; d_result (2 x u64): [0] hashes of the result, [1] the trouble word of the write.
struct SetopsFilterArgs {
    const uint64_t *d_hashes, *d_offsets;
    uint64_t n, total;
    const uint64_t *d_other_hashes, *d_other_offsets;
    uint64_t other_len;
    uint32_t keep_present, grid;
    uint64_t *d_out_offsets, *d_result;
    void* d_workspace;
    uint64_t workspace_bytes;
    // values (setops_core.hpp: SetopsValueMode).  CARRY / RANGE: d_abunds is aligned with d_hashes; TAKE: d_other_abunds is aligned
    // with d_other_hashes and keep_present is 1; RANGE: no other sketch, a hash is kept when range_lo <= its abundance <= range_hi.
    uint32_t values = 0;
    const uint64_t *d_abunds = nullptr, *d_other_abunds = nullptr;
    uint64_t range_lo = 0, range_hi = ~0ull;
};
// what the count leaves for the write (the workspace keeps the rest)
struct SetopsFilterState {
    QIndex qi;
    uint64_t other_max = 0, total = 0;
    bool counted = false;
};
size_t setops_filter_workspace_bytes(uint64_t n, uint64_t total, uint64_t other_len);
// The two modes of the one kernel, with the scan of the counts between them.  The count writes d_out_offsets and reads the total
// back (it synchronises the stream), so that the caller can make room; the write puts the kept hashes into d_out_hashes (room for
// `capacity` >= the total) and synchronises.  *trouble: setops_core.hpp's SetopsTrouble -- then the output holds nothing of use.
// With values, d_out_abunds (the same capacity) gets every kept hash's value at the same position.
hipError_t setops_filter_count(const SetopsFilterArgs& args, SetopsFilterState& state, uint64_t* total_out, hipStream_t stream);
hipError_t setops_filter_write(const SetopsFilterArgs& args, const SetopsFilterState& state, uint64_t* d_out_hashes, uint64_t capacity,
                               uint32_t* trouble, hipStream_t stream, uint64_t* d_out_abunds = nullptr);

// ---- abund_set.hip (the abundance column of a resident collection) ------------------------------------------------------------
// d_result (2 x u64): [0] the largest of d_abunds[0, total), [1] the first position of a 0 (2^64 - 1: none).  Does not synchronise.
hipError_t abund_check_launch(const uint64_t* d_abunds, uint64_t total, uint64_t* d_result, hipStream_t stream);
// d_sums[r] = the wrapping u64 sum of d_abunds[d_offsets[r], d_offsets[r + 1])
hipError_t abund_row_sums_launch(const uint64_t* d_abunds, const uint64_t* d_offsets, uint64_t n, uint64_t* d_sums, hipStream_t stream);

// ---- synth.hip --------------------------------------------------------------------
hipError_t synth_dna_launch(uint8_t* d_out, uint64_t start, uint64_t n, uint64_t seed, uint64_t record_len,
                            hipStream_t stream);

// ---- compare.hip ------------------------------------------------------------------
// CSR of sorted unique u64 rows on device -> common[i][j] for i in [row_lo,row_hi), all j.
hipError_t compare_counts_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n,
                                 uint32_t row_lo, uint32_t row_hi, uint32_t* d_common /*[(row_hi-row_lo)][n]*/,
                                 hipStream_t stream);
// Sharded all-pairs: row tiles (16 rows each) rb_first, rb_first + rb_stride, ... of the n x n problem,
// upper-triangle tiles only; d_common holds the owned tiles back to back ([rb_count * 16][n]).
hipError_t compare_blocks_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n, uint32_t rb_first,
                                 uint32_t rb_stride, uint32_t rb_count, uint32_t* d_common, hipStream_t stream);
// m[j][i] = m[i][j] for i < j on a full n x n matrix
hipError_t symmetrize_launch(uint32_t* d_common, uint32_t n, hipStream_t stream);
hipError_t jaccard_from_counts_launch(const uint32_t* d_common, const uint64_t* d_offsets, uint32_t n,
                                      uint32_t row_lo, uint32_t row_hi, double* d_out, hipStream_t stream);

// ---- compare_ext.hip (bottom-k and abundance-weighted all-pairs) --------------------------------
// Bottom-k sketches (CSR of sorted rows, d_nums[i] = num of sketch i): d_common[i][j] = |A ∩ B ∩ bottom_num(A ∪ B)| with num of
// the lower index (minhash.rs:593-621; the diagonal holds the row sizes), d_union[i][j] = |bottom_num(A ∪ B)| and
// d_jaccard = common / max(1, union) with 1.0 on the diagonal (either may be null).  Full n x n matrices.
hipError_t compare_num_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, const uint32_t* d_nums, uint32_t n,
                              uint32_t* d_common, uint32_t* d_union, double* d_jaccard, hipStream_t stream);
// Abundance-tracking sketches: d_prod[i][j] = sum over common hashes of abund_i * abund_j (u64, wrapping; the diagonal holds the
// row's sum of squares), d_sumsq[i] the same sums of squares, d_common the plain intersection sizes (minhash.rs:635-680).
// narrow: every abundance fits 32 bits (one v_mad_u64_u32 per common hash instead of a 64 x 64 product).
hipError_t compare_abund_launch(const uint64_t* d_hashes, const uint64_t* d_abunds, const uint64_t* d_offsets, uint32_t n,
                                bool narrow, uint32_t* d_common, unsigned long long* d_prod, unsigned long long* d_sumsq,
                                hipStream_t stream, uint64_t total = 0);

// abund_pairs.hip: the same two matrices (diagonals excluded: the caller's row kernel writes them) from joins of per-block lists
// sorted by hash; scratch from the library's arena.  hipErrorNotSupported: 2^32 elements or more -- the caller keeps the walk.
hipError_t abund_pairs_launch(const uint64_t* d_hashes, const uint64_t* d_abunds, const uint64_t* d_offsets, uint32_t n, uint64_t total,
                              bool narrow, uint32_t* d_common, unsigned long long* d_prod, hipStream_t stream);
// Lists with several scaled values: gather the first new_off[r + 1] - new_off[r] hashes of the rows starting at src_start[r] into
// a CSR of their own; then move the entries sub[a][b] of an m x m matrix over rows[] whose pair class max(class_of[rows[a]],
// class_of[rows[b]]) equals `cls` to out[rows[a]][rows[b]] of the n x n matrix.
hipError_t csr_prefix_gather_launch(const uint64_t* d_hashes, const uint64_t* d_src_start, const uint64_t* d_new_off, uint32_t m,
                                    uint64_t* d_out, hipStream_t stream);
hipError_t class_scatter_launch(const uint32_t* d_sub, uint32_t m, const uint32_t* d_rows, const uint32_t* d_class_of, uint32_t cls,
                                uint32_t n, uint32_t* d_out, hipStream_t stream);

// ---- bitindex.hip (dense compare path) ---------------------------------------------------------
hipError_t bitmap_build_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n, const uint64_t* d_dict,
                               uint64_t U, uint32_t* d_bits, uint32_t words_per_row, hipStream_t stream);
// rows: 16-row tiles rb_first, rb_first + rb_stride, ... (rb_count); d_common [rb_count*16][n]; every column, or with
// upper_only every entry on or above the diagonal (entries below it are left as they were: the caller mirrors)
hipError_t bitmatrix_launch(const uint32_t* d_bits, uint32_t words_per_row, uint32_t n, uint32_t rb_first,
                            uint32_t rb_stride, uint32_t rb_count, uint32_t* d_common, hipStream_t stream, bool upper_only = false);

// ---- dictindex.hip (the compare index without a sort) -------------------------------------------
constexpr int DICT_BUCKETS = 512;          // hash-space buckets, one workgroup each
constexpr int DICT_MAX_DISTINCT = 1024;    // distinct hashes a bucket can hold; fuller collections use the sort below
size_t dict_scratch_bytes(uint32_t n);
// slice bounds, pass 1 (distinct hashes + holders per bucket, classified against `threshold`), scan.  The caller zeroes the
// first 256 bytes of d_scratch (the builder's parameters live there; d_out may point at byte 64 of it).  d_out (5 values,
// zero on entry): distinct hashes, frequent ones, rare pair increments, rare elements, buckets that overflowed
hipError_t dict_count_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n, uint32_t threshold, void* d_scratch,
                             unsigned long long* d_out, hipStream_t stream);
// pass 2: bit rows (zeroed by the caller) and the rows of every rare hash (d_rare_end[p] = end of p's run)
hipError_t dict_emit_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n, void* d_scratch, uint32_t* d_bits,
                            uint32_t words_per_row, uint32_t* d_rare_rows, uint32_t* d_rare_end, hipStream_t stream);

// ---- sparse_pairs.hip (inverted compare path) ---------------------------------------------------
size_t inverted_temp_bytes(uint64_t total);
hipError_t inverted_sort_launch(const uint64_t* d_hashes, const uint64_t* d_offsets, uint32_t n, uint64_t total,
                                uint64_t* d_keys_a, uint64_t* d_keys_b, uint32_t* d_rows_tmp, uint32_t* d_rows_sorted,
                                uint32_t* d_counts, uint64_t* d_n_runs, void* d_temp, size_t temp_bytes, hipStream_t stream);
// one read-back for the host: d_out[0] distinct hashes, d_out[1] frequent ones, d_out[2] rare pair increments (zeroed by
// the caller); flags / run offsets / frequent ranks sized for max_runs (= total elements) + 1 entries
hipError_t inverted_classify_launch(const uint32_t* d_counts, const uint64_t* d_n_runs, uint64_t max_runs, uint32_t threshold,
                                    uint32_t* d_freq_flag, uint64_t* d_run_off, uint64_t* d_freq_rank, unsigned long long* d_out,
                                    void* d_temp, size_t temp_bytes, hipStream_t stream);
hipError_t inverted_apply_launch(const uint64_t* d_run_off, const uint32_t* d_freq_flag, const uint64_t* d_freq_rank,
                                 uint64_t n_runs, uint64_t total, const uint32_t* d_rows_sorted, uint32_t* d_run_end,
                                 uint32_t* d_bits, uint32_t words_per_row, hipStream_t stream);
// common[local row][col] += rare-hash contributions, for the rows of the 16-row tiles rb_first, rb_first + rb_stride, ...
hipError_t rare_pairs_launch(const uint32_t* d_rows_sorted, const uint32_t* d_run_end, uint64_t total, uint32_t n,
                             uint32_t rb_first, uint32_t rb_stride, uint32_t rb_count, uint32_t* d_common, hipStream_t stream,
                             bool upper_only = false);

}  // namespace smg
