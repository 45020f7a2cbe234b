// setops.hip -- set algebra on a CSR collection of flat sketches, without leaving device memory.
//
// GPU counterpart of the reference's sketch editing: MinHash.merge / intersection / remove_many (src/core/src/sketch/minhash.rs:
// 432-516, 560-589, 406-430) behind `sig merge --flatten`, `sig intersect` and `sig subtract` (src/sourmash/sig/__main__.py:459-712),
// which work on one pair of sketch objects at a time.  Here
//   * the merge turns every hash of the set into a (group, hash) pair, sorts the pairs (device_sort.hip: sort_pairs), counts the
//     runs of equal pairs (rle_pairs) and keeps, in order, the runs whose count reaches the group's need: need 1 is the union of
//     the group's rows, need = rows of the group their intersection;
//   * the filter walks every row once and keeps the hashes that are (intersect) or are not (subtract) members of another sketch:
//     one sketch for every row, looked up through a query index (qindex.hpp), or the row of the same number of a second set.
// An abundance set (a u64 column aligned with the hashes) goes through the same two: the filter moves a value with every kept hash --
// the hash's own (carry), the other sketch's at the found position (take: sig inflate), or it keeps by a range of the hash's own
// (range: sig filter) -- and the merge writes the sum of a run's abundances, or the run's length, beside the kept hash.  Both are
// static choices, so that the flat forms are the code they were.
// The rules both share with the host are setops_core.hpp's.  Offsets and totals are 64-bit throughout.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include "device_api.hpp"
#include "qindex.hpp"
#include "setops_core.hpp"

namespace smg {

namespace {

unsigned blocks_for(uint64_t n, unsigned cap = 65536) {
    const uint64_t b = (n + SETOPS_BLOCK - 1) / SETOPS_BLOCK;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

size_t scan_bytes(uint64_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)(n ? n : 1), rocprim::plus<uint64_t>(),
                                  (hipStream_t)0);
    return bytes;
}

size_t inclusive_scan_bytes(uint64_t n) {
    size_t bytes = 0;
    (void)rocprim::inclusive_scan(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)(n ? n : 1), rocprim::plus<uint64_t>(), (hipStream_t)0);
    return bytes;
}

// The kept lanes of a chunk take their places: -> the lane's position in the chunk (meaningful for kept lanes), *total the chunk's
// kept lanes.  s_wave: SETOPS_WAVES words of LDS; two barriers, so that the words can be used again by the next chunk.
__device__ __forceinline__ uint32_t chunk_place(bool keep, uint32_t* s_wave, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t mask = __ballot(keep);
    if (lane == 0) s_wave[wave] = setops_wave_total(mask);
    __syncthreads();
    const uint32_t at = setops_wave_base(s_wave, wave) + setops_lane_rank(mask, lane);
    *total = setops_chunk_total(s_wave);
    __syncthreads();
    return at;
}

// ---- merge ---------------------------------------------------------------------------------------------------------------------

// group_rows[g] = rows of group g
__global__ __launch_bounds__(SETOPS_BLOCK) void setops_group_rows_kernel(const uint32_t* __restrict__ groups, uint64_t n, uint64_t n_groups,
                                                                         uint32_t* __restrict__ group_rows) {
    for (uint64_t r = (uint64_t)blockIdx.x * SETOPS_BLOCK + threadIdx.x; r < n; r += (uint64_t)gridDim.x * SETOPS_BLOCK) {
        const uint64_t g = groups ? groups[r] : 0u;
        if (g < n_groups) atomicAdd(&group_rows[g], 1u);
    }
}

// A lane per input hash finds its row by a binary search in the offsets and writes the pair: packed, keys = (group << hbits) | hash;
// wide, keys = hash; vals = group either way.  Every hash value is a pair, 0 included.  PAYLOAD (the summing merge): vals = the
// group above the hash's position in the input (setops_payload), so that the sorted pair still knows where its abundance lies.
template <bool PAYLOAD>
__global__ __launch_bounds__(SETOPS_BLOCK) void setops_assign_kernel(const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                                     uint64_t total, const uint32_t* __restrict__ groups, SetopsKeyForm form,
                                                                     uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
    const uint64_t base = offsets[0];
    for (uint64_t j = (uint64_t)blockIdx.x * SETOPS_BLOCK + threadIdx.x; j < total; j += (uint64_t)gridDim.x * SETOPS_BLOCK) {
        const uint64_t r = setops_row_of(offsets, n, base + j);
        const uint64_t g = groups ? groups[r] : 0u, h = hashes[base + j];
        keys[j] = form.packed ? setops_pack(form, g, h) : h;
        vals[j] = PAYLOAD ? setops_payload(g, j) : g;
    }
}

// The summing merge, behind the sort: a sorted pair's payload gives its group (what the run-length pass compares) and the place of
// its abundance, which is gathered into sorted order for the scan.
__global__ __launch_bounds__(SETOPS_BLOCK) void setops_payload_split_kernel(const uint64_t* __restrict__ payload, uint64_t total,
                                                                            const uint64_t* __restrict__ abunds, const uint64_t* __restrict__ offsets,
                                                                            uint64_t* __restrict__ group_out, uint64_t* __restrict__ abund_out) {
    const uint64_t base = offsets[0];
    for (uint64_t i = (uint64_t)blockIdx.x * SETOPS_BLOCK + threadIdx.x; i < total; i += (uint64_t)gridDim.x * SETOPS_BLOCK) {
        const uint64_t p = payload[i];
        group_out[i] = setops_payload_group(p);
        abund_out[i] = abunds[base + setops_payload_pos(p)];
    }
}

// The runs [0, *n_runs) in chunks of SETOPS_BLOCK: count mode leaves every chunk's kept runs in chunk_count, write mode puts the kept
// runs' hashes and groups at chunk_base[chunk] + their place in the chunk.  n_chunks covers the most runs there can be.
// VALUES (setops_core.hpp: SetopsMergeValues), static: SUM writes the run's sum beside the hash, from the inclusive scan of the
// sorted pairs' abundances and the run's start (the exclusive scan of the counts); COUNT writes the run's length.
template <uint32_t VALUES>
__global__ __launch_bounds__(SETOPS_BLOCK) void setops_keep_kernel(const uint64_t* __restrict__ run_key, const uint64_t* __restrict__ run_group,
                                                                   const uint64_t* __restrict__ run_count, const uint64_t* __restrict__ n_runs_p,
                                                                   uint64_t n_chunks, SetopsKeyForm form, const uint32_t* __restrict__ need,
                                                                   uint32_t need_all, const uint32_t* __restrict__ group_rows, uint32_t write,
                                                                   uint64_t* __restrict__ chunk_count, const uint64_t* __restrict__ chunk_base,
                                                                   uint64_t capacity, uint64_t* __restrict__ out_hash, uint32_t* __restrict__ out_group,
                                                                   const uint64_t* __restrict__ run_start, const uint64_t* __restrict__ abund_scan,
                                                                   uint64_t* __restrict__ out_abund) {
    __shared__ uint32_t s_wave[SETOPS_WAVES];
    const uint64_t n_runs = *n_runs_p;
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint64_t i = c * SETOPS_BLOCK + threadIdx.x;
        bool keep = false;
        uint64_t g = 0, key = 0, count = 0;
        if (i < n_runs) {
            g = run_group[i];
            key = run_key[i];
            count = run_count[i];
            keep = setops_keep(count, setops_need(need, need_all, group_rows, g));
        }
        uint32_t total;
        const uint32_t at = chunk_place(keep, s_wave, &total);
        if (!write) {
            if (threadIdx.x == 0) chunk_count[c] = total;
        } else if (keep) {
            const uint64_t pos = setops_out_pos(chunk_base[c], 0, at, 0);
            if (pos < capacity) {
                out_hash[pos] = form.packed ? setops_packed_hash(form, key) : key;
                out_group[pos] = (uint32_t)g;
                if (VALUES != SETOPS_MERGE_FLAT)
                    out_abund[pos] = setops_merge_value(VALUES, count, VALUES == SETOPS_MERGE_SUM ? setops_run_sum(abund_scan, run_start[i], count) : 0ull);
            }
        }
    }
}

// offsets[g] = first kept run of a group >= g, for g = 0 .. n_groups
__global__ __launch_bounds__(SETOPS_BLOCK) void setops_group_offsets_kernel(const uint32_t* __restrict__ kept_group, const uint64_t* __restrict__ n_kept_p,
                                                                            uint64_t n_groups, uint64_t* __restrict__ offsets) {
    const uint64_t n_kept = *n_kept_p;
    for (uint64_t g = (uint64_t)blockIdx.x * SETOPS_BLOCK + threadIdx.x; g <= n_groups; g += (uint64_t)gridDim.x * SETOPS_BLOCK)
        offsets[g] = g == n_groups ? n_kept : setops_group_start(kept_group, n_kept, g);
}

// lens[g] = the row's length after the num cut (lens[n_groups] = 0, so that a scan over n_groups + 1 closes the offsets)
__global__ __launch_bounds__(SETOPS_BLOCK) void setops_num_lens_kernel(const uint64_t* __restrict__ offsets, uint64_t n_groups, uint64_t num,
                                                                       uint64_t* __restrict__ lens) {
    for (uint64_t g = (uint64_t)blockIdx.x * SETOPS_BLOCK + threadIdx.x; g <= n_groups; g += (uint64_t)gridDim.x * SETOPS_BLOCK)
        lens[g] = g == n_groups ? 0 : setops_num_cut(offsets[g + 1] - offsets[g], num);
}

struct MergeLayout {
    size_t keys_a, vals_a, keys_b, vals_b, counts, kept_hash, kept_group, chunk_count, chunk_base, group_rows, tmp_off, lens, scal, prim, prim_bytes, end;
    size_t sorted_group = 0, sorted_abund = 0, abund_scan = 0, run_start = 0, kept_abund = 0;      // (with values only)
    uint64_t n_chunks;
    MergeLayout(uint64_t total, uint64_t n_groups, bool values = false) {
        n_chunks = (total + SETOPS_BLOCK - 1) / SETOPS_BLOCK;
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t p = at; at += al256(bytes); return p; };
        keys_a = take((total + 1) * 8); vals_a = take((total + 1) * 8); keys_b = take((total + 1) * 8); vals_b = take((total + 1) * 8);
        counts = take((total + 1) * 8); kept_hash = take((total + 1) * 8); kept_group = take((total + 1) * 4);
        chunk_count = take((n_chunks + 2) * 8); chunk_base = take((n_chunks + 2) * 8);
        group_rows = take((n_groups + 1) * 4); tmp_off = take((n_groups + 2) * 8); lens = take((n_groups + 2) * 8); scal = take(256);
        prim_bytes = sort_pairs_temp_bytes(total);
        if (rle_pairs_temp_bytes(total) > prim_bytes) prim_bytes = rle_pairs_temp_bytes(total);
        if (scan_bytes(n_chunks + 1) > prim_bytes) prim_bytes = scan_bytes(n_chunks + 1);
        if (scan_bytes(n_groups + 1) > prim_bytes) prim_bytes = scan_bytes(n_groups + 1);
        if (values) {
            sorted_group = take((total + 1) * 8); sorted_abund = take((total + 1) * 8); abund_scan = take((total + 1) * 8);
            run_start = take((total + 1) * 8); kept_abund = take((total + 1) * 8);
            if (scan_bytes(total) > prim_bytes) prim_bytes = scan_bytes(total);
            if (inclusive_scan_bytes(total) > prim_bytes) prim_bytes = inclusive_scan_bytes(total);
        }
        prim = take(prim_bytes);
        end = at + 256;
    }
};

// ---- filter --------------------------------------------------------------------------------------------------------------------

// pieces[r] = work items of row r (pieces[n] = 0: the scan over n + 1 entries leaves the number of items in piece_start[n])
__global__ __launch_bounds__(SETOPS_BLOCK) void setops_pieces_kernel(const uint64_t* __restrict__ offsets, uint64_t n, uint64_t* __restrict__ pieces) {
    for (uint64_t r = (uint64_t)blockIdx.x * SETOPS_BLOCK + threadIdx.x; r <= n; r += (uint64_t)gridDim.x * SETOPS_BLOCK)
        pieces[r] = r == n ? 0 : setops_pieces(offsets[r + 1] - offsets[r]);
}

__global__ __launch_bounds__(SETOPS_BLOCK) void setops_table_kernel(const uint64_t* __restrict__ Q, uint64_t n, uint32_t shift, uint32_t buckets, uint32_t* __restrict__ T) {
    qindex_fill_bucket(Q, n, shift, buckets, T, blockIdx.x * SETOPS_BLOCK + threadIdx.x);
}
__global__ __launch_bounds__(SETOPS_BLOCK) void setops_record_kernel(const uint64_t* __restrict__ Q, const uint32_t* __restrict__ T, uint32_t buckets, QRec* __restrict__ rec) {
    qindex_fill_record(Q, T, buckets, rec, blockIdx.x * SETOPS_BLOCK + threadIdx.x);
}

struct FilterKernelArgs {
    const uint64_t *hashes, *offsets;
    uint64_t n;
    const uint64_t* piece_start;                    // n + 1: the first work item of every row; [n] = the number of items
    QIndex qi;                                      // one sketch: the other sketch behind its index
    uint64_t other_n, other_max;
    const uint64_t *other_hashes, *other_offsets;   // row-wise: the second set
    uint32_t keep_present, write;
    uint64_t* piece_count;                          // count mode writes it, write mode compares with it
    const uint64_t* piece_base;                     // the scan of piece_count: where a piece's kept hashes start in the output
    uint64_t* out;
    unsigned long long* ticket;
    uint32_t* trouble;
    // values (read by the value-moving instantiations only)
    const uint64_t *abunds, *other_abunds;          // aligned with hashes / with other_hashes (one sketch: with the caller's unpadded copy)
    uint64_t range_lo, range_hi;
    uint64_t* out_abund;
};

// One kernel, two modes.  A workgroup takes a work item -- a row, or a piece of a long one -- by ticket (its first is its own
// number, every later one gridDim.x + a ticket), walks it in chunks of SETOPS_BLOCK hashes and keeps, in row order, the hashes whose
// membership in the other sketch is what the operation keeps.  Count mode leaves the item's kept hashes in piece_count; write mode
// puts them behind piece_base[item] and reports an item that kept another number than was counted.  A workgroup waits on its own
// barriers only.
// VALUES (setops_core.hpp: SetopsValueMode) is static, so that the flat form reads, holds and writes nothing more than it did:
// CARRY stores the hash's own abundance beside it; TAKE keeps the position the lookup found and stores the other sketch's abundance
// at that position (one global read per kept hash, in write mode only; a staged partner's hashes are read from LDS, its abundances
// are not staged); RANGE makes no lookup at all and keeps by the hash's own abundance.
template <bool ROWWISE, uint32_t VALUES>
__global__ __launch_bounds__(SETOPS_BLOCK) void setops_filter_kernel(FilterKernelArgs a) {
    __shared__ __attribute__((aligned(16))) uint64_t s_partner[ROWWISE ? SETOPS_LDS_PARTNER : 1];
    __shared__ uint32_t s_wave[SETOPS_WAVES];
    __shared__ unsigned long long s_next[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_items = a.piece_start[a.n];
    uint64_t t = blockIdx.x;
    for (uint32_t step = 0; t < n_items; ++step) {
        if (tid == 0) s_next[step & 1u] = (unsigned long long)gridDim.x + atomicAdd(a.ticket, 1ull);
        const uint64_t r = setops_row_of(a.piece_start, a.n, t);
        const uint64_t lo = a.offsets[r], hi = a.offsets[r + 1];
        const uint64_t i0 = lo + (t - a.piece_start[r]) * SETOPS_SPLIT;
        const uint64_t i1 = hi - i0 > SETOPS_SPLIT ? i0 + SETOPS_SPLIT : hi;
        uint64_t other_n = a.other_n, other_max = a.other_max;
        const uint64_t* partner = nullptr;
        bool staged = false;
        if (ROWWISE) {
            const uint64_t plo = a.other_offsets[r];
            other_n = a.other_offsets[r + 1] - plo;
            partner = a.other_hashes + plo;
            other_max = other_n ? partner[other_n - 1] : 0;
            staged = other_n <= SETOPS_LDS_PARTNER;
            if (staged) {
                for (uint32_t k = tid; k < (uint32_t)other_n; k += SETOPS_BLOCK) s_partner[k] = partner[k];
                __syncthreads();
            }
        }
        const uint64_t base = a.write ? a.piece_base[t] : 0, counted = a.write ? a.piece_count[t] : 0;
        uint64_t running = 0;
        for (uint64_t c = i0; c < i1; c += SETOPS_BLOCK) {
            const uint64_t i = c + tid;
            bool keep = false;
            uint64_t x = 0;
            uint64_t own = 0, where = SETOPS_NOT_FOUND;                // (value forms only: the hash's abundance, its place in the other sketch)
            if (i < i1) {
                x = a.hashes[i];
                if (VALUES == SETOPS_VALUES_RANGE) {
                    own = a.abunds[i];
                    keep = setops_in_range(own, a.range_lo, a.range_hi);
                } else if (VALUES == SETOPS_VALUES_TAKE) {
                    if (ROWWISE) {
                        where = staged ? setops_member_at(x, other_n, other_max, [&](uint64_t v) { return setops_find(s_partner, other_n, v); })
                                       : setops_member_at(x, other_n, other_max, [&](uint64_t v) { return setops_find(partner, other_n, v); });
                        if (where != SETOPS_NOT_FOUND) where += partner - a.other_hashes;
                    } else {
                        where = setops_member_at(x, other_n, other_max, [&](uint64_t v) {
                            const uint32_t p = q_find_rec(a.qi, v);
                            return p == NONE32 ? SETOPS_NOT_FOUND : (uint64_t)p;
                        });
                    }
                    keep = where != SETOPS_NOT_FOUND;
                } else {
                    bool present;
                    if (ROWWISE) {
                        // (two calls, so that each search knows its address space: LDS reads, or global ones)
                        present = staged ? setops_member(x, other_n, other_max, [&](uint64_t v) { return setops_search(s_partner, other_n, v); })
                                         : setops_member(x, other_n, other_max, [&](uint64_t v) { return setops_search(partner, other_n, v); });
                    } else {
                        present = setops_member(x, other_n, other_max, [&](uint64_t v) { return q_find_rec(a.qi, v) != NONE32; });
                    }
                    keep = setops_filter_keeps(present, a.keep_present != 0);
                }
            }
            uint32_t total;
            const uint32_t at = chunk_place(keep, s_wave, &total);
            // (a place behind the counted size is never written: the mismatch is reported below, nothing lands in another item's room)
            if (a.write && keep && running + at < counted) {
                const uint64_t pos = setops_out_pos(base, running, at, 0);
                a.out[pos] = x;
                if (VALUES == SETOPS_VALUES_CARRY) own = a.abunds[i];
                if (VALUES != SETOPS_VALUES_NONE)
                    a.out_abund[pos] = setops_filter_value(VALUES, own, VALUES == SETOPS_VALUES_TAKE ? a.other_abunds[where] : 0ull);
            }
            running += total;
        }
        if (tid == 0) {
            if (!a.write) a.piece_count[t] = running;
            else if (running != counted) atomicOr(a.trouble, (uint32_t)SETOPS_COUNT_MISMATCH);
        }
        __syncthreads();                                 // s_next is written, s_partner is free again
        t = s_next[step & 1u];
    }
}

// out_offsets[r] = where row r starts in the output: the base of its first piece (r = n: the total)
__global__ __launch_bounds__(SETOPS_BLOCK) void setops_row_offsets_kernel(const uint64_t* __restrict__ piece_start, const uint64_t* __restrict__ piece_base,
                                                                          uint64_t n, uint64_t* __restrict__ out_offsets) {
    for (uint64_t r = (uint64_t)blockIdx.x * SETOPS_BLOCK + threadIdx.x; r <= n; r += (uint64_t)gridDim.x * SETOPS_BLOCK)
        out_offsets[r] = piece_base[piece_start[r]];
}

struct FilterLayout {
    size_t pieces, piece_start, piece_count, piece_base, Q, T, rec, scal, prim, prim_bytes, end;
    uint64_t p_max, max_buckets;
    FilterLayout(uint64_t n, uint64_t total, uint64_t other_len) {
        p_max = n + total / SETOPS_SPLIT;                // (setops_pieces(len) <= 1 + len / SETOPS_SPLIT)
        max_buckets = 2 * other_len + 2;
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t p = at; at += al256(bytes); return p; };
        pieces = take((n + 2) * 8); piece_start = take((n + 2) * 8); piece_count = take((p_max + 2) * 8); piece_base = take((p_max + 2) * 8);
        Q = take((other_len + 8) * 8); T = take((max_buckets + 2) * 4); rec = take((max_buckets + 1) * sizeof(QRec)); scal = take(256);
        prim_bytes = scan_bytes(n + 1);
        if (scan_bytes(p_max + 1) > prim_bytes) prim_bytes = scan_bytes(p_max + 1);
        prim = take(prim_bytes);
        end = at + 256;
    }
};

}  // namespace

// ---- merge ---------------------------------------------------------------------------------------------------------------------

size_t setops_merge_workspace_bytes(uint64_t total, uint64_t n_groups) { return MergeLayout(total, n_groups).end; }
size_t setops_merge_values_workspace_bytes(uint64_t total, uint64_t n_groups) { return MergeLayout(total, n_groups, true).end; }

hipError_t setops_merge_run(const SetopsMergeArgs& a, uint64_t* total_out, hipStream_t st) {
    if (!total_out || !a.d_out_offsets || !a.d_result) return hipErrorInvalidValue;
    *total_out = 0;
    if (a.total > SETOPS_MERGE_MAX_HASHES || a.n_groups > 0xfffffffeull || a.n >= 0xffffffffull) return hipErrorInvalidValue;
    if (a.values > SETOPS_MERGE_COUNT || (a.values == SETOPS_MERGE_SUM && a.total && !a.d_abunds) || (a.values && a.total && !a.d_out_abunds))
        return hipErrorInvalidValue;
    const bool sum = a.values == SETOPS_MERGE_SUM;
    const MergeLayout L(a.total, a.n_groups, a.values != SETOPS_MERGE_FLAT);
    if (a.workspace_bytes < L.end) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = hipMemsetAsync(a.d_result, 0, 16, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.d_out_offsets, 0, (a.n_groups + 1) * 8, st)) != hipSuccess) return e;
    if (a.total == 0 || a.n_groups == 0 || a.n == 0) return hipStreamSynchronize(st);
    char* ws = static_cast<char*>(a.d_workspace);
    uint64_t *keys_a = (uint64_t*)(ws + L.keys_a), *vals_a = (uint64_t*)(ws + L.vals_a), *keys_b = (uint64_t*)(ws + L.keys_b),
             *vals_b = (uint64_t*)(ws + L.vals_b), *counts = (uint64_t*)(ws + L.counts), *chunk_count = (uint64_t*)(ws + L.chunk_count),
             *chunk_base = (uint64_t*)(ws + L.chunk_base), *tmp_off = (uint64_t*)(ws + L.tmp_off), *lens = (uint64_t*)(ws + L.lens),
             *scal = (uint64_t*)(ws + L.scal);
    uint32_t *kept_group = (uint32_t*)(ws + L.kept_group), *group_rows = (uint32_t*)(ws + L.group_rows);
    void* prim = ws + L.prim;
    const SetopsKeyForm form = setops_key_form(a.max_hash, a.n_groups);
    const uint64_t total = a.total;

    if (a.need_all) {
        if ((e = hipMemsetAsync(group_rows, 0, (a.n_groups + 1) * 4, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(setops_group_rows_kernel, dim3(blocks_for(a.n)), dim3(SETOPS_BLOCK), 0, st, a.d_groups, a.n, a.n_groups, group_rows);
    }
    if (sum)
        hipLaunchKernelGGL(setops_assign_kernel<true>, dim3(blocks_for(total)), dim3(SETOPS_BLOCK), 0, st, a.d_hashes, a.d_offsets, a.n, total, a.d_groups, form,
                           keys_a, vals_a);
    else
        hipLaunchKernelGGL(setops_assign_kernel<false>, dim3(blocks_for(total)), dim3(SETOPS_BLOCK), 0, st, a.d_hashes, a.d_offsets, a.n, total, a.d_groups,
                           form, keys_a, vals_a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the pairs ordered by (group, hash), and the runs of equal pairs: run_key (the packed key, or the hash), run_group, counts
    const uint64_t *run_key, *run_group;
    uint64_t *sorted_group = (uint64_t*)(ws + L.sorted_group), *sorted_abund = (uint64_t*)(ws + L.sorted_abund), *abund_scan = (uint64_t*)(ws + L.abund_scan),
             *run_start = (uint64_t*)(ws + L.run_start);
    size_t pb = L.prim_bytes;
    // (the run-length pass writes a count per run; the scan below reads `total` of them, so the ones behind the last run are 0)
    if (sum && (e = hipMemsetAsync(counts, 0, (total + 1) * 8, st)) != hipSuccess) return e;
    if (form.packed) {
        if ((e = sort_pairs(keys_a, keys_b, vals_a, vals_b, total, (int)(form.hbits + form.gbits), prim, L.prim_bytes, st)) != hipSuccess) return e;
        const uint64_t* groups_sorted = vals_b;
        if (sum) {      // the payload splits into the group and the pair's abundance, both in sorted order
            hipLaunchKernelGGL(setops_payload_split_kernel, dim3(blocks_for(total)), dim3(SETOPS_BLOCK), 0, st, vals_b, total, a.d_abunds, a.d_offsets,
                               sorted_group, sorted_abund);
            groups_sorted = sorted_group;
        }
        if ((e = rle_pairs(keys_b, groups_sorted, total, keys_a, vals_a, counts, scal, prim, L.prim_bytes, st)) != hipSuccess) return e;
        run_key = keys_a; run_group = vals_a;
    } else if (!sum) {
        // two stable passes: by hash, then by group
        if ((e = sort_pairs(keys_a, keys_b, vals_a, vals_b, total, (int)form.hbits, prim, L.prim_bytes, st)) != hipSuccess) return e;
        if ((e = sort_pairs(vals_b, vals_a, keys_b, keys_a, total, (int)form.gbits, prim, L.prim_bytes, st)) != hipSuccess) return e;
        if ((e = rle_pairs(vals_a, keys_a, total, vals_b, keys_b, counts, scal, prim, L.prim_bytes, st)) != hipSuccess) return e;
        run_key = keys_b; run_group = vals_b;
    } else {
        // the same two stable passes with the payload for a group: the second orders by the payload's group bits only
        if ((e = sort_pairs(keys_a, keys_b, vals_a, vals_b, total, (int)form.hbits, prim, L.prim_bytes, st)) != hipSuccess) return e;
        if ((e = sort_pairs(vals_b, vals_a, keys_b, keys_a, total, (int)form.gbits, prim, L.prim_bytes, st, 32)) != hipSuccess) return e;
        hipLaunchKernelGGL(setops_payload_split_kernel, dim3(blocks_for(total)), dim3(SETOPS_BLOCK), 0, st, vals_a, total, a.d_abunds, a.d_offsets,
                           sorted_group, sorted_abund);
        if ((e = rle_pairs(sorted_group, keys_a, total, vals_b, keys_b, counts, scal, prim, L.prim_bytes, st)) != hipSuccess) return e;
        run_key = keys_b; run_group = vals_b;
    }
    if (sum) {
        // run sums without atomics or a loop per run: one inclusive scan of the abundances in sorted order (wrapping u64: exact
        // modulo 2^64), and the runs' starts from the exclusive scan of their counts (entries behind the last run are 0 and not used)
        pb = L.prim_bytes;
        if ((e = rocprim::inclusive_scan(prim, pb, (const uint64_t*)sorted_abund, abund_scan, (size_t)total, rocprim::plus<uint64_t>(), st)) != hipSuccess) return e;
        pb = L.prim_bytes;
        if ((e = rocprim::exclusive_scan(prim, pb, (const uint64_t*)counts, run_start, (uint64_t)0, (size_t)total, rocprim::plus<uint64_t>(), st)) != hipSuccess)
            return e;
    }
    // with a num cut the kept runs stop over in the workspace, and the cut rows are gathered from there
    uint64_t* kept_hash = a.num ? (uint64_t*)(ws + L.kept_hash) : a.d_out_hashes;
    uint64_t* kept_abund = !a.values ? nullptr : a.num ? (uint64_t*)(ws + L.kept_abund) : a.d_out_abunds;
    uint64_t* kept_off = a.num ? tmp_off : a.d_out_offsets;
    if (!kept_hash || !a.d_out_hashes) return hipErrorInvalidValue;
    if ((e = hipMemsetAsync(chunk_count, 0, (L.n_chunks + 2) * 8, st)) != hipSuccess) return e;
    const unsigned g_keep = (unsigned)(L.n_chunks < 65536 ? L.n_chunks : 65536);
    auto keep_launch = [&](uint32_t write) {
#define SMG_KEEP_LAUNCH(V)                                                                                                                           \
    hipLaunchKernelGGL(setops_keep_kernel<V>, dim3(g_keep), dim3(SETOPS_BLOCK), 0, st, run_key, run_group, counts, scal, L.n_chunks, form, a.d_need, \
                       a.need_all, group_rows, write, chunk_count, chunk_base, total, kept_hash, kept_group, run_start, abund_scan, kept_abund)
        if (a.values == SETOPS_MERGE_SUM) SMG_KEEP_LAUNCH(SETOPS_MERGE_SUM);
        else if (a.values == SETOPS_MERGE_COUNT) SMG_KEEP_LAUNCH(SETOPS_MERGE_COUNT);
        else SMG_KEEP_LAUNCH(SETOPS_MERGE_FLAT);
#undef SMG_KEEP_LAUNCH
    };
    keep_launch(0u);
    pb = L.prim_bytes;
    if ((e = rocprim::exclusive_scan(prim, pb, (const uint64_t*)chunk_count, chunk_base, (uint64_t)0, (size_t)(L.n_chunks + 1), rocprim::plus<uint64_t>(), st)) !=
        hipSuccess)
        return e;
    keep_launch(1u);
    hipLaunchKernelGGL(setops_group_offsets_kernel, dim3(blocks_for(a.n_groups + 1)), dim3(SETOPS_BLOCK), 0, st, kept_group, chunk_base + L.n_chunks,
                       a.n_groups, kept_off);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.num) {
        hipLaunchKernelGGL(setops_num_lens_kernel, dim3(blocks_for(a.n_groups + 1)), dim3(SETOPS_BLOCK), 0, st, tmp_off, a.n_groups, a.num, lens);
        pb = L.prim_bytes;
        if ((e = rocprim::exclusive_scan(prim, pb, (const uint64_t*)lens, a.d_out_offsets, (uint64_t)0, (size_t)(a.n_groups + 1), rocprim::plus<uint64_t>(),
                                         st)) != hipSuccess)
            return e;
        if ((e = csr_prefix_gather_launch(kept_hash, tmp_off, a.d_out_offsets, (uint32_t)a.n_groups, a.d_out_hashes, st)) != hipSuccess) return e;
        if (a.values && (e = csr_prefix_gather_launch(kept_abund, tmp_off, a.d_out_offsets, (uint32_t)a.n_groups, a.d_out_abunds, st)) != hipSuccess) return e;
    }
    if ((e = hipMemcpyAsync(a.d_result, a.d_out_offsets + a.n_groups, 8, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(a.d_result + 1, scal, 8, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(total_out, a.d_result, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    return hipStreamSynchronize(st);
}

// ---- filter --------------------------------------------------------------------------------------------------------------------

size_t setops_filter_workspace_bytes(uint64_t n, uint64_t total, uint64_t other_len) { return FilterLayout(n, total, other_len).end; }

namespace {

hipError_t filter_launch(const SetopsFilterArgs& a, const FilterLayout& L, const QIndex& qi, uint64_t other_max, uint32_t write, uint64_t* d_out,
                         uint64_t* d_out_abunds, hipStream_t st) {
    char* ws = static_cast<char*>(a.d_workspace);
    uint64_t* scal = (uint64_t*)(ws + L.scal);
    FilterKernelArgs k;
    k.hashes = a.d_hashes; k.offsets = a.d_offsets; k.n = a.n;
    k.piece_start = (const uint64_t*)(ws + L.piece_start);
    k.qi = qi; k.other_n = a.d_other_offsets ? 0 : a.other_len; k.other_max = other_max;
    k.other_hashes = a.d_other_hashes; k.other_offsets = a.d_other_offsets;
    k.keep_present = a.keep_present; k.write = write;
    k.piece_count = (uint64_t*)(ws + L.piece_count); k.piece_base = (const uint64_t*)(ws + L.piece_base);
    k.out = d_out;
    k.ticket = (unsigned long long*)scal;
    k.trouble = (uint32_t*)(scal + 1);
    k.abunds = a.d_abunds; k.other_abunds = a.d_other_abunds; k.range_lo = a.range_lo; k.range_hi = a.range_hi; k.out_abund = d_out_abunds;
    hipError_t e = hipMemsetAsync(scal, 0, 8, st);               // in stream order: the launch in front has finished with the counter
    if (e != hipSuccess) return e;
    const unsigned full = 256u * 8u;
    const unsigned g = a.grid ? a.grid : (unsigned)(L.p_max < full ? L.p_max : full);
    const bool rowwise = a.d_other_offsets != nullptr;
#define SMG_FILTER_LAUNCH(RW, V) hipLaunchKernelGGL((setops_filter_kernel<RW, V>), dim3(g), dim3(SETOPS_BLOCK), 0, st, k)
    switch (a.values) {
    case SETOPS_VALUES_NONE: if (rowwise) SMG_FILTER_LAUNCH(true, SETOPS_VALUES_NONE); else SMG_FILTER_LAUNCH(false, SETOPS_VALUES_NONE); break;
    case SETOPS_VALUES_CARRY: if (rowwise) SMG_FILTER_LAUNCH(true, SETOPS_VALUES_CARRY); else SMG_FILTER_LAUNCH(false, SETOPS_VALUES_CARRY); break;
    case SETOPS_VALUES_TAKE: if (rowwise) SMG_FILTER_LAUNCH(true, SETOPS_VALUES_TAKE); else SMG_FILTER_LAUNCH(false, SETOPS_VALUES_TAKE); break;
    case SETOPS_VALUES_RANGE: if (rowwise) return hipErrorInvalidValue; SMG_FILTER_LAUNCH(false, SETOPS_VALUES_RANGE); break;
    default: return hipErrorInvalidValue;
    }
#undef SMG_FILTER_LAUNCH
    return hipGetLastError();
}

}  // namespace

hipError_t setops_filter_count(const SetopsFilterArgs& a, SetopsFilterState& s, uint64_t* total_out, hipStream_t st) {
    if (!total_out || !a.d_out_offsets || !a.d_result) return hipErrorInvalidValue;
    *total_out = 0;
    s = SetopsFilterState();
    if (a.n >= 0xffffffffull || a.grid > (1u << 20) || (!a.d_other_offsets && a.other_len > SETOPS_OTHER_MAX_HASHES)) return hipErrorInvalidValue;
    if (a.values > SETOPS_VALUES_RANGE) return hipErrorInvalidValue;
    if ((a.values == SETOPS_VALUES_CARRY || a.values == SETOPS_VALUES_RANGE) && a.total && !a.d_abunds) return hipErrorInvalidValue;
    if (a.values == SETOPS_VALUES_RANGE && (a.d_other_offsets || a.other_len)) return hipErrorInvalidValue;
    if (a.values == SETOPS_VALUES_TAKE && (!a.keep_present || ((a.d_other_offsets || a.other_len) && !a.d_other_abunds))) return hipErrorInvalidValue;
    const FilterLayout L(a.n, a.total, a.d_other_offsets ? 0 : a.other_len);
    if (a.workspace_bytes < L.end) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = hipMemsetAsync(a.d_result, 0, 16, st)) != hipSuccess) return e;
    if (a.n == 0) {
        if ((e = hipMemsetAsync(a.d_out_offsets, 0, 8, st)) != hipSuccess) return e;
        s.counted = true;                               // no rows: a count of nothing, and nothing to write
        return hipStreamSynchronize(st);
    }
    char* ws = static_cast<char*>(a.d_workspace);
    uint64_t *pieces = (uint64_t*)(ws + L.pieces), *piece_start = (uint64_t*)(ws + L.piece_start), *piece_count = (uint64_t*)(ws + L.piece_count),
             *piece_base = (uint64_t*)(ws + L.piece_base), *Q = (uint64_t*)(ws + L.Q), *scal = (uint64_t*)(ws + L.scal);
    uint32_t* T = (uint32_t*)(ws + L.T);
    QRec* rec = (QRec*)(ws + L.rec);
    void* prim = ws + L.prim;
    if ((e = hipMemsetAsync(scal, 0, 256, st)) != hipSuccess) return e;
    // the one sketch behind a query index with records, built once: a padded copy, the table, the records
    QIndex qi;
    qi.Q = nullptr; qi.nq = 0; qi.T = nullptr; qi.shift = 0; qi.qmax = 0; qi.rec = nullptr;
    if (!a.d_other_offsets && a.other_len) {
        const uint64_t nq = a.other_len;
        if (!a.d_other_hashes) return hipErrorInvalidValue;
        if ((e = hipMemcpyAsync(Q, a.d_other_hashes, nq * 8, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(Q + nq, 0, 64, st)) != hipSuccess) return e;
        uint64_t q_max = 0;
        if ((e = hipMemcpyAsync(&q_max, Q + nq - 1, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        uint32_t shift = 0, buckets = 0;
        qindex_geometry(nq, q_max, &shift, &buckets);
        if ((uint64_t)buckets > L.max_buckets) return hipErrorInvalidValue;      // (qindex_geometry: never more than 2 n + 1; an unsorted sketch could)
        hipLaunchKernelGGL(setops_table_kernel, dim3((buckets + 1 + SETOPS_BLOCK - 1) / SETOPS_BLOCK), dim3(SETOPS_BLOCK), 0, st, Q, nq, shift, buckets, T);
        hipLaunchKernelGGL(setops_record_kernel, dim3((buckets + SETOPS_BLOCK - 1) / SETOPS_BLOCK), dim3(SETOPS_BLOCK), 0, st, Q, T, buckets, rec);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        qi.Q = Q; qi.nq = nq; qi.T = T; qi.shift = shift; qi.qmax = q_max; qi.rec = rec;
    }
    s.qi = qi;
    s.other_max = qi.qmax;
    // the work items, counted; one exclusive scan of the counts gives every item's place, and with it the rows' offsets
    hipLaunchKernelGGL(setops_pieces_kernel, dim3(blocks_for(a.n + 1)), dim3(SETOPS_BLOCK), 0, st, a.d_offsets, a.n, pieces);
    size_t pb = L.prim_bytes;
    if ((e = rocprim::exclusive_scan(prim, pb, (const uint64_t*)pieces, piece_start, (uint64_t)0, (size_t)(a.n + 1), rocprim::plus<uint64_t>(), st)) != hipSuccess)
        return e;
    if ((e = hipMemsetAsync(piece_count, 0, (L.p_max + 2) * 8, st)) != hipSuccess) return e;
    if ((e = filter_launch(a, L, qi, s.other_max, 0u, nullptr, nullptr, st)) != hipSuccess) return e;
    pb = L.prim_bytes;
    if ((e = rocprim::exclusive_scan(prim, pb, (const uint64_t*)piece_count, piece_base, (uint64_t)0, (size_t)(L.p_max + 1), rocprim::plus<uint64_t>(), st)) !=
        hipSuccess)
        return e;
    hipLaunchKernelGGL(setops_row_offsets_kernel, dim3(blocks_for(a.n + 1)), dim3(SETOPS_BLOCK), 0, st, piece_start, piece_base, a.n, a.d_out_offsets);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(a.d_result, a.d_out_offsets + a.n, 8, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(total_out, a.d_result, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    s.counted = true;
    s.total = *total_out;
    return hipSuccess;
}

hipError_t setops_filter_write(const SetopsFilterArgs& a, const SetopsFilterState& s, uint64_t* d_out_hashes, uint64_t capacity, uint32_t* trouble,
                               hipStream_t st, uint64_t* d_out_abunds) {
    if (!trouble || !s.counted || capacity < s.total) return hipErrorInvalidValue;
    *trouble = SETOPS_OK;
    if (a.n == 0 || s.total == 0) return hipSuccess;
    if (!d_out_hashes || (a.values != SETOPS_VALUES_NONE && !d_out_abunds)) return hipErrorInvalidValue;
    const FilterLayout L(a.n, a.total, a.d_other_offsets ? 0 : a.other_len);
    hipError_t e;
    if ((e = filter_launch(a, L, s.qi, s.other_max, 1u, d_out_hashes, d_out_abunds, st)) != hipSuccess) return e;
    uint64_t* scal = (uint64_t*)(static_cast<char*>(a.d_workspace) + L.scal);
    uint64_t word = 0;
    if ((e = hipMemcpyAsync(a.d_result + 1, scal + 1, 8, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&word, scal + 1, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    *trouble = (uint32_t)word;
    return hipSuccess;
}

}  // namespace smg
