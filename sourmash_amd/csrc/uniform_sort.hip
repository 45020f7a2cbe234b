// uniform_sort.hip -- sort + unique (+ multiplicities) of keys that are uniform on [0, thr], with the count read on the device.
//
// The kept hashes of a sketch are MurmurHash3 values: their top bits say where they go.  Instead of the general radix sort's seven
// passes and a run-length encode (device_sort.hip), the keys are scattered to leaves of the key space in one or two 256-way
// passes, every leaf is sorted and deduplicated in LDS by one workgroup, and a scan + copy packs the leaves (plan and rules:
// uniform_sort_core.hpp).  Small inputs take one workgroup and one kernel.  Nothing here reads a size back: grids are sized from
// n_max and workgroups past min(*d_n, n_max) leave at once.  Keys that do not spread as the plan assumes raise *d_fellback and the
// caller sorts the untouched input with sort_unique.
#include <hip/hip_runtime.h>
#include "device_api.hpp"
#include "uniform_sort_core.hpp"

namespace smg {
namespace {

constexpr uint32_t NO_BASE = 0xffffffffu;

__device__ __forceinline__ uint64_t us_count(const unsigned long long* d_n, uint64_t n_max) {
    const uint64_t n = *d_n;
    return n < n_max ? n : n_max;
}

// keys[0, n) in LDS, sorted by T threads
template <int T>
__device__ __forceinline__ void us_sort_lds(uint64_t* keys, uint32_t n) {
    const uint32_t P = us_pow2(n);
    for (uint32_t k = 2, j = 0; k <= P; us_next_step(k, j)) {
        for (uint32_t t = threadIdx.x; t < P / 2; t += T) {
            uint32_t a, b;
            us_pair(t, k, j, a, b);
            us_compare_exchange(keys, n, a, b);
        }
        __syncthreads();
    }
}

// exclusive prefix of v over the workgroup's T threads and the total; wsum: T / 64 words of LDS, free again on return
template <int T>
__device__ __forceinline__ uint32_t us_block_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < T / 64; ++w) {
        const uint32_t t = wsum[w];
        if (w < wave) base += t;
        all += t;
    }
    __syncthreads();
    total = all;
    return base + x - v;
}

// src[0, n) (global) -> sorted in s[0, n) (LDS) by T threads of E keys each: counting sort over B bins (bins: B + 1 words of LDS,
// thread t owns the bins [t * B / T, (t + 1) * B / T)), ranks inside a bin by us_before; the sorting network when a bin is crowded
template <int T, int E, int B, bool LEAF>
__device__ __forceinline__ void us_sort_keys(const uint64_t* src, uint32_t n, uint32_t bin_shift, uint64_t* s, uint32_t* bins,
                                             uint32_t* wsum) {
    constexpr int BPT = B / T;
    static_assert(B % T == 0, "bins per thread");
#pragma unroll
    for (int i = 0; i < BPT; ++i) bins[threadIdx.x + i * T] = 0;
    __syncthreads();
    uint64_t key[E];
    uint32_t at[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t i = threadIdx.x + e * T;
        key[e] = 0;
        at[e] = 0;
        if (i < n) {
            key[e] = src[i];
            at[e] = atomicAdd(&bins[LEAF ? us_bin_leaf(bin_shift, key[e]) : us_bin_small(bin_shift, key[e])], 1u);
        }
    }
    __syncthreads();
    uint32_t mine[BPT], sum = 0, most = 0;
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
        mine[i] = bins[threadIdx.x * BPT + i];
        sum += mine[i];
        most = mine[i] > most ? mine[i] : most;
    }
    uint32_t total;
    uint32_t start = us_block_scan<T>(sum, wsum, total);
    if (__syncthreads_or(most > US_BIN_LIMIT)) {
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (threadIdx.x + e * T < n) s[threadIdx.x + e * T] = key[e];
        __syncthreads();
        us_sort_lds<T>(s, n);
        return;
    }
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
        bins[threadIdx.x * BPT + i] = start;
        start += mine[i];
    }
    if (threadIdx.x == T - 1) bins[B] = start;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (threadIdx.x + e * T >= n) continue;
        at[e] += bins[LEAF ? us_bin_leaf(bin_shift, key[e]) : us_bin_small(bin_shift, key[e])];
        s[at[e]] = key[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (threadIdx.x + e * T >= n) continue;
        const uint32_t b = LEAF ? us_bin_leaf(bin_shift, key[e]) : us_bin_small(bin_shift, key[e]);
        const uint32_t lo = bins[b], hi = bins[b + 1];
        uint32_t rank = lo;
        for (uint32_t m = lo; m < hi; ++m) rank += us_before(s[m], m, key[e], at[e]) ? 1u : 0u;
        at[e] = rank;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (threadIdx.x + e * T < n) s[at[e]] = key[e];
    __syncthreads();
}

// The distinct keys of the sorted keys[0, n) (LDS) to out[0, total), their run lengths to counts (may be null); thread t owns the
// slots [t * E, t * E + E).  A run's head writes minus its slot, the run's tail adds its slot + 1 behind a barrier.  -> total
template <int T, int E, typename CT>
__device__ __forceinline__ uint32_t us_unique_write(const uint64_t* keys, uint32_t n, uint32_t* scan, uint64_t* out, CT* counts) {
    const uint32_t lo = threadIdx.x * E;
    uint32_t heads = 0;
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (lo + e < n && us_is_head(keys, lo + e)) ++heads;
    uint32_t total;
    const uint32_t first = us_block_scan<T>(heads, scan, total);
    uint32_t q = first;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t i = lo + e;
        if (i < n && us_is_head(keys, i)) {
            out[q] = keys[i];
            if (counts) counts[q] = (CT)0 - (CT)i;
            ++q;
        }
    }
    if (counts) {
        __syncthreads();
        q = first;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t i = lo + e;
            if (i >= n) break;
            if (us_is_head(keys, i)) ++q;
            if (us_is_tail(keys, n, i)) counts[q - 1] += (CT)(i + 1);
        }
    }
    return total;
}

// ---- small form: everything in one workgroup ---------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void us_small_kernel(const uint64_t* __restrict__ keys, const unsigned long long* __restrict__ d_n,
                                                        uint64_t n_max, uint32_t small_shift, uint64_t* __restrict__ out,
                                                        uint64_t* __restrict__ counts, uint64_t* __restrict__ d_n_out,
                                                        uint32_t* __restrict__ d_fellback) {
    __shared__ uint64_t s[US_SMALL_MAX];
    __shared__ uint32_t bins[US_SMALL_BINS + 1];
    __shared__ uint32_t scan[1024 / 64];
    const uint32_t n = (uint32_t)us_count(d_n, n_max < US_SMALL_MAX ? n_max : US_SMALL_MAX);
    us_sort_keys<1024, US_SMALL_MAX / 1024, US_SMALL_BINS, false>(keys, n, small_shift, s, bins, scan);
    const uint32_t total = us_unique_write<1024, US_SMALL_MAX / 1024, uint64_t>(s, n, scan, out, counts);
    if (threadIdx.x == 0) {
        *d_n_out = total;
        *d_fellback = 0;
    }
}

// ---- bucket form ---------------------------------------------------------------------------------------------------------------
// One 256-way scatter pass.  First pass: the keys d_keys[0, min(*d_n, n_max)) to the coarse regions (or straight to the leaves).
// Second pass: the keys of every coarse region to its 256 leaves; workgroup b takes tile b % tiles_per_region of region
// b / tiles_per_region.  cursor[d] counts what digit d's region has been asked to hold, dst_cap slots each.
template <bool SECOND>
__global__ __launch_bounds__(256) void us_scatter_kernel(const UsPlan p, const uint64_t* __restrict__ src,
                                                         const unsigned long long* __restrict__ d_n, uint64_t n_max,
                                                         const uint32_t* __restrict__ src_cursor, uint32_t tiles_per_region,
                                                         uint32_t* __restrict__ cursor, uint64_t* __restrict__ dst, uint64_t dst_cap,
                                                         uint32_t* __restrict__ d_fellback) {
    __shared__ uint32_t hist[US_FANOUT];
    __shared__ uint32_t base[US_FANOUT];
    uint64_t region = 0, begin, n;
    if (!SECOND) {
        n = us_count(d_n, n_max);
        begin = (uint64_t)blockIdx.x * US_TILE;
    } else {
        // (this pass raises the flag too: one lane reads it for the whole workgroup, or some lanes would miss the barriers below)
        __shared__ uint32_t quit;
        if (threadIdx.x == 0) quit = *d_fellback;
        __syncthreads();
        if (quit) return;
        region = blockIdx.x / tiles_per_region;
        const uint64_t held = src_cursor[region];
        n = held < p.region_cap ? held : p.region_cap;
        begin = (uint64_t)(blockIdx.x % tiles_per_region) * US_TILE;
        src += region * p.region_cap;
        cursor += region * US_FANOUT;
        dst += region * US_FANOUT * dst_cap;
    }
    if (begin >= n) return;
    hist[threadIdx.x] = 0;
    __syncthreads();
    constexpr int E = US_TILE / 256;
    uint64_t key[E];
    uint32_t digit[E], rank[E];
    bool stray = false;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint64_t i = begin + (uint64_t)e * 256 + threadIdx.x;
        digit[e] = US_FANOUT;
        rank[e] = 0;
        key[e] = 0;
        if (i < n) {
            key[e] = src[i];
            digit[e] = SECOND ? us_digit_second(p, region, key[e]) : us_digit_first(p, key[e]);
            if (digit[e] < US_FANOUT) rank[e] = atomicAdd(&hist[digit[e]], 1u);
            else stray = true;
        }
    }
    if (stray) atomicOr(d_fellback, 1u);
    __syncthreads();
    {
        const uint32_t c = hist[threadIdx.x];
        uint32_t b = NO_BASE;
        if (c) {
            const uint32_t at = atomicAdd(&cursor[threadIdx.x], c);
            if (us_reserve_ok(at, c, dst_cap)) b = at;
            else atomicOr(d_fellback, 1u);
        }
        base[threadIdx.x] = b;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (digit[e] >= US_FANOUT) continue;
        const uint32_t b = base[digit[e]];
        if (b != NO_BASE) dst[(uint64_t)digit[e] * dst_cap + b + rank[e]] = key[e];
    }
}

// one workgroup per leaf: sort, drop duplicates, distinct keys back to the head of the leaf's region
__global__ __launch_bounds__(256) void us_leaf_kernel(uint32_t shift, const uint32_t* __restrict__ cursor, uint64_t* __restrict__ leaves,
                                                      uint32_t* __restrict__ leaf_counts, uint32_t* __restrict__ leaf_distinct,
                                                      const uint32_t* __restrict__ d_fellback) {
    __shared__ uint64_t s[US_LEAF_CAP];
    __shared__ uint32_t bins[US_LEAF_BINS + 1];
    __shared__ uint32_t scan[256 / 64];
    if (*d_fellback) return;
    const uint64_t leaf = blockIdx.x;
    const uint32_t held = cursor[leaf];
    const uint32_t n = held < US_LEAF_CAP ? held : US_LEAF_CAP;
    uint64_t* mine = leaves + leaf * US_LEAF_CAP;
    us_sort_keys<256, US_LEAF_CAP / 256, US_LEAF_BINS, true>(mine, n, shift, s, bins, scan);
    const uint32_t total = us_unique_write<256, US_LEAF_CAP / 256, uint32_t>(s, n, scan, mine,
                                                                            leaf_counts ? leaf_counts + leaf * US_LEAF_CAP : nullptr);
    if (threadIdx.x == 0) leaf_distinct[leaf] = total;
}

// offsets[l] = distinct keys in front of leaf l, offsets[L] = *d_n_out = all of them; one workgroup
__global__ __launch_bounds__(1024) void us_scan_kernel(const uint32_t* __restrict__ leaf_distinct, uint32_t n_leaves,
                                                       uint32_t* __restrict__ offsets, uint64_t* __restrict__ d_n_out,
                                                       const uint32_t* __restrict__ d_fellback) {
    __shared__ uint32_t wsum[1024 / 64];
    if (*d_fellback) return;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_leaves; base += 4096) {      // 4 leaves per thread and trip
        const uint32_t l = base + threadIdx.x * 4;
        uint32_t v[4], sum = 0, total;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = l + i < n_leaves ? leaf_distinct[l + i] : 0;
            sum += v[i];
        }
        uint32_t at = carry + us_block_scan<1024>(sum, wsum, total);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (l + i < n_leaves) offsets[l + i] = at;
            at += v[i];
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        offsets[n_leaves] = carry;
        *d_n_out = carry;
    }
}

__global__ __launch_bounds__(256) void us_pack_kernel(const uint64_t* __restrict__ leaves, const uint32_t* __restrict__ leaf_counts,
                                                      const uint32_t* __restrict__ offsets, uint64_t* __restrict__ out,
                                                      uint64_t* __restrict__ counts, const uint32_t* __restrict__ d_fellback) {
    if (*d_fellback) return;
    const uint64_t leaf = blockIdx.x;
    const uint32_t at = offsets[leaf], n = offsets[leaf + 1] - at;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        out[at + i] = leaves[leaf * US_LEAF_CAP + i];
        if (counts) counts[at + i] = leaf_counts[leaf * US_LEAF_CAP + i];
    }
}

__global__ void us_report_kernel(const unsigned long long* __restrict__ d_n, const uint64_t* __restrict__ d_n_out,
                                 const uint32_t* __restrict__ d_fellback, uint64_t* __restrict__ report) {
    report[0] = *d_n;
    report[1] = *d_n_out;
    report[2] = *d_fellback;
}

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// the bucket form's workspace: [cursors: coarse regions, then leaves][distinct per leaf][offsets][coarse regions][leaf regions][counts]
struct UsLayout {
    size_t coarse_cursors, leaf_cursors, cursor_bytes, distinct, offsets, coarse, leaves, counts, total;
};
UsLayout us_layout(const UsPlan& p, bool counts) {
    UsLayout y{};
    const size_t n_leaf_cursors = p.form == US_TWO_PASS ? (size_t)p.regions * US_FANOUT : US_FANOUT;
    y.coarse_cursors = 0;
    y.leaf_cursors = up256(US_FANOUT * 4);
    y.cursor_bytes = y.leaf_cursors + up256(n_leaf_cursors * 4);
    y.distinct = y.cursor_bytes;
    y.offsets = y.distinct + up256(n_leaf_cursors * 4);
    y.coarse = y.offsets + up256((n_leaf_cursors + 1) * 4);
    y.leaves = y.coarse + up256((size_t)p.regions * p.region_cap * 8);
    y.counts = y.leaves + up256((size_t)p.leaves * US_LEAF_CAP * 8);          // (a key of [0, thr] has a leaf below p.leaves)
    y.total = y.counts + (counts ? up256((size_t)p.leaves * US_LEAF_CAP * 4) : 0);
    return y;
}

}  // namespace

size_t sort_unique_uniform_temp_bytes(uint64_t n_max, uint64_t thr, bool counts) {
    const UsPlan p = us_plan(n_max, thr);
    if (p.form == US_SMALL || p.form == US_DECLINE) return 256;
    return us_layout(p, counts).total;
}

// Over every thr.  The next larger shift did not fit, so a leaf expects 399 keys or more: leaves x 1,024 slots stay under 2.6 n_max.
// The coarse regions are sized for 256 full leaves each, and the last one may hold a single leaf: with 257 leaves, two regions of
// n_max slots each; 1.5 n_max with three regions, less with more.  The cursor, count and offset arrays are 12 bytes per leaf.
size_t sort_unique_uniform_temp_bound(uint64_t n_max, bool counts) {
    if (n_max <= US_SMALL_MAX) return 256;
    return up256((size_t)n_max * 8 * 5 + (counts ? (size_t)n_max * 4 * 3 : 0) + ((size_t)8 << 20));
}

uint32_t sort_unique_uniform_form(uint64_t n_max, uint64_t thr, size_t temp_bytes, bool counts) {
    const UsPlan p = us_plan(n_max, thr);
    if (p.form == US_SMALL || p.form == US_DECLINE) return p.form;
    return temp_bytes < us_layout(p, counts).total ? (uint32_t)US_DECLINE : p.form;
}

hipError_t sort_unique_uniform(const uint64_t* d_keys, const unsigned long long* d_n, uint64_t n_max, uint64_t thr, uint64_t* d_out,
                               uint64_t* d_counts, uint64_t* d_n_out, uint32_t* d_fellback, void* d_temp, size_t temp_bytes,
                               hipStream_t stream) {
    const UsPlan p = us_plan(n_max, thr);
    const uint32_t form = sort_unique_uniform_form(n_max, thr, temp_bytes, d_counts != nullptr);
    if (form == US_SMALL) {
        hipLaunchKernelGGL(us_small_kernel, dim3(1), dim3(1024), 0, stream, d_keys, d_n, n_max, us_small_shift(thr), d_out, d_counts, d_n_out,
                           d_fellback);
        return hipGetLastError();
    }
    if (form == US_DECLINE) return hipMemsetD32Async((hipDeviceptr_t)d_fellback, 1, 1, stream);
    const UsLayout y = us_layout(p, d_counts != nullptr);
    char* base = (char*)d_temp;
    uint32_t* coarse_cursors = (uint32_t*)(base + y.coarse_cursors);
    uint32_t* leaf_cursors = (uint32_t*)(base + y.leaf_cursors);
    uint32_t* distinct = (uint32_t*)(base + y.distinct);
    uint32_t* offsets = (uint32_t*)(base + y.offsets);
    uint64_t* coarse = (uint64_t*)(base + y.coarse);
    uint64_t* leaves = (uint64_t*)(base + y.leaves);
    uint32_t* leaf_counts = d_counts ? (uint32_t*)(base + y.counts) : nullptr;
    hipError_t e = hipMemsetAsync(d_fellback, 0, 4, stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(base, 0, y.cursor_bytes, stream);
    if (e != hipSuccess) return e;
    const uint32_t tiles = (uint32_t)((n_max + US_TILE - 1) / US_TILE);
    if (form == US_ONE_PASS) {
        hipLaunchKernelGGL(us_scatter_kernel<false>, dim3(tiles), dim3(256), 0, stream, p, d_keys, d_n, n_max, (const uint32_t*)nullptr, 1u,
                           leaf_cursors, leaves, (uint64_t)US_LEAF_CAP, d_fellback);
    } else {
        hipLaunchKernelGGL(us_scatter_kernel<false>, dim3(tiles), dim3(256), 0, stream, p, d_keys, d_n, n_max, (const uint32_t*)nullptr, 1u,
                           coarse_cursors, coarse, p.region_cap, d_fellback);
        const uint32_t tpr = (uint32_t)((p.region_cap + US_TILE - 1) / US_TILE);
        hipLaunchKernelGGL(us_scatter_kernel<true>, dim3((uint32_t)p.regions * tpr), dim3(256), 0, stream, p, (const uint64_t*)coarse, d_n,
                           n_max, (const uint32_t*)coarse_cursors, tpr, leaf_cursors, leaves, (uint64_t)US_LEAF_CAP, d_fellback);
    }
    const uint32_t L = (uint32_t)p.leaves;
    hipLaunchKernelGGL(us_leaf_kernel, dim3(L), dim3(256), 0, stream, p.shift, (const uint32_t*)leaf_cursors, leaves, leaf_counts, distinct,
                       (const uint32_t*)d_fellback);
    hipLaunchKernelGGL(us_scan_kernel, dim3(1), dim3(1024), 0, stream, (const uint32_t*)distinct, L, offsets, d_n_out,
                       (const uint32_t*)d_fellback);
    hipLaunchKernelGGL(us_pack_kernel, dim3(L), dim3(256), 0, stream, (const uint64_t*)leaves, (const uint32_t*)leaf_counts,
                       (const uint32_t*)offsets, d_out, d_counts, (const uint32_t*)d_fellback);
    return hipGetLastError();
}

hipError_t sort_report_launch(const unsigned long long* d_n, const uint64_t* d_n_out, const uint32_t* d_fellback, uint64_t* d_report,
                              hipStream_t stream) {
    hipLaunchKernelGGL(us_report_kernel, dim3(1), dim3(1), 0, stream, d_n, d_n_out, d_fellback, d_report);
    return hipGetLastError();
}

}  // namespace smg
