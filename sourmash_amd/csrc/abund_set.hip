// abund_set.hip -- the two passes an abundance column of a resident collection (capi_common.hpp: SketchSet::abunds) needs beside the
// set algebra (setops.hip): the check of a column that arrives from outside (its largest value, and the first position of a zero,
// which no stored abundance may be), and the per-row sums (MinHash.sum_abundances of every row).  Sums wrap in u64.
#include <hip/hip_runtime.h>
#include "device_api.hpp"

namespace smg {

namespace {

constexpr uint32_t ABUND_BLOCK = 256;

__device__ __forceinline__ uint64_t wave_shfl_down_u64(uint64_t v, uint32_t delta) {
    const uint32_t lo = __shfl_down((uint32_t)v, delta, 64), hi = __shfl_down((uint32_t)(v >> 32), delta, 64);
    return ((uint64_t)hi << 32) | lo;
}

// result[0] = the largest abundance, result[1] = the first position of a zero (the caller starts it at 2^64 - 1: none).  A lane
// walks the column with the grid's stride, a wave folds its lanes' answers by shuffles, and its first lane sends them on: two
// atomics a wave, on two words (max and min commute: the answer does not depend on the order).
__global__ __launch_bounds__(ABUND_BLOCK) void abund_check_kernel(const uint64_t* __restrict__ abunds, uint64_t total, unsigned long long* __restrict__ result) {
    uint64_t hi = 0, zero_at = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * ABUND_BLOCK + threadIdx.x; i < total; i += (uint64_t)gridDim.x * ABUND_BLOCK) {
        const uint64_t a = abunds[i];
        if (a > hi) hi = a;
        if (a == 0 && i < zero_at) zero_at = i;
    }
    for (uint32_t d = 32; d; d >>= 1) {
        const uint64_t h2 = wave_shfl_down_u64(hi, d), z2 = wave_shfl_down_u64(zero_at, d);
        if (h2 > hi) hi = h2;
        if (z2 < zero_at) zero_at = z2;
    }
    if ((threadIdx.x & 63u) == 0) {
        if (hi) atomicMax(&result[0], (unsigned long long)hi);
        if (zero_at != ~0ull) atomicMin(&result[1], (unsigned long long)zero_at);
    }
}

// sums[r] = the sum of row r's abundances: a wave a row, its lanes striding the row, one fold by shuffles
__global__ __launch_bounds__(ABUND_BLOCK) void abund_row_sums_kernel(const uint64_t* __restrict__ abunds, const uint64_t* __restrict__ offsets, uint64_t n,
                                                                     uint64_t* __restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (ABUND_BLOCK / 64);
    for (uint64_t r = (uint64_t)blockIdx.x * (ABUND_BLOCK / 64) + (threadIdx.x >> 6); r < n; r += waves) {
        const uint64_t lo = offsets[r], hi = offsets[r + 1];
        uint64_t s = 0;
        for (uint64_t i = lo + lane; i < hi; i += 64) s += abunds[i];
        for (uint32_t d = 32; d; d >>= 1) s += wave_shfl_down_u64(s, d);
        if (lane == 0) sums[r] = s;
    }
}

}  // namespace

hipError_t abund_check_launch(const uint64_t* d_abunds, uint64_t total, uint64_t* d_result, hipStream_t st) {
    static const uint64_t init[2] = {0ull, ~0ull};
    hipError_t e = hipMemcpyAsync(d_result, init, 16, hipMemcpyHostToDevice, st);
    if (e != hipSuccess || total == 0) return e;
    const uint64_t b = (total + ABUND_BLOCK - 1) / ABUND_BLOCK;
    hipLaunchKernelGGL(abund_check_kernel, dim3((unsigned)(b > 2048 ? 2048 : b)), dim3(ABUND_BLOCK), 0, st, d_abunds, total, (unsigned long long*)d_result);
    return hipGetLastError();
}

hipError_t abund_row_sums_launch(const uint64_t* d_abunds, const uint64_t* d_offsets, uint64_t n, uint64_t* d_sums, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uint64_t b = (n + ABUND_BLOCK / 64 - 1) / (ABUND_BLOCK / 64);
    hipLaunchKernelGGL(abund_row_sums_kernel, dim3((unsigned)(b > 65536 ? 65536 : b)), dim3(ABUND_BLOCK), 0, st, d_abunds, d_offsets, n, d_sums);
    return hipGetLastError();
}

}  // namespace smg
