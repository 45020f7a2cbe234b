// hll.hip -- HyperLogLog registers on the GPU (sketch/hyperloglog/mod.rs: add_sequence = SigsTrait::add_sequence over add_hash).
//
// The hot loop is the sketch kernel's (sketch_kernel.hpp / kmer_core.hpp): canonical k-mer -> MurmurHash3 (seed 42) for
// every start position of a stretch; only the sink differs.  Instead of keeping hashes under a threshold, every hash h != 0
// updates one register: reg[h & (2^p - 1)] = max(reg, clz64(h >> p) + 1 - p).  Ranks are geometric (rank r with probability
// 2^-r), so after the first few thousand k-mers nearly every update is a read that finds a value at least as large.
//
//   p <= 14: each workgroup keeps its own register file in LDS (one u32 per register: ds_max_u32 is native; 64 KiB at p = 14)
//            and folds it into the device array at the end (read, atomicMax only where larger).  The grid is sized so that
//            the fold -- 2^p checks per workgroup -- stays a small share of the hashing (tile_launch.hpp: lds_grid).
//   p >= 15: the LDS file would cost occupancy; the update goes to the device array (at most 1 MiB, L2 resident) behind a
//            read filter.
// Device registers are u32 (atomicMax has no byte form); hll_pack_launch narrows them to the u8 layout of the host container.
//
// k = 1 .. 88 take the fused kernel (hll_dense.hip, six parts).  Longer k-mers (up to sketch_dna_max_k()) take the run-time-k
// walk's per-position output (kmer_hashes_launch) in bounded chunks, folded by hll_hashes_kernel.
//
// Roofline: like the sketch kernel, bound by VALU integer issue (12 64-bit multiplies per k-mer); the input is 1 B/base.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "arena.hpp"
#include "device_api.hpp"
#include "hll_kernel.hpp"

namespace smg {

// fold a u64 hash array into the registers (skip_zero: hash 0 marks "no k-mer here" in a per-position array)
__global__ __launch_bounds__(SK_BLOCK) void hll_hashes_kernel(const uint64_t* __restrict__ hashes, uint64_t n, uint32_t p,
                                                              uint32_t* regs, int skip_zero) {
    const uint64_t mask = ((uint64_t)1 << p) - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * SK_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SK_BLOCK) {
        const uint64_t h = hashes[i];
        if (skip_zero && h == 0) continue;
        const uint32_t idx = (uint32_t)(h & mask);
        const uint32_t r = hll_rank(h, p);
        if (regs[idx] < r) atomicMax(&regs[idx], r);
    }
}

__global__ __launch_bounds__(SK_BLOCK) void hll_pack_kernel(const uint32_t* __restrict__ regs, uint32_t n, uint8_t* __restrict__ out) {
    for (uint32_t i = blockIdx.x * SK_BLOCK + threadIdx.x; i < n; i += gridDim.x * SK_BLOCK) out[i] = (uint8_t)regs[i];
}

hipError_t hll_hashes_launch(const uint64_t* d_hashes, uint64_t n, uint32_t p, uint32_t* d_regs, bool skip_zero, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t nb = (n + SK_BLOCK - 1) / SK_BLOCK;
    const unsigned grid = (unsigned)(nb < 2048 ? nb : 2048);
    hipLaunchKernelGGL(hll_hashes_kernel, dim3(grid), dim3(SK_BLOCK), 0, stream, d_hashes, n, p, d_regs, skip_zero ? 1 : 0);
    return hipGetLastError();
}

hipError_t hll_pack_launch(const uint32_t* d_regs, uint32_t n, uint8_t* d_out, hipStream_t stream) {
    const uint32_t nb = (n + SK_BLOCK - 1) / SK_BLOCK;
    hipLaunchKernelGGL(hll_pack_kernel, dim3(nb < 1024 ? nb : 1024), dim3(SK_BLOCK), 0, stream, d_regs, n, d_out);
    return hipGetLastError();
}

hipError_t hll_dna_launch(const uint8_t* d_seq, uint64_t len, uint32_t k, uint32_t p, uint32_t* d_regs, hipStream_t stream) {
    if (k == 0 || len < k) return hipSuccess;
    if (p < 4 || p > 18) return hipErrorInvalidValue;
    if (k <= (uint32_t)SK_FAST_MAX_K) return launcher<HllLaunch>(k)(d_seq, len, p, d_regs, stream);
    if (k > sketch_dna_max_k()) return hipErrorInvalidValue;
    // per-position hashes of up to CHUNK k-mers at a time (8 B each), then the fold
    constexpr uint64_t CHUNK = (uint64_t)16 << 20;
    const uint64_t nk = len - k + 1;
    const uint64_t cap = nk < CHUNK ? nk : CHUNK;
    void* tmp = nullptr;
    hipError_t e = arena_alloc(&tmp, cap * 8, stream);
    if (e != hipSuccess) return e;
    uint64_t* d_h = static_cast<uint64_t*>(tmp);
    for (uint64_t off = 0; off < nk && e == hipSuccess; off += CHUNK) {
        const uint64_t n = nk - off < CHUNK ? nk - off : CHUNK;
        e = hipMemsetAsync(d_h, 0, n * 8, stream);
        if (e == hipSuccess) e = kmer_hashes_launch(d_seq + off, n + k - 1, k, HLL_SEED, d_h, n, stream);
        if (e == hipSuccess) e = hll_hashes_launch(d_h, n, p, d_regs, true, stream);
    }
    arena_free(tmp, stream);
    return e;
}

}  // namespace smg
