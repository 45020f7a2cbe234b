// sketch_multi.hip -- several ksizes of one DNA stretch in ONE pass (round 6).
//
// What the reference does here: Signature::add_sequence hands every k-mer window to each of the signature's sketches in turn
// (src/core/src/signature.rs:661-677: one SeqToHashes walk per ksize).  sketch.hip runs one launch per ksize, which costs nothing
// on long inputs -- everything after the staging of the bytes depends on k (both strands' words, the canonical compare,
// MurmurHash3: 112 of the 116 instructions a k-mer costs at k = 31) -- but a single genome is 4.6 MB: three launches of ~30-50 us
// each where the work is ~55 us.  Here a tile's bytes are staged once, every lane pulls the window of the LARGEST ksize into
// registers, and process_lane<K> (kmer_core.hpp: the same code as the per-ksize kernels) runs for each ksize on the window's
// prefix, each with its own LDS list of kept hashes and its own output.  Instantiated for the ksize sets listed at the end
// (21 / 31 / 51: the standard set of `sourmash sketch dna -p k=21,k=31,k=51`); any other set takes the per-ksize launches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketch_kernel.hpp"
#include "device_api.hpp"

namespace smg {

namespace {

constexpr int SM_N = 3;              // ksizes per pass
constexpr int SM_OUT_CAP = 1024;     // LDS staging entries for kept hashes, per ksize (8 KiB each)

// The largest ksize keeps the plain 64-bit constant multiply (murmur3.hpp, mul_c64<C, PLAIN>): with the limb form in all three the
// kernel no longer fits the 168 registers of 3 waves per SIMD (2 spilled, 12 bytes of scratch per lane at 21 / 31 / 51).
constexpr bool SM_PLAIN_MUL_LAST = true;

struct MultiArgs {
    uint64_t thr[SM_N];
    uint64_t* out[SM_N];
    unsigned long long* count[SM_N];
    uint64_t cap[SM_N];
    uint32_t start[SM_N];            // k-mers of ksize j start at positions >= start[j] of the (aligned) buffer: in front of that lies
                                     // the halo of a LONGER ksize, whose k-mers of this size the previous piece has hashed already
};

template <int KA, int KB, int KC>
__global__ __launch_bounds__(SK_BLOCK) __attribute__((amdgpu_waves_per_eu(3, 8))) void sketch_dna_multi_kernel(const uint8_t* __restrict__ seq, uint64_t len, uint64_t seed, MultiArgs a,
                                                                    uint64_t n_tiles, uint32_t skip) {
    static_assert(KA < KB && KB < KC, "ascending ksizes: the window of the last one holds the others'");
    constexpr int P = 16;
    using T = TileGeom<KC, P, SK_BLOCK>;
    constexpr int TILE = T::TILE, LANE_RD = T::LANE_RD, IN_CHUNKS = T::IN_CHUNKS;
    __shared__ __attribute__((aligned(16))) uint32_t s_in[IN_CHUNKS * 4];
    __shared__ uint64_t s_out[SM_N][SM_OUT_CAP];
    __shared__ unsigned int s_cnt[SM_N];
    __shared__ unsigned long long s_base[SM_N];
    using Sink = LdsSink<SM_OUT_CAP, SK_BLOCK>;
    const Sink sink[SM_N] = {Sink{{s_out[0]}, &s_cnt[0], &s_base[0], {a.out[0]}, a.count[0], a.cap[0]},
                             Sink{{s_out[1]}, &s_cnt[1], &s_base[1], {a.out[1]}, a.count[1], a.cap[1]},
                             Sink{{s_out[2]}, &s_cnt[2], &s_base[2], {a.out[2]}, a.count[2], a.cap[2]}};
    const int tid = threadIdx.x;
    if (tid < SM_N) s_cnt[tid] = 0;

    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t base = tile * (uint64_t)TILE;
        __syncthreads();
        stage_tile<IN_CHUNKS, false, SK_BLOCK>(seq, base, len, skip, s_in, nullptr, nullptr);
        __syncthreads();
        uint32_t raw[LANE_RD];
        read_window<LANE_RD, P>(s_in, tid, raw);
        const uint64_t lane0 = base + (uint64_t)tid * P;
        auto keep = [&](int j, int o, uint64_t h) {
            if (lane0 + (uint64_t)o < (uint64_t)a.start[j]) return;        // hashed with the previous piece (see MultiArgs)
            sink[j].append(h);
        };
        // one ksize after the other on the same registers (a fence keeps the scheduler from interleaving three hash pipelines)
        // (the window passes through an empty asm between the phases: without it the compiler shares the upper-cased and
        //  complemented words of the three phases and overlaps their hash pipelines -- 219 registers, two waves per SIMD)
        auto fence = [&]() {
#pragma unroll
            for (int i = 0; i < LANE_RD; ++i) asm volatile("" : "+v"(raw[i]));
            __builtin_amdgcn_sched_barrier(0);
        };
        process_lane<KA, P, true>(raw, seed, a.thr[0], [&](int o, uint64_t h) { keep(0, o, h); });
        fence();
        process_lane<KB, P, true>(raw, seed, a.thr[1], [&](int o, uint64_t h) { keep(1, o, h); });
        fence();
        process_lane<KC, P, true, SM_PLAIN_MUL_LAST>(raw, seed, a.thr[2], [&](int o, uint64_t h) { keep(2, o, h); });
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SM_N; ++j) sink[j].flush(SM_OUT_CAP / 2);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SM_N; ++j) sink[j].flush(1);
}

template <int KA, int KB, int KC>
hipError_t launch_multi(const uint8_t* d_new, uint64_t n_new, uint64_t seed, const SketchMultiOut* o, hipStream_t stream) {
    const TileSpan t = align_to_tiles(d_new - (KC - 1), (uint64_t)(KC - 1) + n_new, (uint64_t)SK_BLOCK * 16);
    if (t.n_tiles == 0) return hipSuccess;
    MultiArgs a;
    const int ks[SM_N] = {KA, KB, KC};
    for (int j = 0; j < SM_N; ++j) {
        a.thr[j] = o[j].thr; a.out[j] = o[j].out; a.count[j] = o[j].count; a.cap[j] = o[j].cap;
        a.start[j] = t.skip + (uint32_t)(KC - ks[j]);
    }
    hipLaunchKernelGGL((sketch_dna_multi_kernel<KA, KB, KC>), dim3(sk_grid(t.n_tiles)), dim3(SK_BLOCK), 0, stream, t.seq, t.len, seed,
                       a, t.n_tiles, t.skip);
    return hipGetLastError();
}

}  // namespace

bool sketch_dna_multi_supported(const uint32_t* ks, int n) { return n == 3 && ks[0] == 21 && ks[1] == 31 && ks[2] == 51; }

// d_new: the first NEW byte; the (largest k) - 1 bytes in front of it are readable and hold the stream's previous bytes (or
// separators); outs[j] belongs to ks[j], ascending.  hipErrorNotSupported: the caller launches per ksize.
hipError_t sketch_dna_multi_launch(const uint8_t* d_new, uint64_t n_new, const uint32_t* ks, int n, uint64_t seed, const SketchMultiOut* outs,
                                   hipStream_t stream) {
    if (!sketch_dna_multi_supported(ks, n)) return hipErrorNotSupported;
    if (n_new == 0) return hipSuccess;
    return launch_multi<21, 31, 51>(d_new, n_new, seed, outs, stream);
}

}  // namespace smg
