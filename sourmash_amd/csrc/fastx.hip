// fastx.hip -- FASTA / FASTQ record structure resolved on the GPU.
//
// The reference parses sequence files on the host, one record at a time (screed / needletail:
// src/sourmash/command_sketch.py:697,746-768, src/core/benches/compute.rs:35-38).  Here the host only moves raw
// file bytes into HBM; which bytes are sequence is decided on the device at memory bandwidth:
//   state      per byte, the kind of line it is on.  FASTA: the kind of the most recent line start (1 = sequence line, 2 = header
//              line: it starts with '>'); FASTQ: the number of line starts so far mod 4 (line 0 of every 4 is the header, line 1 the
//              sequence).
//   keep       a byte stays if it is on a sequence line and is not CR/LF, or if it is the first byte of a header
//              line ('>' / '@'): that one remains in the stream as the record separator -- it is outside ACGT, so
//              it kills exactly the k-mers that would span two records, which is what one add_sequence call per
//              record achieves
//   compact    order preserving, over 8 KiB blocks.
// Round 6: three launches, none of them per byte.  Rounds 1-5 ran a byte-wise rocPRIM scan for the states (one state byte written
// and read twice per input byte: 46 us of the 87 us a 4.6 MB genome's parse took).  A block's states depend on what lies in front
// of it only through ONE value -- the state of the byte before the block -- so
//   fx_summary_kernel   per block: what it does to that value (FASTA: the kind of its last line start, if any; FASTQ: its number of
//                       line starts) and its kept bytes and header lines as a function of it (FASTA: the part before the block's
//                       first line start counts only on a sequence line; FASTQ: one count per phase 0 .. 3);
//   fx_offsets_kernel   one workgroup walks the summaries: every block's entry state, kept bytes -> output offset, the records, the
//                       carry for the next piece;
//   fx_scatter_kernel   every block recomputes its flags from its entry state, compacts itself in LDS and writes its bytes out
//                       contiguously.
// Chunks are chained through a 4-byte carry (state of the last byte, "ended on a newline"), so a file streams through in pieces
// of any size.
#include <hip/hip_runtime.h>
#include <cstring>
#include "fastx_api.hpp"
#include "fastx_core.hpp"

namespace smg {

namespace {

// BlockSum, LaneBits, the per-lane masks, the fold rules and the per-block step: fastx_core.hpp (shared with the host emulation)

// exclusive scan over the workgroup's lanes: FASTA "last non-zero", FASTQ sum.  *total: the inclusive value of the last lane.
template <bool LASTNZ>
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl = fx_fold<LASTNZ>(o, incl);
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < FX_THREADS / 64; ++w) {
        const uint32_t x = s_wave[w];
        if (w < wave) before = fx_fold<LASTNZ>(before, x);
        all = fx_fold<LASTNZ>(all, x);
    }
    *total = all;
    uint32_t prev = __shfl_up(incl, 1);                          // inclusive value of the lane in front
    if (lane == 0) prev = 0u;
    return fx_fold<LASTNZ>(before, prev);
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* s_red) {        // -> thread 0 holds the sum
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    if (threadIdx.x == 0) for (int w = 0; w < FX_THREADS / 64; ++w) t += s_red[w];
    return t;
}

__global__ __launch_bounds__(FX_THREADS) void fx_summary_kernel(const uint8_t* __restrict__ raw, uint64_t n, int fastq,
                                                                 const uint8_t* __restrict__ carry, BlockSum* __restrict__ sums) {
    __shared__ uint32_t s_wave[FX_THREADS / 64], s_red[FX_THREADS / 64];
    const uint64_t base = (uint64_t)blockIdx.x * FX_BLOCK_BYTES + (uint64_t)threadIdx.x * FX_PER_THREAD;
    uint8_t bytes[FX_PER_THREAD];
    const LaneBits b = lane_bits(raw, base, n, carry[1], bytes);
    BlockSum out{};
    if (!fastq) {
        uint32_t m1, m2, kind, last;
        fasta_masks(b, &m1, &m2, &kind);
        const uint32_t inh = block_excl<true>(kind, s_wave, &last);
        const uint32_t local = inh == 1 ? __popc(m1) : __popc(m2);
        const uint32_t pre = inh == 0 ? __popc(m1 & ~m2) : 0u;
        const uint32_t c0 = block_sum(local, s_red), c1 = block_sum(pre, s_red), h = block_sum(__popc(b.ls & b.gt), s_red);
        out.cnt[0] = c0; out.cnt[1] = c1; out.hdr[0] = h; out.last_kind = last;
    } else {
        uint32_t M[4], all;
        fastq_classes(b, M);
        const uint32_t r = block_excl<false>(__popc(b.ls), s_wave, &all);
        uint32_t cq[4], hq[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) { uint32_t hm; cq[q] = __popc(fastq_keep(b, M, q, &hm)); hq[q] = __popc(hm); }
#pragma unroll
        for (uint32_t p = 0; p < 4; ++p) {
            const uint32_t q = (p + r) & 3u;
            const uint32_t c = q == 0 ? cq[0] : q == 1 ? cq[1] : q == 2 ? cq[2] : cq[3];
            const uint32_t h = q == 0 ? hq[0] : q == 1 ? hq[1] : q == 2 ? hq[2] : hq[3];
            out.cnt[p] = block_sum(c, s_red);
            out.hdr[p] = block_sum(h, s_red);
        }
        out.starts = all;
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = out;
}

// one workgroup: entry state and output offset of every block, totals, the next piece's carry
__global__ __launch_bounds__(FX_SPANS) void fx_offsets_kernel(const BlockSum* __restrict__ sums, unsigned n_blocks, int fastq,
                                                          const uint8_t* __restrict__ raw, uint64_t n, const uint8_t* __restrict__ carry,
                                                          uint8_t* __restrict__ carry_out, uint8_t* __restrict__ entry,
                                                          unsigned long long* __restrict__ block_off, unsigned long long* __restrict__ total,
                                                          unsigned long long* __restrict__ n_records,
                                                          unsigned long long* __restrict__ block_rec) {
    __shared__ unsigned long long part[FX_SPANS];
    __shared__ uint32_t st[FX_SPANS];
    const unsigned per = (n_blocks + FX_SPANS - 1) / FX_SPANS;
    const unsigned lo = threadIdx.x * per, hi = lo + per < n_blocks ? lo + per : n_blocks;
    // what this thread's span does to the state
    uint32_t eff = 0;
    for (unsigned i = lo; i < hi; ++i) {
        if (fastq) eff = fx_fold<false>(eff, sums[i].starts);
        else eff = fx_fold<true>(eff, sums[i].last_kind);
    }
    st[threadIdx.x] = eff;
    __syncthreads();
    for (int d = 1; d < FX_SPANS; d <<= 1) {                         // Hillis-Steele inclusive scan of the spans' effects
        const uint32_t mine = st[threadIdx.x];
        const uint32_t v = threadIdx.x >= (unsigned)d ? st[threadIdx.x - d] : 0;
        __syncthreads();
        st[threadIdx.x] = fastq ? fx_fold<false>(v, mine) : fx_fold<true>(v, mine);
        __syncthreads();
    }
    const uint32_t before = threadIdx.x ? st[threadIdx.x - 1] : 0u;
    uint32_t e = fx_entry_state(fastq, carry, before);
    unsigned long long kept = 0, recs = 0;
    for (unsigned i = lo; i < hi; ++i) {                          // the per-block step (fastx_core.hpp)
        const BlockSum* s = sums + i;
        entry[i] = (uint8_t)e;
        if (fastq) fx_block_step<true>(s, e, kept, recs); else fx_block_step<false>(s, e, kept, recs);
    }
    if (hi == n_blocks && lo < hi) {                             // the thread that owns the last block: the carry
        carry_out[0] = (uint8_t)e;
        carry_out[1] = fx_ended_on_lf(raw[n - 1]);
    }
    part[threadIdx.x] = kept;
    __syncthreads();
    for (int d = 1; d < FX_SPANS; d <<= 1) {
        const unsigned long long v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (unsigned i = lo; i < hi; ++i) {
        const BlockSum* s = sums + i;
        const uint32_t ei = entry[i];
        block_off[i] = run;
        run += fx_block_kept(s, fastq, ei);
    }
    if (threadIdx.x == FX_SPANS - 1) *total = part[FX_SPANS - 1];
    // records: a sum over the threads through the same scratch
    __syncthreads();
    part[threadIdx.x] = recs;
    __syncthreads();
    for (int d = FX_SPANS / 2; d > 0; d >>= 1) {
        if (threadIdx.x < (unsigned)d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(n_records, part[0]);
    if (!block_rec) return;
    // block_rec[i] = header lines in front of block i (the ordinal of its first record): one more prefix over the same scratch
    __syncthreads();
    part[threadIdx.x] = recs;
    __syncthreads();
    for (int d = 1; d < FX_SPANS; d <<= 1) {
        const unsigned long long v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long ord = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (unsigned i = lo; i < hi; ++i) {
        block_rec[i] = ord;
        ord += fx_block_records(sums + i, fastq, entry + i);
    }
}

// every block: flags from its entry state, compacted in LDS, written out contiguously
__global__ __launch_bounds__(FX_THREADS) void fx_scatter_kernel(const uint8_t* __restrict__ raw, uint64_t n, int fastq,
                                                                 const uint8_t* __restrict__ carry, const uint8_t* __restrict__ entry,
                                                                 const unsigned long long* __restrict__ block_off, uint8_t* __restrict__ out,
                                                                 const unsigned long long* __restrict__ block_rec,
                                                                 unsigned long long* __restrict__ rec_starts, uint64_t rec_cap) {
    __shared__ uint8_t s_out[FX_BLOCK_BYTES];
    __shared__ uint32_t s_wave[FX_THREADS / 64];
    const uint64_t base = (uint64_t)blockIdx.x * FX_BLOCK_BYTES + (uint64_t)threadIdx.x * FX_PER_THREAD;
    uint8_t bytes[FX_PER_THREAD];
    const LaneBits b = lane_bits(raw, base, n, carry[1], bytes);
    const uint32_t e = entry[blockIdx.x];
    uint32_t mask, dummy, hdr;                                   // hdr: the kept header bytes among mask
    if (!fastq) {
        uint32_t m1, m2, kind;
        fasta_masks(b, &m1, &m2, &kind);
        const uint32_t inh = block_excl<true>(kind, s_wave, &dummy);
        mask = (inh ? inh : e) == 1u ? m1 : m2;
        hdr = b.ls & b.gt;
    } else {
        uint32_t M[4];
        fastq_classes(b, M);
        const uint32_t r = block_excl<false>(__popc(b.ls), s_wave, &dummy);
        mask = fastq_keep(b, M, (e + r) & 3u, &hdr);
    }
    const uint32_t cnt = __popc(mask);
    __syncthreads();                                             // s_wave is reused
    uint32_t total;
    unsigned pos = block_excl<false>(cnt, s_wave, &total);
    if (rec_starts) {                                            // the j-th record starts just behind the j-th kept header byte
        __syncthreads();
        unsigned long long ord = block_rec[blockIdx.x] + block_excl<false>(__popc(hdr), s_wave, &dummy);
        const unsigned long long at = block_off[blockIdx.x] + pos;
        for (uint32_t h = hdr; h; h &= h - 1u, ++ord) {
            const uint32_t below = (h & (0u - h)) - 1u;
            if (ord < rec_cap) rec_starts[ord] = fx_record_start(at, mask, below);
        }
    }
#pragma unroll
    for (int j = 0; j < FX_PER_THREAD; ++j)
        if (mask & (1u << j)) s_out[pos++] = bytes[j];
    __syncthreads();
    uint8_t* dst = out + block_off[blockIdx.x];
    for (unsigned i = threadIdx.x; i < total; i += FX_THREADS) dst[i] = s_out[i];
}

// dst[j] = last H bytes of (old halo ++ the n new bytes at src); src[-H .. -1] is the old halo
__global__ void halo_kernel(const uint8_t* __restrict__ src, const unsigned long long* __restrict__ n_new, int H,
                            uint8_t* __restrict__ dst) {
    const long long n = (long long)*n_new;
    for (int j = threadIdx.x; j < H; j += blockDim.x) dst[j] = src[n + j - H];
}

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

}  // namespace

// temp layout: [block summaries][entry states u8][block offsets u64]
size_t fastx_temp_bytes(uint64_t max_chunk) {
    const uint64_t n_blocks = (max_chunk + FX_BLOCK_BYTES - 1) / FX_BLOCK_BYTES + 1;
    return align256(n_blocks * sizeof(BlockSum)) + align256(n_blocks) + align256(n_blocks * 8) + 256;
}
// ... and with the record starts: [first record ordinal of every block u64] behind it
size_t fastx_records_temp_bytes(uint64_t max_chunk) {
    const uint64_t n_blocks = (max_chunk + FX_BLOCK_BYTES - 1) / FX_BLOCK_BYTES + 1;
    return fastx_temp_bytes(max_chunk) + align256(n_blocks * 8);
}

// d_state: unused since round 6 (the per-byte states are never materialised); kept in the signature for the callers' scratch layout
hipError_t fastx_compact_launch(const uint8_t* d_raw, uint64_t n, int fastq, uint8_t* d_carry, uint8_t* d_state,
                                uint8_t* d_out, unsigned long long* d_n_out, unsigned long long* d_n_records,
                                void* d_temp, size_t temp_bytes, hipStream_t stream, bool last_piece,
                                unsigned long long* d_record_starts, uint64_t record_cap) {
    (void)d_state;
    if (n == 0) return hipMemsetAsync(d_n_out, 0, 8, stream);
    if (temp_bytes < (d_record_starts ? fastx_records_temp_bytes(n) : fastx_temp_bytes(n))) return hipErrorInvalidValue;
    const uint64_t n_blocks = (n + FX_BLOCK_BYTES - 1) / FX_BLOCK_BYTES;
    if (n_blocks > 0x7fffffffull) return hipErrorInvalidValue;
    BlockSum* sums = reinterpret_cast<BlockSum*>(d_temp);
    uint8_t* entry = reinterpret_cast<uint8_t*>((char*)d_temp + align256((n_blocks + 1) * sizeof(BlockSum)));
    unsigned long long* block_off = reinterpret_cast<unsigned long long*>((char*)entry + align256(n_blocks + 1));
    unsigned long long* block_rec = d_record_starts ? reinterpret_cast<unsigned long long*>((char*)d_temp + fastx_temp_bytes(n)) : nullptr;
    // the carry is read (first byte) and rewritten (last byte) by the same launches: go through a second slot
    hipLaunchKernelGGL(fx_summary_kernel, dim3((unsigned)n_blocks), dim3(FX_THREADS), 0, stream, d_raw, n, fastq, d_carry, sums);
    hipLaunchKernelGGL(fx_offsets_kernel, dim3(1), dim3(FX_SPANS), 0, stream, (const BlockSum*)sums, (unsigned)n_blocks, fastq, d_raw, n, d_carry,
                       d_carry + 2, entry, block_off, d_n_out, d_n_records, block_rec);
    hipLaunchKernelGGL(fx_scatter_kernel, dim3((unsigned)n_blocks), dim3(FX_THREADS), 0, stream, d_raw, n, fastq, d_carry, (const uint8_t*)entry,
                       (const unsigned long long*)block_off, d_out, (const unsigned long long*)block_rec, d_record_starts, record_cap);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || last_piece) return e;
    return hipMemcpyAsync(d_carry, d_carry + 2, 2, hipMemcpyDeviceToDevice, stream);
}

hipError_t fastx_halo_launch(const uint8_t* d_src, const unsigned long long* d_n_new, int halo, uint8_t* d_dst,
                             hipStream_t stream) {
    if (halo <= 0) return hipSuccess;
    hipLaunchKernelGGL(halo_kernel, dim3(1), dim3(256), 0, stream, d_src, d_n_new, halo, d_dst);
    return hipGetLastError();
}

}  // namespace smg
