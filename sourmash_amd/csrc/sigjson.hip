// sigjson.hip -- the hash arrays of signature JSON turned into u64 on the device.
//
// What the reference does here: serde_json deserialises every signature into a struct, `mins` into a Vec<u64>
// (src/core/src/signature.rs:569-659, src/core/src/sketch/minhash.rs:103-184); loading a collection of 10^4 - 10^5 sketches is
// digit parsing (~85 KB of decimal text per sketch of 5,000 hashes) on the host's cores.  Here the inflated JSON text stays in
// HBM (gunzip.hip leaves it there) and
//   sj_spans_kernel   a wavefront per document finds the `"mins":[ ... ]` and `"abundances":[ ... ]` arrays: where they begin and end,
//                     how many commas they hold, whether they hold anything but digits, commas and white space
//   sj_parse_kernel   a wavefront per `mins` array: the array is cut into 64 pieces, a prefix sum of the pieces' comma counts
//                     gives every number its index, every lane parses the numbers that begin in its piece; the values are
//                     checked for strictly ascending order (minhash.rs:161-171 sorts on load: such a document goes to the host) and
//                     counted against the down-sampling threshold
//   sj_take_bytes     everything OUTSIDE the arrays (a few hundred bytes a document) packed for the host, which reads the
//                     metadata with the same scanner as before (collection.hpp) -- the arrays replaced by their index
//   sj_take_u64       the kept prefix of every selected array -> its row of the CSR
// Anything unusual in an array (a float, a minus sign, unsorted or repeated values, more arrays than slots) flags the document
// and the host parses it as before: the result is the host's result or an error, never something else.
//
// The rules of both kernels -- the key match, the tile tallies, the chunk geometry, the number parser with its overflow and
// termination rules, the order pass -- are in sigjson_core.hpp, which also compiles for the host; here are the thread indices, the
// ballots, the prefix sum and the reduction.  tests/sigjson_cases.py holds a reference written from the rules and the named
// cases at every seam (lane, chunk, look-ahead, alignment, 2^64, keep_max, tile bits); tests/test_sigjson_core_cpu.py runs them
// through a host emulation (tests/native/sigjson_emul.cpp), tests/test_gpu_sigjson_edges.py through smgpu_sigjson_parse_raw.
#include <hip/hip_runtime.h>
#include "sigjson_api.hpp"

namespace smg {

namespace {

// first position >= from (< len) whose byte satisfies pred, by 64-byte tiles; len if none.  Uniform result.
template <class Pred>
__device__ __forceinline__ uint64_t find_first(const uint8_t* t, uint64_t from, uint64_t len, Pred pred) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t p = from; p < len; p += 64) {
        const uint64_t i = p + lane;
        const bool hit = i < len && pred(i);
        const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
        if (m) return p + (uint64_t)__builtin_ctzll(m);
    }
    return len;
}

__global__ __launch_bounds__(64) void sj_spans_kernel(const uint8_t* __restrict__ base, const SjDoc* __restrict__ docs, uint32_t n_docs,
                                                      SjSpan* __restrict__ spans, uint32_t* __restrict__ doc_flags) {
    const uint32_t d = blockIdx.x;
    if (d >= n_docs) return;
    const SjDoc doc = docs[d];
    const uint8_t* t = base + doc.off;
    const uint64_t len = doc.len;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n = 0, flags = 0;
    uint64_t pos = 0;
    while (pos < len) {
        // the next key that opens an array we take: "mins" or "abundances"
        const uint64_t m = find_first(t, pos, len, [&](uint64_t i) { return sj_key_at(t, i, len); });
        if (m >= len) break;
        const uint32_t kind = sj_key_kind(t, m);
        const uint64_t s = sj_array_begin(t, m + sj_key_len(kind), len);
        if (s > len) { pos = m + 1; continue; }
        // its end, its commas, and whether it holds anything but digits, commas and white space
        uint64_t e = len;
        SjTally tally = {0, 0, 0};
        for (uint64_t p = s; p < len; p += 64) {
            const SjByteClass c = sj_class_at(t, p + lane, len);
            const uint64_t close = __builtin_amdgcn_ballot_w64(c.close);
            sj_tile_fold(close, __builtin_amdgcn_ballot_w64(c.comma), __builtin_amdgcn_ballot_w64(c.digit), __builtin_amdgcn_ballot_w64(c.odd), tally);
            if (close) { e = p + (uint64_t)__builtin_ctzll(close); break; }
        }
        if (e >= len) { flags |= SJ_DOC_ODD; break; }                 // no closing bracket
        if (n >= SJ_MAX_SPANS) { flags |= SJ_DOC_ODD; break; }
        if (lane == 0) spans[(uint64_t)d * SJ_MAX_SPANS + n] = sj_span_record(s, e, kind, tally);
        ++n;
        pos = e + 1;
    }
    if (lane == 0) doc_flags[d] = flags | n;
}

// A wavefront per array.  The text goes through LDS 4 KB at a time (coalesced 16-byte loads; a lane reading its own stretch of
// the array byte by byte from HBM was one dependent trip to memory per byte: 17 ms for 6,000 arrays): lane l owns bytes
// [64 l, 64 l + 64) of the chunk, counts its commas, a prefix sum gives every number its index, and the
// lane parses the numbers that begin behind its commas -- they may run on into the next lane's bytes or the 64 bytes read
// beyond the chunk.  Order and the down-sampling count are taken from the written values afterwards.
__global__ __launch_bounds__(64) void sj_parse_kernel(const uint8_t* __restrict__ base, const SjParse* __restrict__ jobs, uint32_t n_jobs,
                                                      uint64_t* __restrict__ values, SjParsed* __restrict__ results, uint64_t keep_max) {
    __shared__ uint4 buf4[SJ_BUF_LINES];
    uint8_t* buf = reinterpret_cast<uint8_t*>(buf4);
    const uint32_t j = blockIdx.x;
    if (j >= n_jobs) return;
    const SjParse job = jobs[j];
    const uint8_t* t = base + job.text_off;
    const uint64_t len = job.len;                                     // bytes between '[' and ']'
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t* out = values + job.value_off;
    uint32_t bad = 0;
    uint64_t index = 0;                                               // numbers in front of the chunk
    for (uint64_t c0 = 0; c0 < len; c0 += SJ_CHUNK) {
        // bytes [c0, c0 + SJ_CHUNK + SJ_AHEAD) of the array -> buf[shift ...], from the 16-byte line they begin in
        const uintptr_t addr = reinterpret_cast<uintptr_t>(t + c0);
        const SjChunkGeom g = sj_chunk_geom(addr, c0, len);
        const uint4* src = reinterpret_cast<const uint4*>(addr - g.shift);
        __syncthreads();
        for (uint32_t l = lane; l < g.lines; l += 64u) buf4[l] = src[l];
        __syncthreads();
        const uint8_t* b = buf + g.shift;                             // b[i] = byte c0 + i of the array, i < want
        const uint32_t commas = sj_lane_commas(b, sj_lane_begin(lane), sj_lane_end(lane, g.in_chunk));
        uint32_t incl = commas;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if (lane >= (uint32_t)o) incl += u; }
        const uint32_t chunk_commas = __shfl(incl, 63);
        const SjChunkIndex ix = sj_chunk_index(index, incl, commas, chunk_commas);
        sj_parse_lane(b, g, lane, c0, len, ix.lane_first, job.n_values, out, bad);
        index = ix.next;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __syncthreads();
    uint32_t kept = 0;
    sj_order_lane(out, job.n_values, lane, keep_max, kept, bad);
    for (int o = 32; o; o >>= 1) { kept += __shfl_xor(kept, o); bad |= __shfl_xor(bad, o); }
    if (lane == 0) {
        SjParsed r;
        r.n_kept = kept;
        r.flags = bad ? SJ_SPAN_ODD : 0u;
        results[j] = r;
    }
}

__global__ __launch_bounds__(256) void sj_take_bytes_kernel(const uint8_t* __restrict__ base, const SjPiece* __restrict__ pieces, uint8_t* __restrict__ out) {
    const SjPiece p = pieces[blockIdx.x];
    for (uint64_t i = threadIdx.x; i < p.n; i += 256u) out[p.dst + i] = base[p.src + i];
}

__global__ __launch_bounds__(256) void sj_take_u64_kernel(const uint64_t* __restrict__ values, const SjPiece* __restrict__ pieces, uint64_t* __restrict__ out) {
    const SjPiece p = pieces[blockIdx.x];
    for (uint64_t i = threadIdx.x; i < p.n; i += 256u) out[p.dst + i] = values[p.src + i];
}

}  // namespace

hipError_t sj_spans_launch(const uint8_t* d_base, const SjDoc* d_docs, uint32_t n_docs, SjSpan* d_spans, uint32_t* d_doc_flags, hipStream_t stream) {
    if (n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(sj_spans_kernel, dim3(n_docs), dim3(64), 0, stream, d_base, d_docs, n_docs, d_spans, d_doc_flags);
    return hipGetLastError();
}

hipError_t sj_parse_launch(const uint8_t* d_base, const SjParse* d_jobs, uint32_t n_jobs, uint64_t* d_values, SjParsed* d_results, uint64_t keep_max,
                           hipStream_t stream) {
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(sj_parse_kernel, dim3(n_jobs), dim3(64), 0, stream, d_base, d_jobs, n_jobs, d_values, d_results, keep_max);
    return hipGetLastError();
}

hipError_t sj_take_bytes_launch(const uint8_t* d_base, const SjPiece* d_pieces, uint32_t n, uint8_t* d_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sj_take_bytes_kernel, dim3(n), dim3(256), 0, stream, d_base, d_pieces, d_out);
    return hipGetLastError();
}

hipError_t sj_take_u64_launch(const uint64_t* d_values, const SjPiece* d_pieces, uint32_t n, uint64_t* d_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sj_take_u64_kernel, dim3(n), dim3(256), 0, stream, d_values, d_pieces, d_out);
    return hipGetLastError();
}

}  // namespace smg
