// Micro-benchmark: what an LDS read costs on gfx950 when its address is off the read's natural alignment.
// ds_read_b128 / ds_read_b64 / ds_read_b32 per wave-instruction at a lane stride of 16 bytes (the sketch kernel's: a lane owns 16
// start positions), byte offsets 0 .. 15, from one region or from two mirrored regions with half the lanes each (forward and
// reverse-complement copy of a tile), at 4, 6 and 8 waves per SIMD.  The figure is LDS-pipe cycles per wave-instruction per CU:
// elapsed cycles / (reads per wave x waves per CU), with every wave of the CU reading all the time.
// Build: hipcc --offload-arch=gfx950 -O3 tools/ubench_lds_unaligned.hip -o tools/ubench_lds_unaligned ; run on the GPU box.
// Results: profiles/strand_lds_ubench.txt, DESIGN.md section 7.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#pragma clang diagnostic ignored "-Wunused-value"
#pragma clang diagnostic ignored "-Wunused-result"

#define ITERS 2048
constexpr int REGION = 272 * 16;   // 256 lanes x 16 bytes + 8 chunks of immediate offsets + the read itself + the byte offset

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// 8 reads in flight, then one wait; the immediates keep the byte phase of the address
#define READ8(OP)                                                                                               \
    asm volatile(OP " %0, %8\n" OP " %1, %8 offset:16\n" OP " %2, %8 offset:32\n" OP " %3, %8 offset:48\n"      \
                 OP " %4, %8 offset:64\n" OP " %5, %8 offset:80\n" OP " %6, %8 offset:96\n" OP " %7, %8 offset:112\n" \
                 "s_waitcnt lgkmcnt(0)\n"                                                                       \
                 : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7)    \
                 : "v"(addr) : "memory")

template <int BYTES, bool TWO>
__global__ __launch_bounds__(256) void k_read(uint32_t* out, uint32_t off) {
    __shared__ __attribute__((aligned(16))) uint32_t s[(TWO ? 2 : 1) * REGION / 4];
    const int tid = threadIdx.x;
    for (int i = tid; i < (TWO ? 2 : 1) * REGION / 4; i += 256) s[i] = i * 2654435761u;
    __syncthreads();
    // one region: byte tid * 16 + off.  Two: the upper half of each wave reads the second region downwards, (255 - tid) * 16 + 16 - off.
    const uint32_t lds = (uint32_t)(size_t)((__attribute__((address_space(3))) uint32_t*)s);
    uint32_t addr = lds + tid * 16 + off;
    if (TWO && (tid & 32)) addr = lds + REGION + (255 - tid) * 16 + 16 - off;
    uint32_t acc = 0;
    for (int i = 0; i < ITERS; ++i) {
        if constexpr (BYTES == 16) {
            u32x4 r0, r1, r2, r3, r4, r5, r6, r7;
            READ8("ds_read_b128");
            acc ^= r0.x ^ r1.y ^ r2.z ^ r3.w ^ r4.x ^ r5.y ^ r6.z ^ r7.w;
        } else if constexpr (BYTES == 8) {
            u32x2 r0, r1, r2, r3, r4, r5, r6, r7;
            READ8("ds_read_b64");
            acc ^= r0.x ^ r1.y ^ r2.x ^ r3.y ^ r4.x ^ r5.y ^ r6.x ^ r7.y;
        } else {
            uint32_t r0, r1, r2, r3, r4, r5, r6, r7;
            READ8("ds_read_b32");
            acc ^= r0 ^ r1 ^ r2 ^ r3 ^ r4 ^ r5 ^ r6 ^ r7;
        }
    }
    out[blockIdx.x * 256 + tid] = acc;
}

typedef void (*kern_t)(uint32_t*, uint32_t);

static bool run(const char* name, kern_t k, int waves_per_simd, uint32_t* d) {
    const int blocks = 256 * waves_per_simd;           // 256 threads = 4 waves = 1 wave per SIMD; 256 CUs
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    printf("%-26s waves/SIMD=%d  cycles per wave-instruction per CU at byte offset 0..15 (2.4 GHz nominal):", name, waves_per_simd);
    for (uint32_t off = 0; off < 16; ++off) {
        hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, d, off);
        hipEventRecord(e0);
        hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, d, off);
        hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) { printf(" HIP error: %s\n", hipGetErrorString(hipGetLastError())); return false; }
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        const double reads_per_cu = (double)ITERS * 8 * 4 * waves_per_simd;
        printf(" %6.2f", ms * 1e-3 * 2.4e9 / reads_per_cu);
    }
    printf("\n");
    fflush(stdout);
    hipEventDestroy(e0); hipEventDestroy(e1);
    return true;
}

int main() {
    uint32_t* d;
    if (hipMalloc(&d, (size_t)256 * 8 * 256 * 4) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    const int waves[] = {4, 6, 8};
#define R(NAME, B, T) for (int w : waves) if (!run(NAME, k_read<B, T>, w, d)) return 1;
    R("ds_read_b128 one region", 16, false) R("ds_read_b128 two mirrored", 16, true)
    R("ds_read_b64  one region", 8, false) R("ds_read_b64  two mirrored", 8, true)
    R("ds_read_b32  one region", 4, false) R("ds_read_b32  two mirrored", 4, true)
    hipFree(d);
    return 0;
}
