// What the runtime says about the appending sketch kernel's residency: workgroups per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor)
// of sketch_dna_kernel<K, 16, false> at k = 21, 31, 51 and 88, with the static LDS and registers the runtime reports, as one JSON
// object.  Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 [-DSMG_SK_R_MAX=n] -I sourmash_amd/csrc tools/sketch_residency.hip -o tools/sketch_residency
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "sketch_kernel.hpp"

template <int K>
static int report(bool last) {
    const void* f = (const void*)smg::sketch_dna_kernel<K, 16, false>;
    int blocks = 0;
    hipFuncAttributes a;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, f, smg::SK_BLOCK, 0) != hipSuccess) return 1;
    if (hipFuncGetAttributes(&a, f) != hipSuccess) return 1;
    printf("  \"k%d\": {\"rounds_max\": %d, \"sink_entries\": %d, \"workgroups_per_cu\": %d, \"waves_per_simd\": %d, \"lds_bytes\": %zu, \"registers\": %d}%s\n",
           K, smg::sk_rounds_max(K, false), smg::sk_out_cap(smg::sk_rounds_max(K, false), smg::sk_lane_positions(K, false)), blocks, blocks * smg::SK_BLOCK / 64 / 4,
           a.sharedSizeBytes, a.numRegs, last ? "" : ",");
    return 0;
}

int main() {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 2; }
    printf("{\n  \"device\": \"%s\", \"cus\": %d, \"lds_per_cu\": %zu,\n", p.gcnArchName, p.multiProcessorCount, p.maxSharedMemoryPerMultiProcessor);
    int rc = report<21>(false) | report<31>(false) | report<51>(false) | report<88>(true);
    printf("}\n");
    return rc;
}
