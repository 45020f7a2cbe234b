// smg_hd.hpp -- SMG_HD: what marks a function of a *_core.hpp header, compiled for the device and for the host by hipcc and for
// the host alone by g++ (the emulations of tests/native/).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef SMG_HD
#if defined(__HIPCC__)
#define SMG_HD __host__ __device__ __forceinline__
#else
#define SMG_HD inline
#endif
#endif

// a loop the device compiler must unroll (g++ does not know the pragma)
#ifndef SMG_UNROLL
#if defined(__HIPCC__)
#define SMG_UNROLL _Pragma("unroll")
#else
#define SMG_UNROLL
#endif
#endif
