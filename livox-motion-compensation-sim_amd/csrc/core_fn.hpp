// core_fn.hpp — the function qualifiers of the scalar cores (DESIGN.md "Core headers"): the headers whose
// text compiles for the device and, unchanged, for the host tests.  Under hipcc each macro is exactly the
// qualifier sequence its functions carried before they shared this header; off the device it is `inline`
// or nothing.  No HIP include.
#pragma once

#if defined(__HIPCC__)
#define MC_CORE_HD __host__ __device__ __forceinline__                            // host + device cores
#define MC_CORE_HD_INLINE __host__ __device__ inline                              // the ray-march core: not forced
#define MC_CORE_HD_NOINLINE __host__ __device__ __attribute__((noinline)) inline  // its out-of-line predicate
#define MC_CORE_DEV __device__ __forceinline__                                    // device-only cores
#define MC_CORE_DEV_NOINLINE __device__ __noinline__                              // their rarely taken paths
#define MC_CORE_DEV_DECL __device__ __forceinline__   // a function the including unit defines, declared for a core
#else
#define MC_CORE_HD inline
#define MC_CORE_HD_INLINE inline
#define MC_CORE_HD_NOINLINE inline
#define MC_CORE_DEV inline
#define MC_CORE_DEV_NOINLINE
#define MC_CORE_DEV_DECL
#endif

// the two pragmas a core's text needs, spelled so that a compiler that does not know them sees nothing
#if defined(__clang__)
#define MC_CORE_NO_CONTRACT _Pragma("clang fp contract(off)")
#define MC_CORE_UNROLL _Pragma("unroll")
#else
#define MC_CORE_NO_CONTRACT
#define MC_CORE_UNROLL
#endif
