// tests/msdf_emu/fdh_device.h -- NOT the library's header of that name: a host shim under which figdraw_amd/csrc/k_msdf.hip, copied beside
// it, compiles as plain C++ (tests/test_msdf_host.py).  The kernel has no barrier, no LDS and no cross-lane operation, so a launch is a
// loop over workgroups and lanes.  The hardware's approximate reciprocal, square root, cube root and arc cosine become libm's: the shim
// checks the kernel's algorithm, its selects and its bounds on a CPU; the GPU tests hold the compiled kernel to the same reference.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstddef>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define __restrict__
struct dim3 { int x, y; dim3(int a, int b = 1) : x(a), y(b) {} };
typedef void* hipStream_t;
struct Idx { int x, y; };
inline Idx threadIdx, blockIdx;
namespace fdh {
inline float frcp(float x) { return 1.0f / x; }
inline float fsqrt(float x) { return sqrtf(x); }
inline float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
inline float cbrt_signed(float x) { return cbrtf(x); }
inline float acos_poly(float x) { return acosf(x); }
}
#define FDH_LAUNCH(kern, grid, block, lds, stream, ...)                     \
  do {                                                                      \
    for (int by_ = 0; by_ < (grid).y; by_++)                                \
      for (int bx_ = 0; bx_ < (grid).x; bx_++)                              \
        for (int t_ = 0; t_ < (block).x; t_++) {                            \
          blockIdx.x = bx_; blockIdx.y = by_; threadIdx.x = t_; threadIdx.y = 0; \
          kern(__VA_ARGS__);                                                \
        }                                                                   \
  } while (0)
