// tests/video_out_emu/fdh_device.h -- NOT the library's header of that name: a host shim under which figdraw_amd/csrc/k_video_export.hip,
// copied beside it, compiles as plain C++ (tests/test_video_out_host.py).  The kernel has no barrier, no shared memory and no atomics: a
// workgroup's lanes run one after the other, once each.
#pragma once
#include <stdint.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define __restrict__
struct dim3 { int x, y; dim3(int a, int b = 1) : x(a), y(b) {} };
typedef void* hipStream_t;
struct Idx { int x, y; };
inline Idx threadIdx, blockIdx;
struct alignas(8) uint2 { uint32_t x, y; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
namespace emu {
inline long workgroups = 0, lanes = 0;
}
#define FDH_LAUNCH(kern, grid, block, bytes_, stream, ...)                              \
  do {                                                                                  \
    for (int by_ = 0; by_ < (grid).y; by_++)                                            \
      for (int bx_ = 0; bx_ < (grid).x; bx_++) {                                        \
        for (int t_ = 0; t_ < (block).x; t_++) {                                        \
          blockIdx.x = bx_; blockIdx.y = by_; threadIdx.x = t_; threadIdx.y = 0;        \
          kern(__VA_ARGS__);                                                            \
          emu::lanes++;                                                                 \
        }                                                                               \
        emu::workgroups++;                                                              \
      }                                                                                 \
  } while (0)
