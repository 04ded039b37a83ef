// tests/atlas_move_emu/fdh_device.h -- NOT the library's header of that name: a host shim under which figdraw_amd/csrc/k_atlas_move.hip, copied
// beside it with fdh_atlas_move.h, compiles as plain C++ (tests/test_atlas_move_host.py).  The kernel has no cross-lane operation and no
// shared memory: a launch runs the workgroups of the grid one after the other and the 64 lanes of each one after the other.
#pragma once
#include <stdint.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
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
namespace emu { inline long workgroups = 0; }
#define FDH_LAUNCH(kern, grid, block, bytes_, stream, ...)                 \
  do {                                                                     \
    for (int bx_ = 0; bx_ < (grid).x; bx_++) {                             \
      for (int t_ = 0; t_ < (block).x; t_++) {                             \
        blockIdx.x = bx_; blockIdx.y = 0; threadIdx.x = t_; threadIdx.y = 0; \
        kern(__VA_ARGS__);                                                 \
      }                                                                    \
      emu::workgroups++;                                                   \
    }                                                                      \
  } while (0)
