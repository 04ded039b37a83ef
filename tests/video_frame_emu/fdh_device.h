// tests/video_frame_emu/fdh_device.h -- NOT the library's header of that name: a host shim under which figdraw_amd/csrc/k_video_import.hip (and k_image_import.hip, whose tail kernel finishes the chain),
// copied beside it, compiles as plain C++ (tests/test_video_frame_host.py).  A workgroup's lanes run one after the other, again and again
// from the kernel's first line; pass p carries every lane to barrier p (or to the kernel's end).  What a lane stores to shared memory in
// front of a barrier is there before any lane reads behind it.  A lane that runs again stores again what it stored before: the kernels
// write no word of shared memory twice and use no atomics, so that is harmless.  A barrier that only some lanes of the workgroup reach
// stops the shim with exit code 4.
#pragma once
#include <stdint.h>
#include <cmath>
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
#define __shared__ static
struct dim3 { int x, y; dim3(int a, int b = 1) : x(a), y(b) {} };
typedef void* hipStream_t;
struct Idx { int x, y; };
inline Idx threadIdx, blockIdx;
struct uint2 { uint32_t x, y; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(16) float4 { float x, y, z, w; };
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline uint32_t max(uint32_t a, uint32_t b) { return a > b ? a : b; }
namespace emu {
struct AtBarrier {};
inline int pass = 0;       // the barrier this pass carries the lanes to
inline int barriers = 0;   // the running lane has passed so many
inline long passes = 0, workgroups = 0;
[[noreturn]] inline void fail(const char* what) { fprintf(stderr, "%s\n", what); exit(4); }
// an IEEE half widened to float, bit by bit (the device has an instruction for it)
inline float half_to_float(uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
  uint32_t bits;
  if (e == 31u) bits = sign | 0x7F800000u | (m << 13);
  else if (e) bits = sign | ((e + 112u) << 23) | (m << 13);
  else if (!m) bits = sign;
  else {  // a denormal half is a normal float
    int shift = 0;
    uint32_t mm = m;
    while (!(mm & 0x400u)) { mm <<= 1; shift++; }
    bits = sign | ((uint32_t)(113 - shift) << 23) | ((mm & 0x3FFu) << 13);
  }
  float f;
  memcpy(&f, &bits, 4);
  return f;
}
}  // namespace emu
inline void __syncthreads() {
  if (emu::barriers == emu::pass) throw emu::AtBarrier();
  emu::barriers++;
}
#define FDH_IMPORT_HALF_TO_FLOAT(bits) emu::half_to_float(bits)
#define FDH_LAUNCH(kern, grid, block, bytes_, stream, ...)                                                  \
  do {                                                                                                      \
    const int n_lanes_ = (block).x;                                                                         \
    for (int by_ = 0; by_ < (grid).y; by_++)                                                                \
      for (int bx_ = 0; bx_ < (grid).x; bx_++) {                                                            \
        for (emu::pass = 0;; emu::pass++) {                                                                 \
          int stopped_ = 0;                                                                                 \
          for (int t_ = 0; t_ < n_lanes_; t_++) {                                                           \
            blockIdx.x = bx_; blockIdx.y = by_; threadIdx.x = t_; threadIdx.y = 0;                          \
            emu::barriers = 0;                                                                              \
            try { kern(__VA_ARGS__); } catch (emu::AtBarrier&) { stopped_++; }                              \
          }                                                                                                 \
          emu::passes++;                                                                                    \
          if (stopped_ == 0) break;                                                                         \
          if (stopped_ != n_lanes_) emu::fail("a barrier reached by some lanes of the workgroup only");     \
        }                                                                                                   \
        emu::workgroups++;                                                                                  \
      }                                                                                                     \
  } while (0)
