// tests/msdf_cubic_emu/fdh_device.h -- NOT the library's header of that name: a host shim under which figdraw_amd/csrc/k_msdf_cubic.hip and
// k_msdf.hip, copied beside it, compile as plain C++ (tests/test_msdf_cubic_host.py).  The shim of tests/msdf_correct_emu: the one
// cross-lane operation is the ballot, and it becomes a loop over the 64 emulated lanes -- a workgroup is run again and again, lane after
// lane; a lane that reaches a ballot nobody has answered yet leaves its vote and stops there, and when all 64 have voted the answer is known
// and the next pass carries every lane one ballot further.  A ballot that only some lanes reach stops the shim with exit code 4.  The
// hardware's approximate reciprocal, square root, cube root and arc cosine become libm's.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define __restrict__
struct dim3 { int x, y; dim3(int a, int b = 1) : x(a), y(b) {} };
typedef void* hipStream_t;
struct Idx { int x, y; };
inline Idx threadIdx, blockIdx;
namespace emu {
struct AtBallot {};
inline std::vector<unsigned long long> answers;  // the ballots of this workgroup answered so far
inline size_t next_ballot = 0;                   // of the lane that is running
inline unsigned long long votes = 0;
inline int lane = 0;
inline long ballots = 0, rounds = 0, workgroups = 0, workgroups_with_rounds = 0;  // statistics for the caller
}
inline unsigned long long __ballot(int pred) {
  if (emu::next_ballot < emu::answers.size()) return emu::answers[emu::next_ballot++];
  if (pred) emu::votes |= 1ull << emu::lane;
  throw emu::AtBallot();
}
#define FDH_MSDF_ANY(p) (__ballot(p) != 0)
namespace fdh {
inline float frcp(float x) { return 1.0f / x; }
inline float fsqrt(float x) { return sqrtf(x); }
inline float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
inline float cbrt_signed(float x) { return cbrtf(x); }
inline float acos_poly(float x) { return acosf(x); }
}
#define FDH_LAUNCH(kern, grid, block, lds, stream, ...)                                          \
  do {                                                                                           \
    for (int by_ = 0; by_ < (grid).y; by_++)                                                     \
      for (int bx_ = 0; bx_ < (grid).x; bx_++) {                                                 \
        emu::answers.clear();                                                                    \
        for (;;) {                                                                               \
          int stopped_ = 0;                                                                      \
          emu::votes = 0;                                                                        \
          for (int t_ = 0; t_ < (block).x; t_++) {                                               \
            blockIdx.x = bx_; blockIdx.y = by_; threadIdx.x = t_; threadIdx.y = 0;               \
            emu::lane = t_; emu::next_ballot = 0;                                                \
            try { kern(__VA_ARGS__); } catch (emu::AtBallot&) { stopped_++; }                    \
          }                                                                                      \
          if (stopped_ == 0) break;                                                              \
          if (stopped_ != (block).x) { fprintf(stderr, "a ballot reached by %d of %d lanes\n", stopped_, (block).x); exit(4); } \
          emu::answers.push_back(emu::votes);                                                    \
          emu::ballots++;                                                                        \
        }                                                                                        \
        emu::workgroups++;                                                                       \
        if (emu::answers.size() > 1) { emu::workgroups_with_rounds++; emu::rounds += (long)emu::answers.size() - 1; } \
      }                                                                                          \
  } while (0)
