// tests/image_sdf_emu/fdh_device.h -- NOT the library's header of that name: a host shim under which figdraw_amd/csrc/k_image_sdf.hip, copied
// beside it, compiles as plain C++ (tests/test_image_sdf_host.py).  A workgroup's lanes run one after the other, again and again from the
// kernel's first line, each pass carrying every lane to the first vote whose answer is not known yet:
// - the workgroup's vote (__syncthreads_or; __syncthreads is one that nobody reads) is a barrier: every lane stops there, and the answer
//   is known when all have -- what a lane stores to shared memory before it is there before any lane reads behind it;
// - a wave's vote (the ballot) is known to be "yes" as soon as one lane says so, and that lane goes on; a lane that says "no" stops and
//   learns the answer in a later pass; when all 64 have said "no" the answer is "no".
// A lane that runs again stores again what it stored before.  The launch's dynamic shared memory is a heap block of exactly the bytes
// asked for: AddressSanitizer sees a read or a write past it.  A vote that only some lanes of its wave or workgroup reach, or waves that
// disagree about which vote is the workgroup's next, stop the shim with exit code 4.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
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
namespace emu {
constexpr int kMaxWaves = 16;
struct AtVote {};
inline std::vector<char> answers[kMaxWaves];  // of the votes of each wave of this workgroup, in order
inline size_t next_vote = 0;                  // of the lane that is running
inline int lane = 0;
inline size_t stopped_at = 0;                 // where the running lane stopped
inline int stopped_kind = 0, stopped_pred = 0;
inline long passes = 0, workgroups = 0;       // statistics for the caller
inline unsigned char* lds = nullptr;          // the launch's dynamic shared memory: exactly the bytes it asked for, from the heap
enum { kWave = 0, kGroup = 1 };
inline bool vote(int kind, int pred) {
  std::vector<char>& a = answers[lane >> 6];
  if (next_vote < a.size()) return a[next_vote++] != 0;
  if (kind == kWave && pred) { a.push_back(1); next_vote++; return true; }
  stopped_at = next_vote; stopped_kind = kind; stopped_pred = pred;
  throw AtVote();
}
[[noreturn]] inline void fail(const char* what) { fprintf(stderr, "%s\n", what); exit(4); }
}  // namespace emu
#define FDH_IMAGE_SDF_WAVE_ANY(p) emu::vote(emu::kWave, (p) ? 1 : 0)
#define FDH_IMAGE_SDF_GROUP_ANY(p) emu::vote(emu::kGroup, (p) ? 1 : 0)
inline void __syncthreads() { emu::vote(emu::kGroup, 0); }
#define FDH_IMAGE_SDF_TOGETHER(a, b, c, d, e, f) ((void)0)
#define HIP_DYNAMIC_SHARED(type, var) type* var = reinterpret_cast<type*>(emu::lds);
namespace fdh {
inline float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
}
#define FDH_LAUNCH(kern, grid, block, bytes_, stream, ...)                                                           \
  do {                                                                                                               \
    const int n_lanes_ = (block).x, n_waves_ = ((block).x + 63) / 64;                                                \
    if (n_waves_ > emu::kMaxWaves) emu::fail("workgroup too large for the shim");                                    \
    emu::lds = new unsigned char[(bytes_)];                                                                          \
    for (int by_ = 0; by_ < (grid).y; by_++)                                                                         \
      for (int bx_ = 0; bx_ < (grid).x; bx_++) {                                                                     \
        for (int w_ = 0; w_ < n_waves_; w_++) emu::answers[w_].clear();                                              \
        for (;;) {                                                                                                   \
          int stopped_ = 0, group_stops_ = 0, group_yes_ = 0;                                                        \
          int wave_stops_[emu::kMaxWaves] = {}, wave_behind_[emu::kMaxWaves] = {};                                   \
          int kinds_[1024];                                                                                          \
          size_t at_[1024];                                                                                          \
          for (int t_ = 0; t_ < n_lanes_; t_++) {                                                                    \
            blockIdx.x = bx_; blockIdx.y = by_; threadIdx.x = t_; threadIdx.y = 0;                                   \
            emu::lane = t_; emu::next_vote = 0;                                                                      \
            kinds_[t_] = -1;                                                                                         \
            try { kern(__VA_ARGS__); } catch (emu::AtVote&) {                                                        \
              stopped_++; kinds_[t_] = emu::stopped_kind; at_[t_] = emu::stopped_at;                                 \
              if (emu::stopped_kind == emu::kGroup) { group_stops_++; group_yes_ |= emu::stopped_pred; }             \
            }                                                                                                        \
          }                                                                                                          \
          emu::passes++;                                                                                             \
          if (stopped_ == 0) break;                                                                                  \
          if (group_stops_) {                                                                                        \
            if (group_stops_ != n_lanes_) emu::fail("a workgroup's vote reached by some of its lanes only");         \
            for (int t_ = 0; t_ < n_lanes_; t_++) if (at_[t_] != emu::answers[t_ >> 6].size() || at_[t_] != at_[0]) emu::fail("the waves of a workgroup disagree about its next vote"); \
            for (int w_ = 0; w_ < n_waves_; w_++) emu::answers[w_].push_back((char)group_yes_);                      \
            continue;                                                                                                \
          }                                                                                                          \
          for (int t_ = 0; t_ < n_lanes_; t_++) {                                                                    \
            if (kinds_[t_] < 0) continue;                                                                            \
            if (at_[t_] < emu::answers[t_ >> 6].size()) wave_behind_[t_ >> 6]++; else wave_stops_[t_ >> 6]++;        \
          }                                                                                                          \
          for (int w_ = 0; w_ < n_waves_; w_++) {                                                                    \
            if (wave_behind_[w_] || !wave_stops_[w_]) continue; /* (a lane that learns an answer in the next pass) */ \
            const int in_wave_ = n_lanes_ - 64 * w_ < 64 ? n_lanes_ - 64 * w_ : 64;                                  \
            if (wave_stops_[w_] != in_wave_) emu::fail("a wave's vote reached by some of its lanes only");           \
            emu::answers[w_].push_back(0);                                                                           \
          }                                                                                                          \
        }                                                                                                            \
        emu::workgroups++;                                                                                           \
      }                                                                                                              \
    delete[] emu::lds;                                                                                               \
  } while (0)
