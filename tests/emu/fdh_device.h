// tests/emu/fdh_device.h -- NOT the library's header of that name: the sequential host shim.  A test copies it beside a kernel's source
// (figdraw_amd/csrc/k_*.hip, unmodified) and a driver (tests/*_emu/emu.cpp), and the three compile as one plain C++17 program
// (tests/emu_build.py).  It checks a kernel's algorithm, its selects, its bounds and where its lanes meet on a CPU; it is no device.
//
// A workgroup's lanes run one after the other, again and again from the kernel's first line.  A lane replays the answers it already
// knows and stops, by exception, at the first collective point nobody has answered yet: a ballot (the wave's) or __syncthreads /
// __syncthreads_or (the workgroup's).  When every lane of the scope has arrived the answer is recorded, and the next pass goes one
// collective point further; a kernel without one costs one pass.  What a lane stores to __shared__ memory before a barrier is there for
// every lane behind it.  A lane that runs again stores again what it stored before: these kernels store out of place.
// A wave's "any" (FDH_IMAGE_SDF_WAVE_ANY) is known to be yes as soon as one lane says so, and that lane goes on within the pass; a lane
// that says no stops and learns the answer in a later pass.  __ballot returns the whole mask, so every lane stops there.
// A ballot that only some lanes of its wave reach, a workgroup's vote or barrier that only some lanes reach, or waves that disagree about
// which vote is the workgroup's next, end the program with exit code 4 and a line on stderr (tests/test_emu_shim_host.py).
// The launch's dynamic shared memory is a heap block of exactly the bytes asked for: AddressSanitizer sees a read or a write past it.
// The hardware's approximate reciprocal, square root, cube root and arc cosine become libm's.
//
// There are two shims, this one and fdh_device_threads.h, because the kernels of the damage codec shuffle values between lanes and read
// what atomics return: a lane run again from the top would add again and hand on another value.  Those run as one thread a lane.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
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
inline Idx threadIdx, blockIdx, blockDim, gridDim;
struct alignas(8) uint2 { uint32_t x, y; };  // the device's alignment: UBSan refuses a wide load or store at any other address
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(16) float4 { float x, y, z, w; };
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline uint32_t max(uint32_t a, uint32_t b) { return a > b ? a : b; }
namespace emu {
constexpr int kMaxWaves = 16;
struct AtCollective {};
enum Scope { kWave, kGroup };
inline std::vector<unsigned long long> answers[kMaxWaves];  // of the collective points of each wave of this workgroup, in order
inline int wave_ballots[kMaxWaves];                         // how many of them are ballots
inline size_t next_point = 0;                               // of the lane that is running
inline int lane = 0;
constexpr size_t kNowhere = ~(size_t)0;
inline struct { size_t at; Scope scope; bool pred; } stops[64 * kMaxWaves];  // where each lane stopped in the pass that is running, and with what
inline unsigned char* lds = nullptr;
// statistics for the caller.  rounds: the ballots a wave took beyond its first, summed; workgroups_with_rounds: workgroups with any
inline long workgroups = 0, lanes = 0, passes = 0, ballots = 0, rounds = 0, workgroups_with_rounds = 0;
[[noreturn]] inline void fail(const char* what) { fprintf(stderr, "%s\n", what); exit(4); }
// (what lies between a kernel and the launcher's catch is inlined at every optimisation level: a throw costs what it has to unwind)
#define EMU_INLINE __attribute__((always_inline)) inline
// -> the answer: a ballot's mask, or 0 / 1.  yes_is_enough: the caller reads "any" alone
EMU_INLINE unsigned long long collective(Scope scope, bool pred, bool yes_is_enough) {
  std::vector<unsigned long long>& a = answers[lane >> 6];
  if (next_point < a.size()) return a[next_point++];
  if (yes_is_enough && pred) { a.push_back(1); next_point++; wave_ballots[lane >> 6]++; ballots++; return 1; }
  stops[lane] = {next_point, scope, pred};
  throw AtCollective();
}
// body(): the kernel's call
template <typename Body>
EMU_INLINE void launch(dim3 grid, dim3 block, size_t bytes, Body body) {
  const int n_lanes = block.x, n_waves = (n_lanes + 63) / 64;
  if (n_waves > kMaxWaves) fail("workgroup too large for the shim");
  blockDim = {block.x, 1}; gridDim = {grid.x, grid.y};
  lds = new unsigned char[bytes];
  for (int by = 0; by < grid.y; by++)
    for (int bx = 0; bx < grid.x; bx++) {
      blockIdx = {bx, by};
      for (int w = 0; w < n_waves; w++) { answers[w].clear(); wave_ballots[w] = 0; }
      for (;;) {  // a pass
        int stopped = 0;
        for (int t = 0; t < n_lanes; t++) {
          threadIdx = {t, 0}; lane = t; next_point = 0;
          stops[t].at = kNowhere;
          try { body(); } catch (AtCollective&) { stopped++; }
        }
        passes++;
        if (!stopped) break;
        int at_group = 0, at_ballot[kMaxWaves] = {}, behind[kMaxWaves] = {};
        unsigned long long group_yes = 0, mask[kMaxWaves] = {};
        for (int t = 0; t < n_lanes; t++) {
          const int w = t >> 6;
          if (stops[t].at == kNowhere) continue;
          if (stops[t].at < answers[w].size()) behind[w]++;  // a later lane's yes answered it: this one learns that in the next pass
          else if (stops[t].scope == kGroup) { at_group++; group_yes |= stops[t].pred; }
          else { at_ballot[w]++; mask[w] |= (unsigned long long)stops[t].pred << (t & 63); }
        }
        if (at_group) {
          if (at_group != n_lanes) fail("a workgroup's vote or barrier reached by some of its lanes only");
          for (int w = 1; w < n_waves; w++) if (answers[w].size() != answers[0].size()) fail("the waves of a workgroup disagree about its next vote");
          for (int w = 0; w < n_waves; w++) answers[w].push_back(group_yes);
          continue;
        }
        for (int w = 0; w < n_waves; w++) {
          if (behind[w] || !at_ballot[w]) continue;
          if (at_ballot[w] != (n_lanes - 64 * w < 64 ? n_lanes - 64 * w : 64)) fail("a ballot reached by some lanes of its wave only");
          answers[w].push_back(mask[w]); wave_ballots[w]++; ballots++;
        }
      }
      bool any_rounds = false;
      for (int w = 0; w < n_waves; w++) if (wave_ballots[w] > 1) { rounds += wave_ballots[w] - 1; any_rounds = true; }
      workgroups++; lanes += n_lanes; workgroups_with_rounds += any_rounds;
    }
  delete[] lds;
}
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
EMU_INLINE unsigned long long __ballot(int pred) { return emu::collective(emu::kWave, pred != 0, false); }
EMU_INLINE int __syncthreads_or(int pred) { return (int)emu::collective(emu::kGroup, pred != 0, false); }
EMU_INLINE void __syncthreads() { __syncthreads_or(0); }
// -DEMU_LANES_ALONE: waves of one lane.  FDH_MSDF_ANY stays undefined and the kernel's own "the lane's own word is the answer" is compiled
#ifndef EMU_LANES_ALONE
#define FDH_MSDF_ANY(p) (__ballot(p) != 0)
#endif
#define FDH_IMAGE_SDF_WAVE_ANY(p) (emu::collective(emu::kWave, (p), true) != 0)
#define FDH_IMAGE_SDF_GROUP_ANY(p) (__syncthreads_or(p) != 0)
#define FDH_IMAGE_SDF_TOGETHER(a, b, c, d, e, f) ((void)0)
#define FDH_IMPORT_HALF_TO_FLOAT(bits) emu::half_to_float(bits)
#define HIP_DYNAMIC_SHARED(type, var) type* var = reinterpret_cast<type*>(emu::lds);
namespace fdh {
inline float frcp(float x) { return 1.0f / x; }
inline float fsqrt(float x) { return sqrtf(x); }
inline float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
inline float cbrt_signed(float x) { return cbrtf(x); }
inline float acos_poly(float x) { return acosf(x); }
}
#define FDH_LAUNCH(kern, grid, block, bytes, stream, ...) emu::launch((grid), (block), (bytes), [&]() __attribute__((always_inline)) { kern(__VA_ARGS__); })
#define hipLaunchKernelGGL FDH_LAUNCH
