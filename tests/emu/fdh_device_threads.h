// tests/emu/fdh_device_threads.h -- NOT the library's fdh_device.h: the threaded host shim, which a test copies under that name beside
// a kernel of the damage codec (figdraw_amd/csrc/k_damage_codec.hip, k_damage_filter.hip, k_damage_move.hip, unmodified), the stand-in
// fdh_damage.h and a driver; they compile as one plain C++20 program (tests/emu_build.py).  A workgroup is 256 std::threads, __syncthreads
// a std::barrier of 256; a wave is 64 of them with a barrier of its own, through which the wave's shuffles and ballots go (the kernels
// call those in wave-uniform, not always workgroup-uniform, control flow).  LDS and global atomics are std::atomic_ref.  It checks the
// kernels' algorithms, barriers and bounds on a CPU; it is no device.
// It stays apart from the sequential shim (fdh_device.h, lanes run again from the top until every collective point is answered) because
// these kernels shuffle values between lanes and read what atomics return: a lane run again would add again and hand on another value.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <barrier>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define __restrict__
#define __shared__ static
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
struct int4 { int x, y, z, w; };
inline uint2 make_uint2(uint32_t a, uint32_t b) { return {a, b}; }
inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return {a, b, c, d}; }
struct dim3 { int x; dim3(int v) : x(v) {} };
typedef void* hipStream_t;
struct Idx { int x; };
inline thread_local Idx threadIdx, blockIdx;
inline Idx gridDim{1};
constexpr Idx blockDim{256};
inline std::barrier<>* g_bar;
inline std::barrier<>* g_wave_bar[4];
inline uint32_t g_xchg[256];
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline void emu_wave_sync() { g_wave_bar[threadIdx.x >> 6]->arrive_and_wait(); }
inline uint32_t __shfl_xor(uint32_t v, int m, int) { g_xchg[threadIdx.x] = v; emu_wave_sync(); uint32_t r = g_xchg[threadIdx.x ^ m]; emu_wave_sync(); return r; }
inline uint32_t __shfl_up(uint32_t v, int d, int) { g_xchg[threadIdx.x] = v; emu_wave_sync(); int l = threadIdx.x & 63; uint32_t r = l >= d ? g_xchg[threadIdx.x - d] : v; emu_wave_sync(); return r; }
inline unsigned long long __ballot(bool p) {
  g_xchg[threadIdx.x] = p ? 1u : 0u;
  emu_wave_sync();
  unsigned long long m = 0;
  for (int l = 0; l < 64; l++) m |= (unsigned long long)g_xchg[(threadIdx.x & ~63) + l] << l;
  emu_wave_sync();
  return m;
}
inline int __popc(uint32_t v) { return __builtin_popcount(v); }
inline int __ffs(uint32_t v) { return __builtin_ffs(v); }
inline uint32_t atomicCAS(uint32_t* p, uint32_t cmp, uint32_t val) { std::atomic_ref<uint32_t> a(*p); a.compare_exchange_strong(cmp, val); return cmp; }
inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { return std::atomic_ref<uint32_t>(*p).fetch_add(v); }
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return std::atomic_ref<unsigned long long>(*p).fetch_add(v); }
using std::min; using std::max;
namespace fdh { constexpr int kBin = 64; }
// one workgroup at a time (a kernel's __shared__ objects are statics), 256 threads; a thread that returns leaves both of its barriers,
// and so does one that a driver's stand-in takes out of the kernel with `throw 0`
template <typename Kernel, typename Params>
inline void emu_launch(Kernel kern, int grid, const Params& P) {
  gridDim.x = grid;
  for (int b = 0; b < grid; b++) {
    std::barrier<> bar(256);
    std::unique_ptr<std::barrier<>> wave[4];
    for (int w = 0; w < 4; w++) { wave[w] = std::make_unique<std::barrier<>>(64); g_wave_bar[w] = wave[w].get(); }
    g_bar = &bar;
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++)
      th.emplace_back([&, t, b] { threadIdx.x = t; blockIdx.x = b; try { kern(P); } catch (int) {} g_wave_bar[t >> 6]->arrive_and_drop(); bar.arrive_and_drop(); });
    for (auto& x : th) x.join();
  }
}
#define FDH_LAUNCH(kern, grid, block, lds, stream, ...) emu_launch(kern, (grid).x, __VA_ARGS__)
