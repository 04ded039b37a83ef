// tests/codec_emu/fdh_device.h -- NOT the library's header of that name: a host shim under which figdraw_amd/csrc/k_damage_codec.hip, copied
// beside it, compiles as plain C++20 (tests/test_damage_stream_host.py).  A workgroup is 256 std::threads, __syncthreads a std::barrier,
// the wave shuffles go through a shared array (every thread of the workgroup takes part: the kernel's shuffles are workgroup-uniform),
// the LDS and global atomics are std::atomic_ref.  It checks the kernel's algorithm, barriers and bounds on a CPU; it is no device.
#pragma once
#include <stdint.h>
#include <atomic>
#include <barrier>
#include <algorithm>
#include <cstring>
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
constexpr Idx blockDim{256};
inline std::barrier<>* g_bar;
inline uint32_t g_xchg[256];
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline uint32_t __shfl_xor(uint32_t v, int m, int) { g_xchg[threadIdx.x] = v; __syncthreads(); uint32_t r = g_xchg[threadIdx.x ^ m]; __syncthreads(); return r; }
inline uint32_t __shfl_up(uint32_t v, int d, int) { g_xchg[threadIdx.x] = v; __syncthreads(); int l = threadIdx.x & 63; uint32_t r = l >= d ? g_xchg[threadIdx.x - d] : v; __syncthreads(); return r; }
inline int __popc(uint32_t v) { return __builtin_popcount(v); }
inline int __ffs(uint32_t v) { return __builtin_ffs(v); }
inline uint32_t atomicCAS(uint32_t* p, uint32_t cmp, uint32_t val) { std::atomic_ref<uint32_t> a(*p); a.compare_exchange_strong(cmp, val); return cmp; }
inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { return std::atomic_ref<uint32_t>(*p).fetch_add(v); }
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return std::atomic_ref<unsigned long long>(*p).fetch_add(v); }
using std::min; using std::max;
namespace fdh { constexpr int kBin = 64; }
#define FDH_LAUNCH(kern, grid, block, lds, stream, ...) emu_launch(grid.x, __VA_ARGS__)
