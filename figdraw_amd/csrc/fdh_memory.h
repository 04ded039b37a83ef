// fdh_memory.h -- the host side's memory vocabulary: the HIP error check, growable device / pinned blocks, the process-wide store of staging
// blocks in device memory (fdh_vram.cpp), and HostVec, the array a lane records into.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "fdh_plain.h"

namespace fdh {

void hip_check(hipError_t e, const char* what);
#define FDH_HIP(x) ::fdh::hip_check((x), #x)

// A caller's pointer as the device addresses it: device memory of `device` as it is, page-locked host memory as its device view; null for
// anything else (pageable memory, another device's, an address nobody has mapped), the runtime's sticky error cleared behind the question.
// What fdh_put_image_device, fdh_put_video_frame and fdh_read_video_frame ask of a plane.
inline void* device_view_of(int device, const void* data) {
  hipPointerAttribute_t attr{};
  const hipError_t err = hipPointerGetAttributes(&attr, data);
  (void)hipGetLastError();
  if (err == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == device) return const_cast<void*>(data);
  if (err == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer) return attr.devicePointer;
  return nullptr;
}

// Fault-hunting builds (-DFDH_POISON=<byte>): every fresh device allocation is filled with that byte before its first use -- a kernel that
// reads memory nothing has written yet then reads the same garbage every time, not what the allocation's previous owner left.
void poison_fresh(void* p, size_t bytes);  // fdh_context.cpp
template <typename T>
struct DeviceBuf {
  T* ptr = nullptr;
  size_t cap = 0;
  void reserve(size_t n) {
    if (n <= cap) return;
    size_t want = cap ? cap : 256;
    while (want < n) want *= 2;
    T* fresh = nullptr;  // allocate first: a failing hipMalloc (FDH_HIP throws) must leave ptr / cap describing a live block
    FDH_HIP(hipMalloc((void**)&fresh, want * sizeof(T)));
    poison_fresh(fresh, want * sizeof(T));
    if (ptr) (void)hipFree(ptr);
    ptr = fresh;
    cap = want;
  }
  void reserve_exact(size_t n) {  // no doubling: a block of tens of megabytes is the size that was asked for
    if (n <= cap) return;
    T* fresh = nullptr;
    FDH_HIP(hipMalloc((void**)&fresh, n * sizeof(T)));
    poison_fresh(fresh, n * sizeof(T));
    if (ptr) (void)hipFree(ptr);
    ptr = fresh;
    cap = n;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
};

template <typename T>
struct PinnedBuf {
  T *ptr = nullptr, *dev = nullptr;  // the block as the host addresses it, and as the device does (taken once, when the block is allocated)
  size_t cap = 0;
  void reserve(size_t n) {
    if (n <= cap) return;
    size_t want = cap ? cap : 256;
    while (want < n) want *= 2;
    reserve_exact(want);
  }
  void reserve_exact(size_t n) {  // no doubling: a block of tens of megabytes is the size that was asked for
    if (n <= cap) return;
    T *fresh = nullptr, *fresh_dev = nullptr;
    FDH_HIP(hipHostMalloc((void**)&fresh, n * sizeof(T), hipHostMallocDefault));
    if (hipError_t e = hipHostGetDevicePointer((void**)&fresh_dev, fresh, 0)) { (void)hipHostFree(fresh); FDH_HIP(e); }
    if (ptr) (void)hipHostFree(ptr);
    ptr = fresh; dev = fresh_dev; cap = n;
  }
  void release() {
    if (ptr) (void)hipHostFree(ptr);
    ptr = dev = nullptr;
    cap = 0;
  }
};

// A growable array of plain data, in ordinary memory or -- `pinned` -- in host memory the GPU fetches over PCIe (hipHostMalloc).
// Pinned memory is written once, front to back, and never read by the CPU: on this platform the CPU's loads from it are not
// served from its caches (a record read back from a pinned lane cost ~100 ns; round 4 measured 82 us for a 700-record frame that
// took 4 us from ordinary memory).  Growth copies what the array holds (doubling: rare once a context has seen its scene).
//
// `vram` (with `pinned`): the same role in DEVICE memory the host writes through the PCIe BAR.  On the MI355X boxes all of HBM is
// host-addressable (large BAR): the CPU's stores into a hipExtMallocWithFlags(hipDeviceMallocUncached) block are write-combined
// posted writes (measured: 128 KB in 3.2 us = 41 GB/s, tools/microbench/bar_write.hip) and the GPU reads what they wrote from its
// own memory instead of fetching it over the link with a round trip per lane: k_upload_frame 7.1 -> ~3 us.  Write-only for the
// CPU -- a load from it crosses the link uncached -- so growth does NOT carry contents over (callers set n = 0 first, as the pinned
// mirrors always did), and a store fence (store_fence()) precedes the hand-over to whoever launches the kernels.
bool vram_staging(int device);  // large-BAR device and FDH_VRAM_STAGING != 0, decided per device ordinal (fdh_vram.cpp)
// Device blocks for staging come from, and go back to, a process-wide store by size class (powers of two from 4 KB): they are
// never handed back to the driver while the process lives.  A block the driver recycles may be memory another allocation's
// kernels wrote through the L2s; the host's stores reach memory BESIDE those caches, and a line written back later lands on top
// of them (tools/thread_churn.py: fresh contexts on four host threads, wrong first frames or a fault in ~5 % of runs).  Staging
// blocks are only ever written by the host and read uncached by the device, so recycled among themselves they carry no such lines.
// The store is keyed by DEVICE ORDINAL: a block allocated on GPU 0 never reaches a context on GPU 1.
void* vram_block_acquire(int device, size_t bytes, size_t* size_class);  // throws Error on failure
void vram_block_release(int device, void* p, size_t size_class);
size_t vram_store_bytes(int device);   // bytes the store of a device holds (released blocks)
int vram_contexts_alive(int device);   // device contexts alive on `device` (the deep strips' threshold goes by it: Context::schedule)
// another context has launched a frame on `device` within the last few milliseconds (block waves go by it: Context::schedule); stamps `who`
bool device_shared_now(int device, const void* who);
void vram_context_born(int device);    // a device context exists on `device` ...
void vram_context_gone(int device);    // ... and is gone: with the last one, the device's store is trimmed to kVramStoreKeep
constexpr size_t kVramStoreKeep = (size_t)16 << 20;
inline void store_fence() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_sfence();
#else
  __sync_synchronize();
#endif
}
template <typename T>
struct HostVec {
  T* p = nullptr;
  size_t n = 0, cap = 0;
  bool pinned = false, vram = false;
  int dev = 0;  // device ordinal of a vram block
  HostVec() = default;
  HostVec(const HostVec&) = delete;
  HostVec& operator=(const HostVec&) = delete;
  ~HostVec() { release(); }
  void free_block(T* q) { if (!q) return; if (pinned && vram) vram_block_release(dev, q, vram_bytes_); else if (pinned) (void)hipHostFree(q); else std::free(q); }
  size_t vram_bytes_ = 0;  // size class of the device block p (vram_block_acquire)
  void release() {
    free_block(p);
    p = nullptr; n = cap = 0;
  }
  void reserve(size_t want) {
    if (want <= cap) return;
    size_t c = cap ? cap : 256;
    while (c < want) c *= 2;
    T* fresh = nullptr;
    size_t fresh_bytes = 0;
    if (pinned && vram) fresh = static_cast<T*>(vram_block_acquire(dev, c * sizeof(T), &fresh_bytes));
    else if (pinned) FDH_HIP(hipHostMalloc((void**)&fresh, c * sizeof(T), hipHostMallocDefault));
    else if (!(fresh = static_cast<T*>(std::aligned_alloc(64, (c * sizeof(T) + 63) & ~(size_t)63)))) throw std::bad_alloc();
    if (n && !(pinned && vram)) std::memcpy(static_cast<void*>(fresh), static_cast<const void*>(p), n * sizeof(T));
    free_block(p);
    p = fresh; cap = c; vram_bytes_ = fresh_bytes;
  }
  // the block as the GPU addresses it
  const uint8_t* device_view() const {
    if (!p) return nullptr;
    if (pinned && vram) return reinterpret_cast<const uint8_t*>(p);
    void* d = nullptr;
    FDH_HIP(hipHostGetDevicePointer(&d, const_cast<void*>(static_cast<const void*>(p)), 0));
    return static_cast<const uint8_t*>(d);
  }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
  T* slot() { if (n == cap) reserve(n + 1); return p + n; }  // the next element's place (not yet counted)
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  T& back() { return p[n - 1]; }
  void clear() { n = 0; }
  void append(const T* src, size_t k) { if (!k) return; reserve(n + k); std::memcpy(static_cast<void*>(p + n), static_cast<const void*>(src), k * sizeof(T)); n += k; }
};

}  // namespace fdh
