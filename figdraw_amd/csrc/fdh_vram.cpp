// fdh_vram.cpp -- the per-device store of staging blocks in device memory (HostVec::vram), and who is alive on a device.
#include "fdh_context.h"

#include <chrono>
#include <cstdlib>
#include <mutex>
#include <vector>

namespace fdh {

// Staging in device memory (HostVec::vram): when the device exposes all of its memory to the host (large BAR: every MI355X box of
// the pool) the recording threads write the frame's records straight into HBM and the gather kernel reads them locally.
// FDH_VRAM_STAGING=0 keeps pinned host memory (the path for devices without a large BAR), =1 forces device memory.
// Decided PER DEVICE (fdh_create takes an ordinal: one process may hold contexts on several GPUs), once, on first use.
namespace {
constexpr int kMaxDevices = 64;
std::mutex g_vram_mu;
int g_vram_probe[kMaxDevices];  // 0 not probed yet, 1 staging in device memory, -1 pinned host memory
// the store of released blocks: by device, then by log2 of the size class
std::vector<void*> g_vram_free[kMaxDevices][48];
int g_vram_contexts[kMaxDevices];  // device contexts alive per device (the store of a device is trimmed when its last one goes)
int vram_class(size_t bytes) { int k = 12; while (((size_t)1 << k) < bytes) k++; return k; }
// the calling thread's current device for the scope (pool threads and callers with contexts on several devices allocate here)
struct DeviceScope {
  int prev = -1, dev;
  explicit DeviceScope(int d) : dev(d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); }
  ~DeviceScope() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};
bool vram_probe(int dev) {
  if (const char* e = std::getenv("FDH_VRAM_STAGING")) return std::atoi(e) != 0;
  DeviceScope scope(dev);
  int large = 0;
  if (hipDeviceGetAttribute(&large, hipDeviceAttributeIsLargeBar, dev) != hipSuccess || !large) return false;
  // ... and a round trip to make sure: the CPU stores a pattern into such a block, a device-to-host copy must bring it back
  uint32_t* d = nullptr;
  if (hipExtMallocWithFlags((void**)&d, 4096, hipDeviceMallocUncached) != hipSuccess || !d) return false;
  bool ok = true;
  for (uint32_t i = 0; i < 1024; i++) d[i] = 0x9e3779b9u * (i + 1);
  store_fence();
  uint32_t back[1024];
  if (hipMemcpy(back, d, sizeof back, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
  for (uint32_t i = 0; ok && i < 1024; i++) ok = back[i] == 0x9e3779b9u * (i + 1);
  (void)hipFree(d);
  return ok;
}
}  // namespace
bool vram_staging(int device) {
  if (device < 0 || device >= kMaxDevices) return false;
  std::lock_guard<std::mutex> lk(g_vram_mu);
  if (g_vram_probe[device] == 0) g_vram_probe[device] = vram_probe(device) ? 1 : -1;
  return g_vram_probe[device] > 0;
}
void* vram_block_acquire(int device, size_t bytes, size_t* size_class) {
  const int k = vram_class(bytes);
  *size_class = (size_t)1 << k;
  if (device < 0 || device >= kMaxDevices) throw Error(FDH_ERR_NO_DEVICE, "staging block asked for a device ordinal out of range");
  {
    std::lock_guard<std::mutex> lk(g_vram_mu);
    auto& fl = g_vram_free[device][k];
    if (!fl.empty()) { void* p = fl.back(); fl.pop_back(); return p; }
  }
  DeviceScope scope(device);  // (a walk-pool thread's current device is whatever it was created with)
  void* p = nullptr;
  FDH_HIP(hipExtMallocWithFlags(&p, (size_t)1 << k, hipDeviceMallocUncached));
  return p;
}
void vram_block_release(int device, void* p, size_t size_class) {
  if (!p) return;
  // (fault hunting: FDH_VRAM_STORE=0 gives blocks back to the driver, as until the end of round 4; =2 neither frees nor reuses them)
  static const int mode = [] { const char* e = std::getenv("FDH_VRAM_STORE"); return e ? std::atoi(e) : 1; }();
  if (mode == 2) return;
  if (mode == 0 || !size_class || device < 0 || device >= kMaxDevices) { (void)hipFree(p); return; }
  std::lock_guard<std::mutex> lk(g_vram_mu);
  g_vram_free[device][vram_class(size_class)].push_back(p);
}
size_t vram_store_bytes(int device) {
  if (device < 0 || device >= kMaxDevices) return 0;
  std::lock_guard<std::mutex> lk(g_vram_mu);
  size_t b = 0;
  for (int k = 0; k < 48; k++) b += g_vram_free[device][k].size() << k;
  return b;
}
int vram_contexts_alive(int device) {
  if (device < 0 || device >= kMaxDevices) return 0;
  std::lock_guard<std::mutex> lk(g_vram_mu);
  return g_vram_contexts[device];
}
// Who launched frames on `device` last: two slots {context, time}.  A context that launches asks whether ANOTHER one has launched within
// the last few milliseconds -- frames of several contexts in flight, as opposed to contexts that merely exist -- and leaves its own stamp.
bool device_shared_now(int device, const void* who) {
  using clock = std::chrono::steady_clock;
  struct Slot { const void* who = nullptr; clock::time_point at{}; };
  static std::mutex mu;
  static Slot slots[kMaxDevices][2];
  if (device < 0 || device >= kMaxDevices) return false;
  constexpr auto kWindow = std::chrono::milliseconds(5);
  const auto now = clock::now();
  std::lock_guard<std::mutex> lk(mu);
  Slot* s = slots[device];
  bool shared = false;
  for (int i = 0; i < 2; i++) shared = shared || (s[i].who != nullptr && s[i].who != who && now - s[i].at < kWindow);
  Slot& mine = s[0].who == who ? s[0] : s[1].who == who ? s[1] : (s[0].at <= s[1].at ? s[0] : s[1]);
  mine.who = who; mine.at = now;
  return shared;
}
void vram_context_born(int device) {
  if (device < 0 || device >= kMaxDevices) return;
  std::lock_guard<std::mutex> lk(g_vram_mu);
  g_vram_contexts[device]++;
}
// The last device context of a device is gone: its store keeps at most kVramStoreKeep bytes (largest blocks go first -- one huge
// frame must not pin its HBM for the life of the process).  Called with the device idle (the context has synchronised its stream).
// The blocks are unmapped UNDER g_vram_mu, and a context counts itself in (vram_context_born) before it creates its stream: freeing
// uncached BAR-visible blocks while another context renders is the trigger of round 4's stale-line faults, so
// while a trim runs no context of the device exists and none can come to exist -- a constructor on another thread waits at the lock.
void vram_context_gone(int device) {
  if (device < 0 || device >= kMaxDevices) return;
  std::lock_guard<std::mutex> lk(g_vram_mu);
  if (--g_vram_contexts[device] > 0) return;
  std::vector<void*> drop;
  size_t held = 0;
  for (int k = 0; k < 48; k++) held += g_vram_free[device][k].size() << k;
  for (int k = 47; k >= 12 && held > kVramStoreKeep; k--)
    while (!g_vram_free[device][k].empty() && held > kVramStoreKeep) { drop.push_back(g_vram_free[device][k].back()); g_vram_free[device][k].pop_back(); held -= (size_t)1 << k; }
  if (drop.empty()) return;
  DeviceScope scope(device);
  (void)hipDeviceSynchronize();
  for (void* p : drop) (void)hipFree(p);
}

}  // namespace fdh
