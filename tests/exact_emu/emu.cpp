// tests/exact_emu/emu.cpp -- figdraw_amd/csrc/k_damage_filter.hip under the threaded host shim (tests/emu/fdh_device_threads.h as
// fdh_device.h, and tests/emu/fdh_damage.h, copied beside this file; the kernel and fdh_damage_read.h come from csrc, unmodified:
// tests/test_damage_exact_host.py).
// usage: emu W H frame.raw mirror.raw all(0|1) stamps.raw|- fill(0|1)   (stamp 7 = pending; mirror.raw: [bin][64][64] uint32)
// -> writes mirror_out.raw and stamps_out.raw, prints the count word; fails when a byte past the mirror or the stamps was written
#include "k_damage_filter.hip"
#include <cstdio>
#include <cstdlib>
static bool load(const char* path, void* to, size_t bytes) {
  FILE* f = fopen(path, "rb");
  const bool ok = f && fread(to, 1, bytes, f) == bytes;
  if (f) fclose(f);
  return ok;
}
int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int W = atoi(argv[1]), H = atoi(argv[2]), all = atoi(argv[5]), fill = atoi(argv[7]);
  const int gx = (W + 63) / 64, gy = (H + 63) / 64, nb = gx * gy, pad = 16;
  std::vector<uint32_t> surf((size_t)W * H);
  // (a uint4 store needs 16-byte alignment: the mirror starts on one)
  std::vector<uint4> mirror_store((size_t)nb * 1024 + pad / 4);
  uint32_t* mirror = reinterpret_cast<uint32_t*>(mirror_store.data());
  std::vector<uint32_t> stamp((size_t)nb + pad, 0);
  if (!load(argv[3], surf.data(), surf.size() * 4) || !load(argv[4], mirror, (size_t)nb * 16384)) return 2;
  if (!all && !load(argv[6], stamp.data(), (size_t)nb * 4)) return 2;
  for (int i = 0; i < pad; i++) mirror[(size_t)nb * 4096 + i] = stamp[(size_t)nb + i] = 0xEEEEEEEEu;
  uint32_t n_pending = nb;
  if (!all) { n_pending = 0; for (int b = 0; b < nb; b++) n_pending += stamp[b] == 7; }
  uint32_t count[2 + pad];
  for (uint32_t& c : count) c = 0xEEEEEEEEu;
  unsigned long long arrivals = 0;
  fdh::DamageFilterParams P{surf.data(), mirror, stamp.data(), &arrivals, count + 1, 7, n_pending, W, H, gx, gy, all, fill};
  fdh::launch_damage_filter(nullptr, P);
  printf("%u\n", count[1]);
  for (int i = 0; i < pad; i++) {
    if (mirror[(size_t)nb * 4096 + i] != 0xEEEEEEEEu) { printf("mirror overrun\n"); return 1; }
    if (stamp[(size_t)nb + i] != 0xEEEEEEEEu) { printf("stamp overrun\n"); return 1; }
  }
  for (int i = 0; i < 2 + pad; i++) if (i != 1 && count[i] != 0xEEEEEEEEu) { printf("count overrun\n"); return 1; }
  FILE* f = fopen("mirror_out.raw", "wb"); fwrite(mirror, 4, (size_t)nb * 4096, f); fclose(f);
  f = fopen("stamps_out.raw", "wb"); fwrite(stamp.data(), 4, nb, f); fclose(f);
  return 0;
}
