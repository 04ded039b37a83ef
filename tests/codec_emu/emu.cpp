// tests/codec_emu/emu.cpp -- figdraw_amd/csrc/k_damage_codec.hip under the threaded host shim (tests/emu/fdh_device_threads.h as
// fdh_device.h, and tests/emu/fdh_damage.h, copied beside this file with the kernel and fdh_damage_read.h: tests/test_damage_stream_host.py).
// usage: emu W H frame.raw all(0|1) stamps.raw|-   (stamp 7 = pending) -> writes dir.bin and payload.bin, prints
// n_tiles and payload_bytes; fails when a byte past either buffer was written
#include "k_damage_codec.hip"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
  int W = atoi(argv[1]), H = atoi(argv[2]);
  std::vector<uint32_t> surf((size_t)W * H);
  FILE* f = fopen(argv[3], "rb"); if (!f || fread(surf.data(), 4, surf.size(), f) != surf.size()) return 2; fclose(f);
  int all = atoi(argv[4]);
  int gx = (W + 63) / 64, gy = (H + 63) / 64, nb = gx * gy;
  std::vector<uint32_t> stamp(nb, 0);
  uint32_t n_pending = nb;
  if (!all) { f = fopen(argv[5], "rb"); if (!f || fread(stamp.data(), 4, nb, f) != (size_t)nb) return 2; fclose(f); n_pending = 0; for (auto s : stamp) n_pending += s == 7; }
  std::vector<uint8_t> payload((size_t)nb * 16384 + 64, 0xEE), dir((size_t)nb * 24 + 64, 0xEE);
  uint32_t counts[2] = {~0u, ~0u};
  unsigned long long cursor = 0;
  fdh::DamageEncodeParams P{surf.data(), stamp.data(), payload.data(), (uint2*)dir.data(), counts, counts + 1, &cursor, 7, n_pending, W, H, gx, gy, all};
  fdh::launch_damage_encode(nullptr, P);
  printf("%u %u\n", counts[0], counts[1]);
  for (size_t i = (size_t)nb * 16384; i < payload.size(); i++) if (payload[i] != 0xEE) { printf("payload overrun\n"); return 1; }
  for (size_t i = (size_t)nb * 24; i < dir.size(); i++) if (dir[i] != 0xEE) { printf("dir overrun\n"); return 1; }
  f = fopen("dir.bin", "wb"); fwrite(dir.data(), 24, counts[0], f); fclose(f);
  f = fopen("payload.bin", "wb"); fwrite(payload.data(), 1, counts[1], f); fclose(f);
  return 0;
}
