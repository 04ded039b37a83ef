// tests/codec_emu/fdh_damage.h -- the shim's side of DamageEncodeParams (a copy of the block in figdraw_amd/csrc/fdh_damage.h: keep the two
// alike) and a launcher that runs the workgroups one after the other
#pragma once
namespace fdh {
struct DamageEncodeParams {
  const uint32_t* surf; const uint32_t* stamp; uint8_t* payload; uint2* dir; uint32_t* n_tiles; uint32_t* payload_bytes;
  unsigned long long* cursor; uint32_t epoch, n_pending; int W, H, bins_x, bins_y, all;
};
void k_damage_encode(const DamageEncodeParams P);
// one workgroup at a time (the shared struct is a static), 256 threads
inline void emu_launch(int grid, const DamageEncodeParams& P) {
  for (int b = 0; b < grid; b++) {
    std::barrier<> bar(256);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back([&, t, b] { threadIdx.x = t; blockIdx.x = b; try { k_damage_encode(P); } catch (int) {} bar.arrive_and_drop(); });
    for (auto& x : th) x.join();
  }
}
void launch_damage_encode(hipStream_t s, const DamageEncodeParams& P);
}
