// tests/codec_emu/fdh_damage.h -- the shim's side of the header of that name: the library's fdh_damage_read.h itself (copied beside it), and a
// launcher that runs the workgroups one after the other
#pragma once
#include "fdh_damage_read.h"
namespace fdh {
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
}
