// tests/move_emu/emu.cpp -- the three kernels of k_damage_move.hip on a CPU.
// usage: emu W H new.raw mirror.raw stamps_pre.raw|- stamps_post.raw max_shift n_moves dx dy ...   (stamp 7 = pending; "-": all = 1)
//   1. k_damage_move_votes and k_damage_move_match over the pre-filter set (new.raw = the surface, mirror.raw = the tile-major mirror of
//      the frame the receiver holds)                                                    -> votes.bin (2 x 513 uint32), moved.bin (a byte a bin)
//   2. k_damage_encode_moved over the post-filter set (what k_damage_filter leaves: the caller works it out) -> dir.bin, payload.bin
// prints n_tiles, payload_bytes and n_copied; fails when a byte past any buffer was written, or surface or mirror changed
#include "k_damage_move.hip"
#include <cstdio>
#include <cstdlib>
static bool load(const char* name, void* p, size_t bytes) {
  FILE* f = fopen(name, "rb");
  const bool ok = f && fread(p, 1, bytes, f) == bytes;
  if (f) fclose(f);
  return ok;
}
static void save(const char* name, const void* p, size_t bytes) { FILE* f = fopen(name, "wb"); fwrite(p, 1, bytes, f); fclose(f); }
int main(int argc, char** argv) {
  if (argc < 9) return 2;
  const int W = atoi(argv[1]), H = atoi(argv[2]);
  const int gx = (W + 63) / 64, gy = (H + 63) / 64, nb = gx * gy;
  std::vector<uint32_t> surf((size_t)W * H), mirror((size_t)nb * 4096), pre(nb, 0), post(nb, 0);
  if (!load(argv[3], surf.data(), surf.size() * 4) || !load(argv[4], mirror.data(), mirror.size() * 4)) return 2;
  const int all = argv[5][0] == '-' && !argv[5][1];
  if (!all && !load(argv[5], pre.data(), (size_t)nb * 4)) return 2;
  if (!load(argv[6], post.data(), (size_t)nb * 4)) return 2;
  const int max_shift = atoi(argv[7]);
  fdh::DamageMoveList L{};
  L.n = atoi(argv[8]);
  if (L.n < 0 || L.n > fdh::kDamageMovesMax || argc < 9 + 2 * L.n) return 2;
  for (int i = 0; i < L.n; i++) { L.dx[i] = (int16_t)atoi(argv[9 + 2 * i]); L.dy[i] = (int16_t)atoi(argv[10 + 2 * i]); }
  const std::vector<uint32_t> surf0 = surf, mirror0 = mirror;
  constexpr int kGuard = 64, kVotes = 2 * fdh::kDamageVoteSpan;

  std::vector<uint32_t> votes(kVotes + kGuard, 0);
  for (int i = kVotes; i < kVotes + kGuard; i++) votes[i] = 0xEEEEEEEEu;
  fdh::DamageMoveVotesParams V{surf.data(), mirror.data(), pre.data(), votes.data(), 7, W, H, gx, gy, all, max_shift};
  fdh::launch_damage_move_votes(nullptr, V);
  for (int i = kVotes; i < kVotes + kGuard; i++) if (votes[i] != 0xEEEEEEEEu) { printf("votes overrun\n"); return 1; }

  std::vector<uint8_t> moved((size_t)nb + kGuard, 0xEE);
  fdh::DamageMoveMatchParams M{surf.data(), mirror.data(), pre.data(), moved.data(), L, 7, W, H, gx, gy, all};
  fdh::launch_damage_move_match(nullptr, M);
  for (size_t i = nb; i < moved.size(); i++) if (moved[i] != 0xEE) { printf("moved overrun\n"); return 1; }

  uint32_t n_pending = 0;
  for (auto s : post) n_pending += s == 7;
  std::vector<uint8_t> payload((size_t)nb * 16384 + kGuard, 0xEE), dir((size_t)nb * 24 + kGuard, 0xEE);
  uint32_t counts[3] = {~0u, ~0u, ~0u};
  unsigned long long cursor = 0;
  fdh::DamageEncodeMovedParams Q{{surf.data(), post.data(), payload.data(), (uint2*)dir.data(), counts, counts + 1, &cursor, 7, n_pending, W, H, gx, gy, 0},
                                 moved.data(), L, counts + 2};
  fdh::launch_damage_encode_moved(nullptr, Q);
  printf("%u %u %u\n", counts[0], counts[1], counts[2]);
  for (size_t i = (size_t)nb * 16384; i < payload.size(); i++) if (payload[i] != 0xEE) { printf("payload overrun\n"); return 1; }
  for (size_t i = (size_t)nb * 24; i < dir.size(); i++) if (dir[i] != 0xEE) { printf("dir overrun\n"); return 1; }
  if (surf != surf0 || mirror != mirror0) { printf("the surface or the mirror was written\n"); return 1; }
  save("votes.bin", votes.data(), (size_t)kVotes * 4);
  save("moved.bin", moved.data(), (size_t)nb);
  if (n_pending) { save("dir.bin", dir.data(), (size_t)24 * counts[0]); save("payload.bin", payload.data(), counts[1]); }
  return 0;
}
