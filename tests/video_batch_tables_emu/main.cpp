// The tables of a batch of video frames (figdraw_amd/csrc/fdh_video_batch.h, as it stands) on placed frames read from a file; plain C++, no HIP.
//   input:  n_levels first m n, then n lines "x y w h format flags"
//   output: what was reserved, then the tables as the batched kernels read them (tests/test_video_frames_host.py compares them with its own)
#include <cstdio>
#include <cstring>
#include <vector>

#include "fdh_video_batch.h"

namespace ii = fdh::image_import;
namespace vi = fdh::video_import;
namespace vb = fdh::video_batch;
int main(int argc, char** argv) {
  FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
  int n_levels, first, m, n;
  if (!f || std::fscanf(f, "%d %d %d %d", &n_levels, &first, &m, &n) != 4 || n < 1 || first < 0 || m < 1 || first + m > n) return 2;
  std::vector<vi::BatchFrame> tab((size_t)n);
  for (auto& t : tab) {
    t = vi::BatchFrame{};
    if (std::fscanf(f, "%d %d %d %d %u %u", &t.x, &t.y, &t.w, &t.h, &t.format, &t.flags) != 6 || t.format > vi::kP010) return 2;
  }
  std::fclose(f);
  std::printf("reserved %zu\n", vb::table_words(tab, n_levels));
  vb::Tables T;
  vb::tables(tab, first, m, n_levels, &T);
  std::printf("n_tiles %u n_tails %u ink_blocks %u words %zu at %zu %zu %zu %zu\n", T.n_tiles, T.n_tails, T.ink_blocks, T.words.size(), T.tail_records_at, T.tiles_at, T.tails_at, T.owner_at);
  std::printf("groups");
  for (int k = 0; k < vb::kGroups; k++) std::printf(" %u %u", T.tile_first[k], T.tile_count[k]);
  std::printf("\n");
  std::vector<vi::BatchFrame> g((size_t)m);  // the records as they are copied to the device
  std::memcpy(g.data(), T.words.data(), (size_t)m * sizeof(vi::BatchFrame));
  for (int k = 0; k < m; k++) {
    std::printf("frame %d at %d %d size %d %d n_store %d ink %d scratch_off %u ink_off %u owner_off %u lw", k, g[k].x, g[k].y, g[k].w, g[k].h, g[k].n_store, g[k].ink, g[k].scratch_off,
                g[k].ink_off, g[k].owner_off);
    for (int l = 0; l < ii::kTileLevels; l++) std::printf(" %d", g[k].lw[l]);
    std::printf(" lh");
    for (int l = 0; l < ii::kTileLevels; l++) std::printf(" %d", g[k].lh[l]);
    std::printf("\n");
  }
  std::vector<ii::BatchImage> r((size_t)T.n_tails);  // ... and the tails', of which the tail's kernel reads these fields
  if (T.n_tails) std::memcpy(r.data(), T.words.data() + T.tail_records_at, (size_t)T.n_tails * sizeof(ii::BatchImage));
  for (uint32_t k = 0; k < T.n_tails; k++) {
    std::printf("tail %u at %d %d size %d %d n_store %d scratch_off %u owner_off %u lw", k, r[k].x, r[k].y, r[k].w, r[k].h, r[k].n_store, r[k].scratch_off, r[k].owner_off);
    for (int l = 0; l < ii::kTileLevels; l++) std::printf(" %d", r[k].lw[l]);
    std::printf(" lh");
    for (int l = 0; l < ii::kTileLevels; l++) std::printf(" %d", r[k].lh[l]);
    std::printf("\n");
  }
  std::printf("tiles");
  for (size_t i = T.tiles_at; i < T.tails_at; i++) std::printf(" %u", T.words[i]);
  std::printf("\ntails");
  for (size_t i = T.tails_at; i < T.owner_at; i++) std::printf(" %u", T.words[i]);
  std::printf("\nowner");
  for (size_t i = T.owner_at; i < T.words.size(); i++) std::printf(" %u", T.words[i]);
  std::printf("\n");
  return 0;
}
