// The tables of a batch of device images (figdraw_amd/csrc/fdh_image_batch.h, as it stands) on placed images read from a file; plain C++, no HIP.
//   input:  n_levels first m n, then n lines "x y w h format"
//   output: what was reserved, then the tables as the batched kernels read them (tests/test_device_images_host.py compares them with its own)
#include <cstdio>
#include <cstring>
#include <vector>

#include "fdh_image_batch.h"

namespace ii = fdh::image_import;
namespace ib = fdh::image_batch;
int main(int argc, char** argv) {
  FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
  int n_levels, first, m, n;
  if (!f || std::fscanf(f, "%d %d %d %d", &n_levels, &first, &m, &n) != 4 || n < 1 || first < 0 || m < 1 || first + m > n) return 2;
  std::vector<ii::BatchImage> tab((size_t)n);
  for (auto& t : tab) {
    t = ii::BatchImage{};
    if (std::fscanf(f, "%d %d %d %d %u", &t.x, &t.y, &t.w, &t.h, &t.format) != 5) return 2;
  }
  std::fclose(f);
  std::printf("reserved %zu\n", ib::table_words(tab, n_levels));
  ib::Tables T;
  ib::tables(tab, first, m, n_levels, &T);
  std::printf("n_tiles %u n_tails %u ink_blocks %u words %zu at %zu %zu %zu\n", T.n_tiles, T.n_tails, T.ink_blocks, T.words.size(), T.tiles_at, T.tails_at, T.owner_at);
  std::printf("groups");
  for (int k = 0; k < ib::kFormats; k++) std::printf(" %u %u", T.tile_first[k], T.tile_count[k]);
  std::printf("\n");
  std::vector<ii::BatchImage> g((size_t)m);  // the records as they are copied to the device
  std::memcpy(g.data(), T.words.data(), (size_t)m * sizeof(ii::BatchImage));
  for (int k = 0; k < m; k++) {
    std::printf("image %d at %d %d size %d %d n_store %d ink %d scratch_off %u ink_off %u owner_off %u lw", k, g[k].x, g[k].y, g[k].w, g[k].h, g[k].n_store, g[k].ink, g[k].scratch_off,
                g[k].ink_off, g[k].owner_off);
    for (int l = 0; l < ii::kTileLevels; l++) std::printf(" %d", g[k].lw[l]);
    std::printf(" lh");
    for (int l = 0; l < ii::kTileLevels; l++) std::printf(" %d", g[k].lh[l]);
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
