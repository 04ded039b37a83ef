// The tables of a batch of glyphs (figdraw_amd/csrc/fdh_glyph_tables.h, as it stands) on placed glyphs read from a file; plain C++, no HIP.
//   input:  n_levels thin_tiles first m n, then n lines "x y w h n_edges" (edge_off: the running sum of n_edges, as pass 1 leaves it)
//   output: what was reserved, then the tables as the batched kernels read them (tests/test_glyph_tables_host.py compares them with its own)
#include <cstdio>
#include <cstring>
#include <vector>

#include "fdh_glyph_tables.h"

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
  int n_levels, thin, first, m, n;
  if (!f || std::fscanf(f, "%d %d %d %d %d", &n_levels, &thin, &first, &m, &n) != 5 || n < 1 || first < 0 || m < 1 || first + m > n) return 2;
  std::vector<fdh::msdf::BatchGlyph> tab((size_t)n);
  uint32_t edges = 0;
  for (auto& t : tab) {
    t = fdh::msdf::BatchGlyph{};
    if (std::fscanf(f, "%d %d %d %d %d", &t.x, &t.y, &t.w, &t.h, &t.n_edges) != 5) return 2;
    t.edge_off = edges;
    edges += (uint32_t)t.n_edges;
  }
  std::fclose(f);
  std::printf("reserved %zu\n", fdh::batch_table_words(tab, thin != 0, n_levels));
  fdh::BatchTables T;
  fdh::batch_tables(tab, first, m, thin != 0, n_levels, &T);
  std::printf("n_tiles %u n_edges %u words %zu\n", T.n_tiles, T.n_edges, T.words.size());
  std::vector<fdh::msdf::BatchGlyph> g((size_t)m);  // the records as they are copied to the device
  std::memcpy(g.data(), T.words.data(), (size_t)m * sizeof(fdh::msdf::BatchGlyph));
  for (int k = 0; k < m; k++)
    std::printf("glyph %d at %d %d size %d %d edge_off %u n_edges %d field_off %u first_tile %u owner_off %u\n", k, g[k].x, g[k].y, g[k].w, g[k].h, g[k].edge_off, g[k].n_edges, g[k].field_off,
                g[k].first_tile, g[k].owner_off);
  const size_t tiles_at = (size_t)m * fdh::kBatchGlyphWords;
  std::printf("tiles");
  for (size_t i = 0; i < T.n_tiles; i++) std::printf(" %u", T.words[tiles_at + i]);
  std::printf("\nowner");
  for (size_t i = tiles_at + T.n_tiles; i < T.words.size(); i++) std::printf(" %u", T.words[i]);
  std::printf("\n");
  return 0;
}
