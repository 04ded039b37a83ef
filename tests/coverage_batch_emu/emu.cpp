// tests/coverage_batch_emu/emu.cpp -- the batched coverage kernels of figdraw_amd/csrc/k_atlas_upload.hip (k_coverage_cells_batch,
// k_coverage_sum_batch, k_lcd_filter_batch: fdh_put_glyph_coverage_batch, include_glyphs/figdraw_hip_coverage.h) against the single launchers of the
// same file (k_rasterize_lines, k_lcd_filter), under the sequential host shim (tests/emu/fdh_device.h), which tests/test_coverage_batch_host.py copies into a
// scratch directory together with k_atlas_upload.hip and fdh_msdf_host.h from csrc, unmodified.
// usage: emu batch.raw out.raw     batch.raw: int32 n, then per glyph int32 w, h, n_lines and n_lines x 4 float32 (x0, y0, x1, y1)
// The images of all glyphs lie in one buffer (and its twin) with 64 words of 0xEE before the first, between two and behind the last; the
// lines and the tables are sized exactly.  The tables are built as batch_tables (fdh_glyph_tables.h) builds them for put_glyph_coverage_batch: a glyph 1 texel wide or
// high has no tiles, and its region must stay as it was.  Every other glyph's bytes must be the single launcher's, unfiltered and
// filtered; no pad may be written, nor the lines, the tables or the filter's input.
// -> out.raw: per glyph w x h words unfiltered, then w x h words filtered (a glyph without tiles: 0xEE), for the caller to compare with the
//    oracle; prints "coverage: D of N glyphs differ; lcd: D differ ..." and "glyphs N tiles T lines L"; exit 0: all equal; 1: a difference,
//    an overrun or a written input
#include "fdh_device.h"
#include "k_atlas_upload.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
namespace {
constexpr int kPad = 64;
struct Glyph { int w, h, n_lines; std::vector<float> lines; size_t at; bool tiles; };  // at: the image's first word in the buffers
bool pads_intact(const std::vector<uint32_t>& v, const std::vector<Glyph>& gs) {
  size_t i = 0;
  for (const Glyph& g : gs) {
    for (; i < g.at; i++) if (v[i] != 0xEEEEEEEEu) return false;
    const size_t end = g.at + (size_t)g.w * g.h;
    if (g.tiles) i = end;
    else for (; i < end; i++) if (v[i] != 0xEEEEEEEEu) return false;
  }
  for (; i < v.size(); i++) if (v[i] != 0xEEEEEEEEu) return false;
  return true;
}
template <typename T> T* exact_copy(const std::vector<T>& v) {  // no slack at all around what a kernel reads
  T* p = new T[v.size() ? v.size() : 1];
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}
}  // namespace
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
  std::vector<Glyph> gs((size_t)n);
  size_t words = kPad;
  for (Glyph& g : gs) {
    int32_t head[3];
    if (fread(head, 4, 3, f) != 3) return 2;
    g.w = head[0]; g.h = head[1]; g.n_lines = head[2];
    g.lines.resize((size_t)g.n_lines * 4);
    if (!g.lines.empty() && fread(g.lines.data(), 4, g.lines.size(), f) != g.lines.size()) return 2;
    g.tiles = g.w > 1 && g.h > 1;
    g.at = words;
    words += (size_t)g.w * g.h + kPad;
  }
  fclose(f);
  std::vector<float> lines;
  std::vector<fdh::msdf::BatchGlyph> tab((size_t)n);
  std::vector<uint32_t> tile_glyph;
  for (int k = 0; k < n; k++) {
    const Glyph& g = gs[(size_t)k];
    fdh::msdf::BatchGlyph& t = tab[(size_t)k];
    t = fdh::msdf::BatchGlyph{};
    t.edge_off = (uint32_t)(lines.size() / 4); t.n_edges = g.n_lines; t.w = g.w; t.h = g.h;
    t.field_off = (uint32_t)g.at; t.first_tile = (uint32_t)tile_glyph.size();
    lines.insert(lines.end(), g.lines.begin(), g.lines.end());
    if (g.tiles) tile_glyph.insert(tile_glyph.end(), (size_t)((g.w + 7) / 8) * ((g.h + 7) / 8), (uint32_t)k);
  }
  const int n_tiles = (int)tile_glyph.size();
  float* d_lines = exact_copy(lines);
  fdh::msdf::BatchGlyph* d_tab = exact_copy(tab);
  uint32_t* d_tiles = exact_copy(tile_glyph);
  std::vector<uint32_t> field(words, 0xEEEEEEEEu), spare(words, 0xEEEEEEEEu);
  fdh::launch_coverage_batch(nullptr, reinterpret_cast<const float4*>(d_lines), d_tab, d_tiles, n_tiles, reinterpret_cast<float*>(spare.data()), field.data());
  bool overrun = !pads_intact(field, gs) || !pads_intact(spare, gs);
  uint32_t* in = new uint32_t[words];
  memcpy(in, field.data(), words * 4);
  std::vector<uint32_t> filtered(words, 0xEEEEEEEEu);
  fdh::launch_lcd_filter_batch(nullptr, d_tab, d_tiles, n_tiles, in, filtered.data());
  overrun = overrun || !pads_intact(filtered, gs);
  const bool input_written = memcmp(in, field.data(), words * 4) != 0 || (!lines.empty() && memcmp(d_lines, lines.data(), lines.size() * 4) != 0) ||
                             (n > 0 && memcmp(d_tab, tab.data(), tab.size() * sizeof tab[0]) != 0) ||
                             (n_tiles > 0 && memcmp(d_tiles, tile_glyph.data(), tile_glyph.size() * 4) != 0);
  delete[] in;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  int differ_plain = 0, differ_lcd = 0;
  for (const Glyph& g : gs) {
    const size_t npx = (size_t)g.w * g.h;
    fwrite(field.data() + g.at, 4, npx, o);
    fwrite(filtered.data() + g.at, 4, npx, o);
    if (!g.tiles) continue;  // (pads_intact has looked at its region)
    std::vector<uint32_t> one(npx, 0xEEEEEEEEu), two(npx, 0xEEEEEEEEu);
    std::vector<float> scratch((size_t)g.h * (g.w + 2));
    float* own = exact_copy(g.lines);
    fdh::launch_rasterize_lines(nullptr, reinterpret_cast<const float4*>(own), g.n_lines, g.w, g.h, scratch.data(), one.data());
    fdh::launch_lcd_filter(nullptr, one.data(), two.data(), g.w, g.h);
    delete[] own;
    differ_plain += memcmp(one.data(), field.data() + g.at, npx * 4) != 0;
    differ_lcd += memcmp(two.data(), filtered.data() + g.at, npx * 4) != 0;
  }
  fclose(o);
  delete[] d_lines; delete[] d_tab; delete[] d_tiles;
  printf("coverage: %d of %d glyphs differ; lcd: %d differ%s%s\n", differ_plain, n, differ_lcd, overrun ? "; overrun" : "", input_written ? "; an input was written" : "");
  printf("glyphs %d tiles %d lines %zu\n", n, n_tiles, lines.size() / 4);
  return differ_plain + differ_lcd + overrun + input_written ? 1 : 0;
}
