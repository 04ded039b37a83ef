// tests/msdf_batch_emu/emu.cpp -- the batched kernels of figdraw_amd/csrc/k_msdf.hip (k_msdf_generate_batch, k_msdf_generate_union_batch,
// k_msdf_correct_batch, k_msdf_correct_union_batch: fdh_put_glyph_outlines, include_glyphs/figdraw_hip_glyphs.h) against the single launchers of the
// same file, under the sequential host shim of tests/emu, which tests/test_msdf_batch_host.py copies here as fdh_device.h together with
// k_msdf.hip and fdh_msdf_host.h from csrc, unmodified.
// usage: emu batch.raw     batch.raw: int32 n, then per glyph int32 w, h, range, n_segs and n_segs x 6 float32 (cx = NaN for a line)
// The fields of all glyphs lie in one buffer with 64 words of 0xEE before the first, between two and behind the last; the tables and the
// records are sized exactly.  In all four flag combinations every glyph's bytes must be the single launcher's, no pad may be written, and
// the correction must not write its input.
// -> prints one line per combination and "glyphs N tiles T edges E"; exit 0: all equal; 1: a difference, an overrun or a written input;
//    3: an open contour; 4: see the shim
#include "fdh_device.h"
#include "k_msdf.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
namespace {
constexpr int kPad = 64;
struct Glyph { int w, h, range, n_edges; float orient; std::vector<float> rec; size_t at; };  // at: the field's first word in the buffer
bool pads_intact(const std::vector<uint32_t>& v, const std::vector<Glyph>& gs) {
  size_t i = 0;
  for (const Glyph& g : gs) {
    for (; i < g.at; i++) if (v[i] != 0xEEEEEEEEu) return false;
    i += (size_t)g.w * g.h;
  }
  for (; i < v.size(); i++) if (v[i] != 0xEEEEEEEEu) return false;
  return true;
}
}  // namespace
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
  std::vector<Glyph> gs((size_t)n);
  size_t words = kPad, n_tiles = 0, n_edges = 0;
  for (Glyph& g : gs) {
    int32_t head[4];
    if (fread(head, 4, 4, f) != 4) return 2;
    g.w = head[0]; g.h = head[1]; g.range = head[2];
    std::vector<float> segs((size_t)head[3] * 6);
    if (!segs.empty() && fread(segs.data(), 4, segs.size(), f) != segs.size()) return 2;
    fdh::msdf::Shape shape;
    if (!fdh::msdf::build_shape(segs.data(), head[3], &shape)) return 3;
    fdh::msdf::edge_records(shape, &g.rec);
    g.n_edges = (int)shape.edges.size(); g.orient = (float)shape.orient;
    g.at = words;
    words += (size_t)g.w * g.h + kPad;
    n_tiles += (size_t)((g.w + 7) / 8) * ((g.h + 7) / 8);
    n_edges += (size_t)g.n_edges;
  }
  fclose(f);
  // the batch's tables, as batch_tables (fdh_glyph_tables.h) builds them for put_glyph_outlines (the field offsets here step over the pads)
  std::vector<float> rec;
  std::vector<fdh::msdf::BatchGlyph> tab((size_t)n);
  std::vector<uint32_t> tile_glyph;
  for (int k = 0; k < n; k++) {
    const Glyph& g = gs[(size_t)k];
    fdh::msdf::BatchGlyph& t = tab[(size_t)k];
    t = fdh::msdf::BatchGlyph{};
    t.edge_off = (uint32_t)(rec.size() / fdh::msdf::kEdgeFloats); t.n_edges = g.n_edges; t.w = g.w; t.h = g.h;
    t.orient = g.orient; t.inv_range = 1.0f / (float)g.range; t.step = (float)g.range / 255.0f;
    t.field_off = (uint32_t)g.at; t.first_tile = (uint32_t)tile_glyph.size();
    rec.insert(rec.end(), g.rec.begin(), g.rec.end());
    tile_glyph.insert(tile_glyph.end(), (size_t)((g.w + 7) / 8) * ((g.h + 7) / 8), (uint32_t)k);
  }
  rec.shrink_to_fit(); tile_glyph.shrink_to_fit();
  int bad = 0;
  for (int overlap = 0; overlap < 2; overlap++) {
    std::vector<uint32_t> field(words, 0xEEEEEEEEu), fixed(words, 0xEEEEEEEEu);
    fdh::launch_msdf_generate_batch(nullptr, overlap != 0, rec.data(), tab.data(), tile_glyph.data(), (int)n_tiles, field.data());
    uint32_t* in = new uint32_t[words];  // no slack at all around what the correction reads
    memcpy(in, field.data(), words * 4);
    fdh::launch_msdf_correct_batch(nullptr, overlap != 0, rec.data(), tab.data(), tile_glyph.data(), (int)n_tiles, in, fixed.data());
    const bool input_written = memcmp(in, field.data(), words * 4) != 0;
    delete[] in;
    int differ_plain = 0, differ_fixed = 0;
    for (const Glyph& g : gs) {
      const size_t npx = (size_t)g.w * g.h;
      std::vector<uint32_t> one(npx, 0xEEEEEEEEu), two(npx, 0xEEEEEEEEu);
      (overlap ? fdh::launch_msdf_generate_union : fdh::launch_msdf_generate)(nullptr, g.rec.data(), g.n_edges, g.w, g.h, g.orient, (float)g.range, one.data());
      (overlap ? fdh::launch_msdf_correct_union : fdh::launch_msdf_correct)(nullptr, g.rec.data(), g.n_edges, g.w, g.h, g.orient, (float)g.range, one.data(), two.data());
      differ_plain += memcmp(one.data(), field.data() + g.at, npx * 4) != 0;
      differ_fixed += memcmp(two.data(), fixed.data() + g.at, npx * 4) != 0;
    }
    const bool overrun = !pads_intact(field, gs) || !pads_intact(fixed, gs);
    printf("overlap %d: generate: %d of %d glyphs differ; correct: %d differ%s%s\n", overlap, differ_plain, n, differ_fixed, overrun ? "; overrun" : "",
           input_written ? "; the input was written" : "");
    bad += differ_plain + differ_fixed + overrun + input_written;
  }
  printf("glyphs %d tiles %zu edges %zu\n", n, n_tiles, n_edges);
  return bad ? 1 : 0;
}
