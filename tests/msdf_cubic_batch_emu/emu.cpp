// tests/msdf_cubic_batch_emu/emu.cpp -- the batched kernels of figdraw_amd/csrc/k_msdf_cubic.hip (k_msdf_generate_cubic_batch,
// k_msdf_correct_cubic_batch: fdh_put_glyph_outlines_cubic, include_glyphs/figdraw_hip_cubic_batch.h) against the single launchers of the same file
// and, for a glyph without a cubic, against k_msdf.hip's, under the sequential host shim of tests/emu, which
// tests/test_msdf_cubic_batch_host.py copies here as fdh_device.h together with k_msdf_cubic.hip, fdh_msdf_cubic_host.h, k_msdf.hip and
// fdh_msdf_host.h from csrc, unmodified.
// usage: emu batch.raw [FIRST]   batch.raw: int32 n, then per glyph int32 w, h, range, n_segs and n_segs x 8 float32 (c2x = NaN: a
//                                quadratic, c1x = NaN: a line).  FIRST (default 0): the batch is cut there as after a growth of the atlas --
//                                the tables are those of glyphs FIRST .. n - 1, edge_off rebased to the first of them (batch_tables, fdh_glyph_tables.h),
//                                and the records are that slice alone.
// The fields of the glyphs lie in one buffer with 64 words of 0xEE before the first, between two and behind the last; the tables and the
// records are sized exactly.  Every glyph's bytes must be the single launchers' (k_msdf_generate_cubic, then k_msdf_correct_cubic on what
// it made), a cubic-free glyph's also k_msdf_generate's and k_msdf_correct's on the six-float outline; no pad may be written, and the
// correction must not write its input.
// -> prints "generate: A of N glyphs differ; correct: B differ; cubic-free: L glyphs, C differ from k_msdf.hip" and
//    "glyphs N tiles T edges E cubics Q"; exit 0: all equal; 1: a difference, an overrun or a written input; 3: an open contour; 4: see the shim
#include "fdh_device.h"
#include "k_msdf.hip"
#include "k_msdf_cubic.hip"
#include <cstring>
namespace {
namespace mc = fdh::msdf::cubic;
constexpr int kPad = 64;
struct Glyph {
  int w, h, range, n_edges;
  float orient;
  bool cubic_free;
  std::vector<float> segs, rec;
  size_t at;  // the field's first word in the buffer
};
bool pads_intact(const std::vector<uint32_t>& v, const std::vector<Glyph>& gs, size_t first) {
  size_t i = 0;
  for (size_t k = first; k < gs.size(); k++) {
    for (; i < gs[k].at; i++) if (v[i] != 0xEEEEEEEEu) return false;
    i += (size_t)gs[k].w * gs[k].h;
  }
  for (; i < v.size(); i++) if (v[i] != 0xEEEEEEEEu) return false;
  return true;
}
}  // namespace
int main(int argc, char** argv) {
  if (argc != 2 && argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
  const int first = argc == 3 ? atoi(argv[2]) : 0;
  if (first < 0 || first >= n) return 2;
  std::vector<Glyph> gs((size_t)n);
  std::vector<float> all_rec;  // of the WHOLE batch, as pass 1 leaves them
  std::vector<fdh::msdf::BatchGlyph> tab((size_t)n);
  int cubics = 0;
  for (int k = 0; k < n; k++) {
    Glyph& g = gs[(size_t)k];
    int32_t head[4];
    if (fread(head, 4, 4, f) != 4) return 2;
    g.w = head[0]; g.h = head[1]; g.range = head[2];
    g.segs.resize((size_t)head[3] * 8);
    if (!g.segs.empty() && fread(g.segs.data(), 4, g.segs.size(), f) != g.segs.size()) return 2;
    mc::Shape shape;
    if (!mc::build_shape(g.segs.data(), head[3], &shape)) return 3;
    mc::edge_records(shape, &g.rec);
    g.n_edges = (int)shape.edges.size(); g.orient = (float)shape.orient;
    g.cubic_free = !mc::holds_cubic(g.segs.data(), head[3]);
    if (k >= first) for (const mc::Edge& e : shape.edges) cubics += e.kind == mc::kCubic;
    fdh::msdf::BatchGlyph& t = tab[(size_t)k];
    t = fdh::msdf::BatchGlyph{};
    t.edge_off = (uint32_t)(all_rec.size() / mc::kCubicEdgeFloats); t.n_edges = g.n_edges; t.w = g.w; t.h = g.h;
    t.orient = g.orient; t.inv_range = 1.0f / (float)g.range; t.step = (float)g.range / 255.0f;
    all_rec.insert(all_rec.end(), g.rec.begin(), g.rec.end());
  }
  fclose(f);
  // the tables of glyphs first .. n - 1, as batch_tables (fdh_glyph_tables.h) builds them (the field offsets here step over the pads)
  const uint32_t edge_base = tab[(size_t)first].edge_off;
  std::vector<float> rec(all_rec.begin() + (size_t)edge_base * mc::kCubicEdgeFloats, all_rec.end());
  std::vector<fdh::msdf::BatchGlyph> sub;
  std::vector<uint32_t> tile_glyph;
  size_t words = kPad, n_edges = 0;
  for (int k = first; k < n; k++) {
    Glyph& g = gs[(size_t)k];
    fdh::msdf::BatchGlyph t = tab[(size_t)k];
    g.at = words;
    words += (size_t)g.w * g.h + kPad;
    t.edge_off -= edge_base; t.field_off = (uint32_t)g.at; t.first_tile = (uint32_t)tile_glyph.size();
    tile_glyph.insert(tile_glyph.end(), (size_t)((g.w + 7) / 8) * ((g.h + 7) / 8), (uint32_t)(k - first));
    n_edges += (size_t)g.n_edges;
    sub.push_back(t);
  }
  rec.shrink_to_fit(); sub.shrink_to_fit(); tile_glyph.shrink_to_fit();
  const int m = n - first, n_tiles = (int)tile_glyph.size();
  std::vector<uint32_t> field(words, 0xEEEEEEEEu), fixed(words, 0xEEEEEEEEu);
  fdh::launch_msdf_generate_cubic_batch(nullptr, rec.data(), sub.data(), tile_glyph.data(), n_tiles, field.data());
  uint32_t* in = new uint32_t[words];  // no slack at all around what the correction reads
  memcpy(in, field.data(), words * 4);
  fdh::launch_msdf_correct_cubic_batch(nullptr, rec.data(), sub.data(), tile_glyph.data(), n_tiles, in, fixed.data());
  const bool input_written = memcmp(in, field.data(), words * 4) != 0;
  delete[] in;
  int differ_plain = 0, differ_fixed = 0, lifted = 0, differ_lifted = 0;
  for (int k = first; k < n; k++) {
    const Glyph& g = gs[(size_t)k];
    const size_t npx = (size_t)g.w * g.h;
    std::vector<uint32_t> one(npx, 0xEEEEEEEEu), two(npx, 0xEEEEEEEEu);
    fdh::launch_msdf_generate_cubic(nullptr, g.rec.data(), g.n_edges, g.w, g.h, g.orient, (float)g.range, one.data());
    fdh::launch_msdf_correct_cubic(nullptr, g.rec.data(), g.n_edges, g.w, g.h, g.orient, (float)g.range, one.data(), two.data());
    differ_plain += memcmp(one.data(), field.data() + g.at, npx * 4) != 0;
    differ_fixed += memcmp(two.data(), fixed.data() + g.at, npx * 4) != 0;
    if (!g.cubic_free) continue;
    lifted++;
    std::vector<float> six, rec6;
    const int n_segs = (int)(g.segs.size() / 8);
    mc::to_quadratic_format(g.segs.data(), n_segs, &six);
    fdh::msdf::Shape s6;
    if (!fdh::msdf::build_shape(six.data(), n_segs, &s6)) return 3;
    fdh::msdf::edge_records(s6, &rec6);
    std::fill(one.begin(), one.end(), 0xEEEEEEEEu); std::fill(two.begin(), two.end(), 0xEEEEEEEEu);
    fdh::launch_msdf_generate(nullptr, rec6.data(), (int)s6.edges.size(), g.w, g.h, (float)s6.orient, (float)g.range, one.data());
    fdh::launch_msdf_correct(nullptr, rec6.data(), (int)s6.edges.size(), g.w, g.h, (float)s6.orient, (float)g.range, one.data(), two.data());
    differ_lifted += memcmp(one.data(), field.data() + g.at, npx * 4) != 0 || memcmp(two.data(), fixed.data() + g.at, npx * 4) != 0;
  }
  const bool overrun = !pads_intact(field, gs, (size_t)first) || !pads_intact(fixed, gs, (size_t)first);
  printf("generate: %d of %d glyphs differ; correct: %d differ; cubic-free: %d glyphs, %d differ from k_msdf.hip%s%s\n", differ_plain, m, differ_fixed, lifted, differ_lifted,
         overrun ? "; overrun" : "", input_written ? "; the input was written" : "");
  printf("glyphs %d tiles %d edges %zu cubics %d\n", m, n_tiles, n_edges, cubics);
  return differ_plain + differ_fixed + differ_lifted + overrun + input_written ? 1 : 0;
}
