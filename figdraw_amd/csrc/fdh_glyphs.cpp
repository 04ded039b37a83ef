// fdh_glyphs.cpp -- class GlyphMaker (fdh_glyphs.h): glyph images, outlines and batches of outlines on their way into the atlas, every step a
// kernel on the context's stream.  One body per kind of work: a single put, a batch's pass 1 per kind of glyph, passes 2 and 3 of every
// batch; what the two segment formats differ in is a SegmentFormat.
#include "fdh_glyphs.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <exception>
#include <string>

#include "fdh_kernels.h"
#include "fdh_atlas_move.h"
#include "fdh_place_batch.h"  // Refusal, place_batch
#include "fdh_msdf_cubic_host.h"

namespace fdh {
namespace mc = msdf::cubic;

void GlyphMaker::release() {
  glyph_a_.release(); glyph_b_.release(); glyph_lines_.release(); glyph_acc_.release(); glyph_edges_.release(); glyph_tab_.release(); glyph_src_.release(); move_tab_.release();
}
namespace {
constexpr uint32_t kLcdFlags = FDH_GLYPH_LCD_FILTER | FDH_GLYPH_LCD_CONTEXT;
constexpr uint32_t kFieldFlags = FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT | FDH_GLYPH_MTSDF_OVERLAP | 0xFF00u;  // (0xFF00: the distance range)
}  // namespace

// A rasterised glyph on its way into the atlas, processed on the device: optional LCD filter (applyLcdFilter, common/
// textrasters/pixie_raster.nim:12-43, what renderPixieGlyph does between fillText and loadGlyphImage :83-91), then the
// level chain of updateSubImage (textures.nim:106-119) -- every step a kernel on the context's stream.
void GlyphMaker::put_glyph_image(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const uint8_t* rgba, uint32_t flags, int out_rect[4]) {
  const Refusal bad{"put_glyph_image"};
  if (w <= 0 || h <= 0 || !rgba) throw bad("empty image");
  if (flags & ~kLcdFlags) throw bad("unknown flag");
  const size_t n = (size_t)w * h;
  if (atlas.has_device()) { glyph_a_.reserve(n); glyph_b_.reserve(n); }
  atlas.make_room(s, w, h);
  const AtlasEntry& e = atlas.place(s, key, w, h, out_rect);
  if (!atlas.has_device()) return;
  FDH_HIP(hipMemcpyAsync(glyph_a_.ptr, rgba, n * 4, hipMemcpyHostToDevice, s));
  glyph_to_atlas(s, atlas, glyph_a_.ptr, glyph_b_.ptr, w, h, e.x, e.y, flags);
}
// device image -> (LCD filter) -> atlas level chain, all on the context's stream; waits for it (the caller's buffers are free after)
void GlyphMaker::glyph_to_atlas(hipStream_t s, const Atlas& atlas, uint32_t* cur, uint32_t* nxt, int w, int h, int x, int y, uint32_t flags) {
  if (flags & FDH_GLYPH_LCD_FILTER) { launch_lcd_filter(s, cur, nxt, w, h); std::swap(cur, nxt); }
  atlas.each_level(x, y, w, h, [&](int level, int lx, int ly, int cw, int ch) {
    launch_atlas_blit(s, atlas.level(level), atlas.size() >> level, lx, ly, cur, cw, ch);
    launch_minify2(s, cur, nxt, cw, ch);
    std::swap(cur, nxt);
  });
  FDH_HIP(hipStreamSynchronize(s));
  FDH_HIP(hipGetLastError());
}

// ---- the two segment formats.  generateGlyph's job (common/fontglyphs.nim:61-106) with an own rasteriser in pixie's place: a glyph OUTLINE
// (segments in pixel units of the w x h image, y down; 6 floats: a quadratic, cx = NaN marks a straight line; 8 floats: include_glyphs/
// figdraw_hip_cubic.h) becomes coverage or a distance field on the device and goes into the atlas.  For coverage the curves are flattened
// here on the host (chord error <= 0.025 px; the same float formula as oracle/figdraw_oracle.c, fo_flatten_outline), the area accumulation
// runs in k_rasterize_lines.  pixie's texels are third-party and unpinned: parity is defined against the oracle's restatement
// of the same published algorithm.  For a distance field the host makes contours, the orientation and the coloured edges (fdh_msdf_host.h,
// fdh_msdf_cubic_host.h), the device the texels.
static int flatten_count(const float* q) {
  const float ddx = q[0] - 2.0f * q[2] + q[4], ddy = q[1] - 2.0f * q[3] + q[5];
  const float dev = std::sqrt(ddx * ddx + ddy * ddy);
  const int n = (int)std::ceil(std::sqrt(dev * 10.0f));  // error of n chords = dev / (4 n^2) <= 0.025 px
  return n < 1 ? 1 : (n > 64 ? 64 : n);
}
// the lines (x0, y0, x1, y1) of an outline's n segments of 6 floats, appended (of 8 floats: msdf::cubic::flatten_outline)
static void flatten_outline(const float* segs, int n, std::vector<float>* lines) {
  for (int i = 0; i < n; i++) {
    const float* q = segs + 6 * (size_t)i;
    if (q[2] != q[2]) { lines->insert(lines->end(), {q[0], q[1], q[4], q[5]}); continue; }
    const int k = flatten_count(q);
    float px = q[0], py = q[1];
    for (int j = 1; j <= k; j++) {
      const float t = (float)j / (float)k, u = 1.0f - t;
      const float x = j == k ? q[4] : (u * u) * q[0] + (2.0f * u * t) * q[2] + (t * t) * q[4];
      const float y = j == k ? q[5] : (u * u) * q[1] + (2.0f * u * t) * q[3] + (t * t) * q[5];
      lines->insert(lines->end(), {px, py, x, y});
      px = x; py = y;
    }
  }
}
// steps 1 to 3 of the specification and, where `rec` is given, the kernels' edge records appended to it; false: an open contour.
// (build_shape and edge_records: those of the namespace of Shape.)
template <typename Shape>
static bool shape_records(const float* segs, int n, std::vector<float>* rec, int* n_edges, float* orient) {
  Shape shape;
  if (!build_shape(segs, n, &shape)) return false;
  *n_edges = (int)shape.edges.size();
  *orient = (float)shape.orient;
  if (rec) {
    std::vector<float> one;
    edge_records(shape, &one);
    rec->insert(rec->end(), one.begin(), one.end());
  }
  return true;
}
struct GlyphMaker::SegmentFormat {
  const char *single, *fields, *coverage;  // the three calls that take this format, as their error messages name them
  const char* fields_flags;                // what the batch of distance fields says of a flag that is not its own
  const char* fields_call;                 // that batch as the coverage batch points to it
  int floats;                              // of a segment
  size_t stride;                           // floats of an edge record
  bool (*holds_cubic)(const float* segs, int n);  // null: the format has no cubic
  int (*lines_of)(const float* seg);
  void (*flatten)(const float* segs, int n, std::vector<float>* lines);
  bool (*records)(const float* segs, int n, std::vector<float>* rec, int* n_edges, float* orient);
  static const SegmentFormat& six();
  static const SegmentFormat& eight();
};
// (function-local: a constant at namespace scope would be emitted for the device as well, with these host functions in it)
const GlyphMaker::SegmentFormat& GlyphMaker::SegmentFormat::six() {
  static const SegmentFormat f = {
    "put_glyph_outline", "put_glyph_outlines", "put_glyph_coverage_batch", "unknown flag (coverage glyphs and the LCD flags are not batched)", "fdh_put_glyph_outlines'",
    6, msdf::kEdgeFloats, nullptr, [](const float* q) { return q[2] != q[2] ? 1 : flatten_count(q); }, flatten_outline, shape_records<msdf::Shape>};
  return f;
}
const GlyphMaker::SegmentFormat& GlyphMaker::SegmentFormat::eight() {
  static const SegmentFormat f = {
    "put_glyph_outline_cubic", "put_glyph_outlines_cubic", "put_glyph_coverage_batch_cubic", "unknown flag (coverage glyphs are fdh_put_glyph_coverage_batch_cubic's)", "fdh_put_glyph_outlines_cubic's",
    8, mc::kCubicEdgeFloats, mc::holds_cubic,
    [](const float* q) {
      if (q[2] != q[2]) return 1;
      if (q[4] == q[4]) return mc::cubic_flatten_count(q);
      const float six[6] = {q[0], q[1], q[2], q[3], q[6], q[7]};
      return flatten_count(six);
    },
    mc::flatten_outline, shape_records<mc::Shape>};
  return f;
}

// ---- the single puts
void GlyphMaker::put_glyph_outline(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]) {
  put_outline(SegmentFormat::six(), s, atlas, key, w, h, segs, n, flags, out_rect);
}
// fdh_put_glyph_outline_cubic (the specification: include_glyphs/figdraw_hip_cubic.h): put_glyph_outline for segments of 8 floats.  Without a cubic
// among them it IS that call, on the same segments in its format.  With one: coverage flattens the cubics on the host too and goes the
// coverage put's way; a distance field goes the six-float field's way with the records and the kernels that know cubics (fdh_msdf_cubic_host.h,
// k_msdf_cubic.hip).
void GlyphMaker::put_glyph_outline_cubic(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]) {
  if (n < 0 || (n > 0 && !segs)) throw Refusal{SegmentFormat::eight().single}("bad outline");
  if (mc::holds_cubic(segs, n)) return put_outline(SegmentFormat::eight(), s, atlas, key, w, h, segs, n, flags, out_rect);
  std::vector<float> six;
  mc::to_quadratic_format(segs, n, &six);
  static const float none[6] = {};
  put_outline(SegmentFormat::six(), s, atlas, key, w, h, n > 0 ? six.data() : none, n, flags, out_rect);
}
// An outline in either format (the eight-float one: with a cubic): everything is validated before anything is packed.  Coverage: flattened, then
// put_lines.  FDH_GLYPH_MTSDF (the specification: include/figdraw_hip.h at that flag): put_field.
void GlyphMaker::put_outline(const SegmentFormat& fmt, hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]) {
  const Refusal bad{fmt.single};
  const bool field = (flags & FDH_GLYPH_MTSDF) != 0, overlap = (flags & FDH_GLYPH_MTSDF_OVERLAP) != 0;
  if (w <= 0 || h <= 0 || w > 4096 || h > 4096) throw bad("image size must be in 1..4096");
  if (n < 0 || (n > 0 && !segs)) throw bad("bad outline");
  if (flags & ~(kLcdFlags | kFieldFlags)) throw bad("unknown flag");
  const uint32_t sdf_range = (flags >> 8) & 255u;
  if (sdf_range && (!field || sdf_range > 64u)) throw bad("a distance range needs FDH_GLYPH_MTSDF and is at most 64");
  if ((flags & FDH_GLYPH_MTSDF_CORRECT) && !field) throw bad("FDH_GLYPH_MTSDF_CORRECT needs FDH_GLYPH_MTSDF");
  if (overlap && fmt.holds_cubic) throw bad("FDH_GLYPH_MTSDF_OVERLAP takes no cubic segment");
  if (overlap && !field) throw bad("FDH_GLYPH_MTSDF_OVERLAP needs FDH_GLYPH_MTSDF");
  if (!field) {
    std::vector<float> lines;
    lines.reserve((size_t)n * 16);
    fmt.flatten(segs, n, &lines);
    put_lines(s, atlas, key, w, h, lines, flags, out_rect);
    return;
  }
  if (flags & kLcdFlags) throw bad("a distance field takes no LCD filter");
  if (n > msdf::kMaxSegments) throw bad("a distance field takes at most 65535 segments");
  const FieldKernels kernels = fmt.holds_cubic ? FieldKernels::cubic : overlap ? FieldKernels::overlap : FieldKernels::plain;
  put_field(fmt, kernels, s, atlas, key, w, h, segs, n, sdf_range ? (float)sdf_range : 4.0f, (flags & FDH_GLYPH_MTSDF_CORRECT) != 0, out_rect);
}
// a coverage glyph from its flattened outline: packed, rasterised, filtered, its level chain built
void GlyphMaker::put_lines(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const std::vector<float>& lines, uint32_t flags, int out_rect[4]) {
  const size_t npx = (size_t)w * h, m = lines.size() / 4;
  if (atlas.has_device()) {
    glyph_a_.reserve(npx);
    glyph_b_.reserve(npx);
    glyph_lines_.reserve(std::max<size_t>(lines.size(), 4));
    glyph_acc_.reserve((size_t)h * (w + 2));
  }
  atlas.make_room(s, w, h);
  const AtlasEntry& e = atlas.place(s, key, w, h, out_rect);
  if (!atlas.has_device()) return;
  if (m) FDH_HIP(hipMemcpyAsync(glyph_lines_.ptr, lines.data(), lines.size() * sizeof(float), hipMemcpyHostToDevice, s));
  launch_rasterize_lines(s, reinterpret_cast<const float4*>(glyph_lines_.ptr), (int)m, w, h, glyph_acc_.ptr, glyph_a_.ptr);
  glyph_to_atlas(s, atlas, glyph_a_.ptr, glyph_b_.ptr, w, h, e.x, e.y, flags);  // (synchronises: `lines` stays alive until then)
}
// A distance field: one copy, one launch, then the level chain every glyph image takes.  Nothing is premultiplied and nothing filtered: the
// four bytes of a texel are four distances.  `correct` (FDH_GLYPH_MTSDF_CORRECT, step 5): one more launch on the same stream, from one glyph
// buffer into the other.  `kernels`: k_msdf_generate and k_msdf_correct; FDH_GLYPH_MTSDF_OVERLAP (step 6), the same records and the same
// launches by the kernels that combine the contours; or those of k_msdf_cubic.hip on its longer records.
void GlyphMaker::put_field(const SegmentFormat& fmt, FieldKernels kernels, hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const float* segs, int n, float range, bool correct,
                           int out_rect[4]) {
  using Generate = void (*)(hipStream_t, const float*, int, int, int, float, float, uint32_t*);
  using Correct = void (*)(hipStream_t, const float*, int, int, int, float, float, const uint32_t*, uint32_t*);
  static const struct { Generate generate; Correct correct; } launchers[] = {  // by FieldKernels
      {launch_msdf_generate, launch_msdf_correct}, {launch_msdf_generate_union, launch_msdf_correct_union}, {launch_msdf_generate_cubic, launch_msdf_correct_cubic}};
  const bool device = atlas.has_device();
  std::vector<float> rec;
  int n_edges = 0;
  float orient = 1.0f;
  if (!fmt.records(segs, n, device ? &rec : nullptr, &n_edges, &orient)) throw Refusal{fmt.single}("a distance field needs closed contours");
  if (device) {
    const size_t npx = (size_t)w * h;
    glyph_a_.reserve(npx);
    glyph_b_.reserve(npx);
    glyph_edges_.reserve(std::max<size_t>(rec.size(), fmt.stride));
  }
  atlas.make_room(s, w, h);
  const AtlasEntry& e = atlas.place(s, key, w, h, out_rect, Stored::chain_or_level0);
  if (!device) return;
  const int x = e.x, y = e.y;
  if (!rec.empty()) FDH_HIP(hipMemcpyAsync(glyph_edges_.ptr, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice, s));
  uint32_t *field = glyph_a_.ptr, *spare = glyph_b_.ptr;
  launchers[(int)kernels].generate(s, glyph_edges_.ptr, n_edges, w, h, orient, range, field);
  if (correct) {
    launchers[(int)kernels].correct(s, glyph_edges_.ptr, n_edges, w, h, orient, range, field, spare);
    std::swap(field, spare);
  }
  // The level chain (updateSubImage's, textures.nim:106-119) stores nothing of an image 1 texel wide or high, not even level 0.  A field is
  // sampled at level 0 alone, and these texels have no other home: such a field gets that level.
  if (w == 1 || h == 1) launch_atlas_blit(s, atlas.level(0), atlas.size(), x, y, field, w, h);
  glyph_to_atlas(s, atlas, field, spare, w, h, x, y, 0u);  // (synchronises: `rec` stays alive until then)
}

// ---- distance fields from coverage images (the specification: include_glyphs/figdraw_hip_image_sdf.h).  What both calls ask of their arguments
// beside the source; -> the range
static int image_sdf_range(const Refusal& bad, int channel, int pad, uint32_t flags) {
  if (channel < 0 || channel > 3) throw bad("channel must be in 0..3");
  if (pad < 0 || pad > 64) throw bad("pad must be in 0..64");
  if (flags & ~0xFF00u) throw bad("unknown flag (FDH_GLYPH_SDF_RANGE only)");
  const uint32_t range = (flags >> 8) & 255u;
  if (range > 64u) throw bad("a distance range is at most 64");
  return range ? (int)range : 4;
}
void GlyphMaker::put_image_sdf(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const uint8_t* rgba, int channel, int pad, uint32_t flags, int out_rect[4]) {
  const Refusal bad{"put_image_sdf"};
  if (w <= 0 || h <= 0 || !rgba) throw bad("empty image");
  const int range = image_sdf_range(bad, channel, pad, flags);
  put_image_field(s, atlas, key, w, h, rgba, 0, 0, channel, pad, range, out_rect);
}
void GlyphMaker::put_image_sdf_of(hipStream_t s, Atlas& atlas, int64_t src_key, int64_t key, int channel, int pad, uint32_t flags, int out_rect[4]) {
  const Refusal bad{"put_image_sdf_of"};
  const int range = image_sdf_range(bad, channel, pad, flags);
  const AtlasEntry* src = atlas.find(src_key);
  if (!src) throw bad("unknown source key");
  if (src_key == key) throw bad("the source and the field need two keys");
  put_image_field(s, atlas, key, src->w, src->h, nullptr, src->x, src->y, channel, pad, range, out_rect);  // (by value: the placement may drop `src`)
}
// The source goes to scratch -- from the host behind the placement, as every put copies; from the atlas AHEAD of it: a placement that grows
// the atlas frees the levels the source is in (Atlas::alloc waits for the stream first) --, one launch makes the field, then the level
// chain every glyph image takes, with the distance field's rule for an image 1 texel wide or high (put_field).
void GlyphMaker::put_image_field(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const uint8_t* rgba, int from_x, int from_y, int channel, int pad, int range, int out_rect[4]) {
  constexpr int64_t kNoAtlasTakes = 1 << 24;  // (a size beyond it fares as this one does, and the sums below stay ints)
  const int ow = (int)std::min<int64_t>((int64_t)w + 2 * pad, kNoAtlasTakes), oh = (int)std::min<int64_t>((int64_t)h + 2 * pad, kNoAtlasTakes);
  const bool device = atlas.has_device();
  if (device) {
    const size_t n = (size_t)ow * oh;
    glyph_a_.reserve(n);
    glyph_b_.reserve(n);
    glyph_src_.reserve((size_t)w * h);
    if (!rgba) {
      const size_t S = (size_t)atlas.size();
      FDH_HIP(hipMemcpy2DAsync(glyph_src_.ptr, (size_t)w * 4, atlas.level(0) + (size_t)from_y * S + from_x, S * 4, (size_t)w * 4, (size_t)h, hipMemcpyDeviceToDevice, s));
    }
  }
  atlas.make_room(s, ow, oh);  // (behind the copy: in keep mode the source may move)
  const AtlasEntry& e = atlas.place(s, key, ow, oh, out_rect, Stored::chain_or_level0);
  if (!device) return;
  const int x = e.x, y = e.y;
  if (rgba) FDH_HIP(hipMemcpyAsync(glyph_src_.ptr, rgba, (size_t)w * h * 4, hipMemcpyHostToDevice, s));
  launch_image_sdf_generate(s, glyph_src_.ptr, w, h, w, channel, pad, range, glyph_a_.ptr);
  if (ow == 1 || oh == 1) launch_atlas_blit(s, atlas.level(0), atlas.size(), x, y, glyph_a_.ptr, ow, oh);
  glyph_to_atlas(s, atlas, glyph_a_.ptr, glyph_b_.ptr, ow, oh, x, y, 0u);  // (synchronises: `rgba` is free after)
}

// ---- fdh_compact_atlas (the specification: include_glyphs/figdraw_hip_atlas.h): the texels of every live entry from the old levels into the new
// ones.  Level 0 of every entry that has a level chain goes into the field buffer (k_atlas_move, one launch), glyph after glyph as a batch
// lays its images out, and the batches' own level chain makes every level of them from there -- level 0 included, with the batches' owner
// bits in compaction order.  An entry with levels of its own (Stored::levels) follows in a second launch of k_atlas_move: its level 0 from
// the old atlas, its other levels from the host's copy, with owner bits against every later rectangle of the new atlas.
static_assert(move::kLevels == kMaxMips, "move::Views holds every level of an atlas");
void GlyphMaker::move_entries(hipStream_t s, const AtlasView& from, const Atlas& to, const std::vector<MovedEntry>& moved, FdhAtlasMoveStats& st) {
  const auto t_tables = std::chrono::steady_clock::now();
  std::vector<msdf::BatchGlyph> tab;
  std::vector<const MovedEntry*> chained;
  std::vector<move::Rect> own_levels;  // the second launch: every rectangle below level 0 in compaction order, those of Stored::levels entries copied
  std::vector<uint32_t> payload;       // ... whose kept levels, one entry after the other
  bool any_own = false;
  for (const MovedEntry& m : moved) {
    const AtlasEntry& e = *m.e;
    each_stored(e, to.size(), to.n_levels(), [&](int, int, int, int w, int h) { st.rects_moved++; st.texels += (int64_t)w * h; });
    if (e.stored != Stored::levels) {
      if ((e.w == 1 || e.h == 1) && e.stored != Stored::chain_or_level0) continue;  // nothing of it is stored
      msdf::BatchGlyph t{};
      t.w = e.w; t.h = e.h; t.x = e.x; t.y = e.y;
      tab.push_back(t);
      chained.push_back(&m);
      each_stored(e, to.size(), to.n_levels(), [&](int l, int x, int y, int w, int h) {
        if (l > 0) own_levels.push_back(move::Rect{0, 0, 0, l, x, y, w, h, false});
      });
      continue;
    }
    any_own = true;
    const size_t base = payload.size();
    payload.insert(payload.end(), e.kept->texels.begin(), e.kept->texels.end());
    each_stored(e, to.size(), to.n_levels(), [&](int l, int x, int y, int w, int h) {
      if (l == 0) { own_levels.push_back(move::Rect{0, m.old_x, m.old_y, 0, x, y, w, h, true}); return; }
      size_t off = base;
      for (int k = 1; k < l; k++) off += (size_t)e.kept->w[k] * e.kept->h[k];
      own_levels.push_back(move::Rect{move::kBuffer, (int)off, 0, l, x, y, w, h, true});
    });
  }
  // ---- the tables
  const int m = (int)tab.size();
  BatchTables T;
  move::Tables G, O;
  size_t field_texels = 0;
  if (m) {
    batch_tables(tab, 0, m, true, to.n_levels(), &T);
    std::vector<move::Rect> gather;
    gather.reserve((size_t)m);
    for (int k = 0; k < m; k++) {
      const AtlasEntry& e = *chained[(size_t)k]->e;
      gather.push_back(move::Rect{0, chained[(size_t)k]->old_x, chained[(size_t)k]->old_y, move::kBuffer, (int)tab[(size_t)k].field_off, 0, e.w, e.h, true});
      field_texels += (size_t)e.w * e.h;
    }
    move::build_tables(gather, &G);
  }
  if (any_own) move::build_tables(own_levels, &O);
  const auto t_move = std::chrono::steady_clock::now();
  st.us_tables = (int32_t)std::chrono::duration_cast<std::chrono::microseconds>(t_move - t_tables).count();
  // ---- the device: buffers first, then the copies and the launches on the stream.  The kept levels lie behind the tables in move_tab_:
  // glyph_src_ is not touched -- in keep mode fdh_put_image_sdf_of has parked its source there when the compaction runs (put_image_field)
  // -- and what the other buffers held is not needed any more by any put that has come as far as its placement.
  glyph_a_.reserve(std::max<size_t>(field_texels, 1));
  glyph_b_.reserve(std::max<size_t>(field_texels, 1));
  glyph_tab_.reserve(std::max<size_t>(T.words.size(), 1));
  move_tab_.reserve(G.words.size() + O.words.size() + payload.size() + 1);
  uint32_t* const d_payload = move_tab_.ptr + G.words.size() + O.words.size();
  move::Views V{};
  for (int l = 0; l < move::kLevels; l++) { V.from[l] = from.level[l]; V.to[l] = to.level(l); }
  V.from_size = from.size; V.from_levels = from.n_levels; V.to_size = to.size(); V.to_levels = to.n_levels();
  V.buf_in = d_payload; V.buf_out = glyph_a_.ptr;
  auto launch = [&](const move::Tables& M, uint32_t* at) {
    FDH_HIP(hipMemcpyAsync(at, M.words.data(), M.words.size() * 4, hipMemcpyHostToDevice, s));
    const uint32_t* tiles = at + (size_t)M.n_records * move::kRecordWords;
    launch_atlas_move(s, V, reinterpret_cast<const move::Record*>(at), tiles, (int)M.n_tiles, tiles + M.n_tiles);
    st.tiles += (int32_t)M.n_tiles;
    st.launches++;
  };
  if (m) {
    launch(G, move_tab_.ptr);
    FDH_HIP(hipMemcpyAsync(glyph_tab_.ptr, T.words.data(), T.words.size() * 4, hipMemcpyHostToDevice, s));
    st.launches += batch_level_chain(s, to, m, T, glyph_a_.ptr, glyph_b_.ptr);
  }
  if (any_own) {
    if (!payload.empty()) FDH_HIP(hipMemcpyAsync(d_payload, payload.data(), payload.size() * 4, hipMemcpyHostToDevice, s));
    launch(O, move_tab_.ptr + G.words.size());
  }
  FDH_HIP(hipStreamSynchronize(s));  // (the tables and the payload stay alive until here)
  FDH_HIP(hipGetLastError());
  st.us_move = (int32_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_move).count();
}

// ---- the batches.  What n single puts do, in three passes: every glyph is validated; every glyph is placed, in order, through Atlas::place; then
// the glyphs that are still in the atlas -- those placed since the last growth -- get their texels from a number of launches that does not
// depend on n.  Single puts overwrite one another where two rectangles meet in a deep level (msdf::kOwnerLevel); one launch has no order, so
// the host paints the rectangles of such a level in put order and gives every glyph the bits of the texels that are still its own
// (batch_tables, fdh_glyph_tables.h).
// Pass 1, what every batch asks of its array and of each glyph in it; check(g): the call's own questions, after these.  -> the sum of w * h
template <typename Check>
static int64_t validate_batch(const Refusal& bad, const FdhGlyphOutline* glyphs, int n, Check check) {
  if (n < 0 || (n > 0 && !glyphs)) throw bad("bad glyph array");
  if (n > 65535) throw bad("at most 65535 glyphs");
  int64_t texels = 0;
  for (int i = 0; i < n; i++) {
    const FdhGlyphOutline& g = glyphs[i];
    if (g.width <= 0 || g.height <= 0 || g.width > 4096 || g.height > 4096) throw bad("image size must be in 1..4096");
    if (g.n_segs < 0 || (g.n_segs > 0 && !g.segs)) throw bad("bad outline");
    check(g);
    texels += (int64_t)g.width * g.height;
  }
  if (texels > ((int64_t)1 << 24)) throw bad("at most 2^24 texels in a batch");
  return texels;
}
// The level chain of a batch whose tables (T, of m glyphs) are in glyph_tab_ and whose images are in `field`: one blit and one minify per
// level, whatever the glyphs' sizes -- the number of launches, which is returned, is the atlas's alone.
int GlyphMaker::batch_level_chain(hipStream_t s, const Atlas& atlas, int m, const BatchTables& T, uint32_t* field, uint32_t* spare) {
  const msdf::BatchGlyph* d_glyphs = reinterpret_cast<const msdf::BatchGlyph*>(glyph_tab_.ptr);
  const uint32_t* d_tiles = glyph_tab_.ptr + (size_t)m * kBatchGlyphWords;
  const uint32_t* d_owner = d_tiles + T.n_tiles;
  int launches = 0;
  for (int l = 0; l < atlas.n_levels(); l++) {
    launch_atlas_blit_batch(s, atlas.level(l), atlas.size() >> l, l, d_glyphs, d_tiles, (int)T.n_tiles, d_owner, field);
    launches++;
    if (l + 1 == atlas.n_levels()) break;  // (a single put minifies once more, into a buffer nobody reads)
    launch_minify2_batch(s, l, d_glyphs, d_tiles, (int)T.n_tiles, field, spare);
    std::swap(field, spare);
    launches++;
  }
  return launches;
}
// what a batch copies to the device beside its tables: the edge records or the lines of all glyphs, glyph after glyph; BatchGlyph::edge_off
// counts in units of `unit` floats
struct GlyphMaker::Payload {
  const std::vector<float>& floats;
  size_t unit;     // (dst is reserved for one unit at the least)
  DeviceBuf<float>& dst;
  bool to_end;     // the copy ends with the array, not with the last placed glyph's part (the records of a batch that ran out of atlas, as ever)
};
// Passes 2 and 3 of every batch, whose pass 1 (the caller's) left `tab` (edge_off, n_edges, w, h and what the kernels want beside) and the
// payload; `texels`: the sum of w * h.  middle(payload on the device, glyph records, tile words, n_tiles, field, spare): the launches that
// make the images in `field` (it may swap the two), -> their number; the level chain follows.  Nothing here refuses a glyph.
template <typename Middle>
void GlyphMaker::place_and_make(hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, int (*out_rects)[4], std::vector<msdf::BatchGlyph>& tab, const Payload& payload,
                                int64_t texels, bool thin_tiles, FdhGlyphBatchStats& stats, Middle middle) {
  const bool device = atlas.has_device();
  stats = FdhGlyphBatchStats{};
  stats.glyphs = n;
  if (n == 0) return;
  // ---- the device buffers, for the whole batch (pass 3 takes a part of it), before any placement as every put does
  if (device) {
    glyph_a_.reserve((size_t)texels);
    glyph_b_.reserve((size_t)texels);
    payload.dst.reserve(std::max<size_t>(payload.floats.size(), payload.unit));
    glyph_tab_.reserve(batch_table_words(tab, thin_tiles, kMaxMips));  // (whatever atlas the batch ends in)
  }
  // ---- pass 2: the places
  // (keep mode: room for all glyphs of the batch at once, before any of them has a place -- only entries that have their texels move)
  if (atlas.keep()) {
    std::vector<int> wh((size_t)n * 2);
    for (int i = 0; i < n; i++) { wh[(size_t)i * 2] = glyphs[i].width; wh[(size_t)i * 2 + 1] = glyphs[i].height; }
    atlas.make_room(s, reinterpret_cast<const int (*)[2]>(wh.data()), n);
  }
  int first = 0, placed = 0;
  std::exception_ptr failed = place_batch(s, atlas, n, out_rects, thin_tiles ? Stored::chain_or_level0 : Stored::chain,
                                          [&](int i, int64_t* key, int* w, int* h) { *key = glyphs[i].key; *w = glyphs[i].width; *h = glyphs[i].height; },
                                          [&](int i, AtlasEntry& e) { tab[(size_t)i].x = e.x; tab[(size_t)i].y = e.y; }, &first, &placed);
  stats.written = placed - first;
  stats.dropped_by_growth = first;
  // ---- pass 3: the texels of glyphs first .. placed - 1
  if (device && placed > first) {
    const int m = placed - first;
    const size_t base = (size_t)tab[(size_t)first].edge_off * payload.unit;
    BatchTables T;
    batch_tables(tab, first, m, thin_tiles, atlas.n_levels(), &T);
    const size_t floats = payload.to_end ? payload.floats.size() - base : (size_t)T.n_edges * payload.unit;
    if (floats) FDH_HIP(hipMemcpyAsync(payload.dst.ptr, payload.floats.data() + base, floats * sizeof(float), hipMemcpyHostToDevice, s));
    FDH_HIP(hipMemcpyAsync(glyph_tab_.ptr, T.words.data(), T.words.size() * 4, hipMemcpyHostToDevice, s));
    const msdf::BatchGlyph* d_glyphs = reinterpret_cast<const msdf::BatchGlyph*>(glyph_tab_.ptr);
    const uint32_t* d_tiles = glyph_tab_.ptr + (size_t)m * kBatchGlyphWords;
    uint32_t *field = glyph_a_.ptr, *spare = glyph_b_.ptr;
    int launches = 0;
    if (T.n_tiles) {  // (none: coverage glyphs 1 texel wide or high alone)
      launches += middle(payload.dst.ptr, d_glyphs, d_tiles, (int)T.n_tiles, field, spare);
      launches += batch_level_chain(s, atlas, m, T, field, spare);
    }
    FDH_HIP(hipStreamSynchronize(s));  // (the payload and `T` stay alive until here)
    FDH_HIP(hipGetLastError());
    stats.tiles = (int32_t)T.n_tiles;
    stats.edges = (int32_t)T.n_edges;
    stats.launches = launches;
    stats.bytes_copied = (int64_t)(floats * sizeof(float) + T.words.size() * 4);
  }
  if (failed) std::rethrow_exception(failed);
}
void GlyphMaker::put_glyph_outlines(hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  put_fields(SegmentFormat::six(), s, atlas, glyphs, n, flags, out_rects);
}
void GlyphMaker::put_glyph_outlines_cubic(hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  put_fields(SegmentFormat::eight(), s, atlas, glyphs, n, flags, out_rects);
}
// fdh_put_glyph_outlines and fdh_put_glyph_outlines_cubic (the specifications: include_glyphs/figdraw_hip_glyphs.h and figdraw_hip_cubic_batch.h): what n
// distance-field calls of put_outline do.  Pass 3: the generator over the tiles of all glyphs, the correction, and per atlas level one blit
// and one minify.  Eight floats without a cubic in any glyph IS the six-float batch, on copies of the segments.  With one, every glyph --
// those without a cubic too -- goes the cubic call's way: mc::build_shape, records of mc::kCubicEdgeFloats floats, and the batched kernels of
// k_msdf_cubic.hip, in which a line or a quadratic runs k_msdf.hip's expressions: such a glyph gets the bytes its single call gives it.
void GlyphMaker::put_fields(const SegmentFormat& fmt, hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  // ---- pass 1: validation.  Nothing below this pass refuses a glyph.
  const Refusal bad{fmt.fields};
  if (flags & ~kFieldFlags) throw bad(fmt.fields_flags);
  if (!(flags & FDH_GLYPH_MTSDF)) throw bad("needs FDH_GLYPH_MTSDF");
  const uint32_t flag_range = (flags >> 8) & 255u;
  if (flag_range > 64u) throw bad("a distance range is at most 64");
  const bool correct = (flags & FDH_GLYPH_MTSDF_CORRECT) != 0, overlap = (flags & FDH_GLYPH_MTSDF_OVERLAP) != 0;
  int64_t segments = 0;
  bool any_cubic = false;
  const int64_t texels = validate_batch(bad, glyphs, n, [&](const FdhGlyphOutline& g) {
    if (g.n_segs > msdf::kMaxSegments) throw bad("a distance field takes at most 65535 segments");
    if (g.sdf_range > 64u) throw bad("a distance range is at most 64");
    segments += g.n_segs;
    any_cubic = any_cubic || (fmt.holds_cubic && fmt.holds_cubic(g.segs, g.n_segs));
  });
  if (segments > ((int64_t)1 << 20)) throw bad("at most 2^20 segments in a batch");
  if (fmt.holds_cubic && !any_cubic) {  // the six-float batch, on copies
    std::vector<std::vector<float>> six((size_t)n);
    std::vector<FdhGlyphOutline> plain(glyphs, glyphs + n);
    for (int i = 0; i < n; i++) {
      mc::to_quadratic_format(glyphs[i].segs, glyphs[i].n_segs, &six[(size_t)i]);
      plain[(size_t)i].segs = six[(size_t)i].data();
    }
    put_fields(SegmentFormat::six(), s, atlas, plain.data(), n, flags, out_rects);
    return;
  }
  if (fmt.holds_cubic && overlap) throw bad("FDH_GLYPH_MTSDF_OVERLAP takes no cubic segment");
  const bool device = atlas.has_device();
  std::vector<float> rec;                        // the records of all glyphs, glyph after glyph (a device context only)
  std::vector<msdf::BatchGlyph> tab((size_t)n);  // edge_off (in records), n_edges, w, h, orient and the range now; the offsets and the place in pass 3
  for (int i = 0; i < n; i++) {
    const FdhGlyphOutline& g = glyphs[i];
    msdf::BatchGlyph& t = tab[(size_t)i];
    t = msdf::BatchGlyph{};
    t.edge_off = (uint32_t)(rec.size() / fmt.stride);
    if (!fmt.records(g.segs, g.n_segs, device ? &rec : nullptr, &t.n_edges, &t.orient)) throw bad("a distance field needs closed contours");
    const float range = g.sdf_range ? (float)g.sdf_range : (flag_range ? (float)flag_range : 4.0f);
    t.w = g.width; t.h = g.height;
    t.inv_range = 1.0f / range; t.step = range / 255.0f;
  }
  const bool cubic = fmt.holds_cubic != nullptr;
  place_and_make(s, atlas, glyphs, n, out_rects, tab, Payload{rec, fmt.stride, glyph_edges_, true}, texels, true, batch_stats_,
                 [&](const float* edges, const msdf::BatchGlyph* d_glyphs, const uint32_t* d_tiles, int n_tiles, uint32_t*& field, uint32_t*& spare) {
                   if (cubic) launch_msdf_generate_cubic_batch(s, edges, d_glyphs, d_tiles, n_tiles, field);
                   else launch_msdf_generate_batch(s, overlap, edges, d_glyphs, d_tiles, n_tiles, field);
                   if (!correct) return 1;
                   if (cubic) launch_msdf_correct_cubic_batch(s, edges, d_glyphs, d_tiles, n_tiles, field, spare);
                   else launch_msdf_correct_batch(s, overlap, edges, d_glyphs, d_tiles, n_tiles, field, spare);
                   std::swap(field, spare);
                   return 2;
                 });
}
void GlyphMaker::put_glyph_coverage_batch(hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  put_coverage(SegmentFormat::six(), s, atlas, glyphs, n, flags, out_rects);
}
void GlyphMaker::put_glyph_coverage_batch_cubic(hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  put_coverage(SegmentFormat::eight(), s, atlas, glyphs, n, flags, out_rects);
}
// The coverage batch in either format (the specifications: include_glyphs/figdraw_hip_coverage.h and figdraw_hip_cubic_batch.h): what n coverage calls
// of put_outline do.  Pass 1 flattens every outline into one array of lines; pass 3: two launches make the coverage of all glyphs
// (k_coverage_cells_batch, k_coverage_sum_batch), one filters it (k_lcd_filter_batch), and every atlas level takes one blit and one minify.
// A glyph 1 texel wide or high is placed and has no tiles: a single put stores nothing of it.
void GlyphMaker::put_coverage(const SegmentFormat& fmt, hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  // ---- pass 1: validation.  Nothing below this pass refuses a glyph.  (FDH_GLYPH_LCD_CONTEXT is resolved by the context.)
  const Refusal bad{fmt.coverage};
  if (flags & ~kLcdFlags) throw bad(std::string("the LCD flags only (distance fields are ") + fmt.fields_call + ")");
  std::vector<msdf::BatchGlyph> tab;  // edge_off, n_edges: the glyph's first line and its line count; orient, inv_range, step: unused
  int64_t segments = 0, n_lines = 0;
  const int64_t texels = validate_batch(bad, glyphs, n, [&](const FdhGlyphOutline& g) {
    if (g.sdf_range) throw bad("a coverage glyph has no distance range");
    segments += g.n_segs;
    if (segments > ((int64_t)1 << 20)) throw bad("at most 2^20 segments in a batch");
    msdf::BatchGlyph t{};
    t.w = g.width; t.h = g.height;
    t.edge_off = (uint32_t)n_lines;
    for (int k = 0; k < g.n_segs; k++) t.n_edges += fmt.lines_of(g.segs + (size_t)fmt.floats * k);
    n_lines += t.n_edges;
    tab.push_back(t);
  });
  if (n_lines > ((int64_t)1 << 22)) throw bad("at most 2^22 flattened lines in a batch");
  std::vector<float> lines;  // of all glyphs, glyph after glyph (a device context only)
  if (atlas.has_device()) {
    lines.reserve((size_t)n_lines * 4);
    for (int i = 0; i < n; i++) fmt.flatten(glyphs[i].segs, glyphs[i].n_segs, &lines);
  }
  place_and_make(s, atlas, glyphs, n, out_rects, tab, Payload{lines, 4, glyph_lines_, false}, texels, false, coverage_stats_,
                 [&](const float* d_lines, const msdf::BatchGlyph* d_glyphs, const uint32_t* d_tiles, int n_tiles, uint32_t*& field, uint32_t*& spare) {
                   launch_coverage_batch(s, reinterpret_cast<const float4*>(d_lines), d_glyphs, d_tiles, n_tiles, reinterpret_cast<float*>(spare), field);
                   if (!(flags & FDH_GLYPH_LCD_FILTER)) return 2;
                   launch_lcd_filter_batch(s, d_glyphs, d_tiles, n_tiles, field, spare);
                   std::swap(field, spare);
                   return 3;
                 });
}

}  // namespace fdh
