// fdh_glyphs.cpp -- class GlyphMaker (fdh_glyphs.h): glyph images, outlines and batches of outlines on their way into the atlas, every step a
// kernel on the context's stream.  One body per kind of work: a single put, a batch's pass 1 per kind of glyph, passes 2 and 3 of every
// batch; what the two segment formats differ in is a SegmentFormat.
#include "fdh_glyphs.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <string>
#include <unordered_set>

#include "fdh_kernels.h"
#include "fdh_atlas_move.h"
#include "fdh_image_batch.h"  // and through it fdh_image_import.h
#include "fdh_video_batch.h"  // and through it fdh_video_import.h
#include "fdh_video_planar.h"
#include "fdh_video_422.h"
#include "fdh_video_alpha.h"
#include "fdh_msdf_cubic_host.h"

namespace fdh {
namespace mc = msdf::cubic;
namespace ii = image_import;
namespace ib = image_batch;
namespace vi = video_import;
namespace vb = video_batch;
namespace vp = video_planar;
namespace v2 = video_422;
namespace va = video_alpha;

void GlyphMaker::release() {
  glyph_a_.release(); glyph_b_.release(); glyph_lines_.release(); glyph_acc_.release(); glyph_edges_.release(); glyph_tab_.release(); glyph_src_.release(); move_tab_.release(); ink_host_.release();
}
namespace {
// a refusal under the name of the call that makes it
struct Refusal {
  const char* who;
  Error operator()(const std::string& what) const { return Error(FDH_ERR_INVALID, std::string(who) + ": " + what); }
};
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

// ---- images from device memory (the specification: include_glyphs/figdraw_hip_device_image.h).  What both calls ask of the struct; -> whether the
// source's rows are 16-byte aligned (a lane's run of four texels is then one load per plane)
static_assert(ii::kLevels == kMaxMips, "image_import::Params holds every level of an atlas");
static bool validate_device_image(const Refusal& bad, const FdhDeviceImage* img) {
  if (!img || !img->data) throw bad("null image");
  if (img->width <= 0 || img->height <= 0) throw bad("empty image");
  if (img->format > FDH_IMAGE_PLANAR_F16) throw bad("unknown format");
  if (img->flags & ~(uint32_t)FDH_IMAGE_STRAIGHT_ALPHA) throw bad("unknown flag");
  if (img->reserved) throw bad("reserved must be 0");
  const bool planar = img->format != FDH_IMAGE_RGBA8;
  if (planar ? !(img->channels == 1 || img->channels == 3 || img->channels == 4) : img->channels != 4)
    throw bad("channels must be 4 for RGBA8 and 1, 3 or 4 for a planar format");
  const int64_t element = img->format == FDH_IMAGE_PLANAR_F16 ? 2 : 4;  // (an RGBA8 texel is one aligned word)
  const bool planes = planar && img->channels > 1;
  if ((uintptr_t)img->data % (uintptr_t)element || img->pitch_bytes % element) throw bad("data and pitch_bytes must be multiples of the element size");
  if (img->pitch_bytes < (int64_t)img->width * element) throw bad("pitch_bytes is below a row's bytes");
  if (planes && (__int128)img->plane_bytes < (__int128)img->pitch_bytes * img->height) throw bad("plane_bytes is below pitch_bytes * height");
  if (planes && img->plane_bytes % element) throw bad("plane_bytes must be a multiple of the element size");
  return (uintptr_t)img->data % 16 == 0 && img->pitch_bytes % 16 == 0 && (!planes || img->plane_bytes % 16 == 0);
}
// On a context with a device: the source as the device addresses it -- device memory of `device`, or page-locked host memory.  Anything
// else (pageable memory, another device's, an address nobody has mapped) is refused, and the runtime's sticky error cleared behind it.
static const void* device_address(const Refusal& bad, int device, const void* data) {
  if (const void* view = device_view_of(device, data)) return view;  // (fdh_memory.h)
  throw bad("the source is neither device memory of the context's device nor page-locked host memory");
}
// the scratch of an import, ahead of the placement as every put reserves: the level-5 image and what k_minify2 makes of it
static void reserve_import(DeviceBuf<uint32_t>& a, DeviceBuf<uint32_t>& b, PinnedBuf<int32_t>& ink_host, int w, int h) {
  if (w > 16384 || h > 16384) return;  // (no atlas takes it: the placement says so)
  const size_t w5 = (size_t)(w + 31) / 32, h5 = (size_t)(h + 31) / 32;
  a.reserve(w5 * h5);
  b.reserve(((w5 + 1) / 2) * ((h5 + 1) / 2));
  ink_host.reserve_exact(ii::kInkTiles * ii::kInkWords);
}
void GlyphMaker::put_device_image(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhDeviceImage* img, int out_rect[4]) {
  const Refusal bad{"put_image_device"};
  const bool wide = validate_device_image(bad, img);
  const FdhDeviceImage src = *img;
  const void* data = nullptr;
  if (atlas.has_device()) {
    data = device_address(bad, device, src.data);
    reserve_import(glyph_a_, glyph_b_, ink_host_, src.width, src.height);
  }
  atlas.make_room(s, src.width, src.height);
  AtlasEntry& e = atlas.place(s, key, src.width, src.height, out_rect);
  if (atlas.has_device()) import_image(s, atlas, e, src, data, wide);
}
void GlyphMaker::update_device_image(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhDeviceImage* img) {
  const Refusal bad{"update_image_device"};
  const bool wide = validate_device_image(bad, img);
  const FdhDeviceImage src = *img;
  const AtlasEntry* old = atlas.find(key);  // (ahead of the pointer's check and the buffers; begin_update says the same again)
  if (!old) throw bad("unknown key");
  if (old->w != src.width || old->h != src.height) throw bad("size mismatch");
  const void* data = nullptr;
  if (atlas.has_device()) {
    data = device_address(bad, device, src.data);
    reserve_import(glyph_a_, glyph_b_, ink_host_, src.width, src.height);
  }
  AtlasEntry& e = atlas.begin_update(bad.who, key, src.width, src.height);
  e.has_ink = false;  // (the old texels' boxes; import_image measures the new ones)
  if (atlas.has_device()) import_image(s, atlas, e, src, data, wide);
}
// Two launches for an image up to 2048 x 2048: k_image_import makes levels 0 .. 5, k_image_import_tail the rest from the level-5 image.
// A larger level-5 image first takes k_minify2 / k_atlas_blit steps, as glyph_to_atlas does, until the tail's workgroup can hold it.
// Waits for the stream once; the tiles' ink blocks are in page-locked memory by then (the kernel stores them there): finish_import, which
// import_video shares.  `data`: the source as the device addresses it; `wide`: its rows are 16-byte aligned.
void GlyphMaker::import_image(hipStream_t s, const Atlas& atlas, AtlasEntry& e, const FdhDeviceImage& img, const void* data, bool wide) {
  ii::Params P{};
  P.data = data; P.pitch_bytes = img.pitch_bytes; P.plane_bytes = img.plane_bytes;
  P.w = img.width; P.h = img.height;
  P.format = img.format; P.channels = img.channels; P.flags = img.flags;
  P.wide = wide && e.w >= 4 ? 1 : 0;
  P.x = e.x; P.y = e.y;
  atlas.each_level(e.x, e.y, e.w, e.h, [&](int, int, int, int, int) { P.n_store++; });
  P.ink = e.w <= ii::kInkMax && e.h <= ii::kInkMax;
  for (int l = 0; l < ii::kTileLevels; l++) { P.lw[l] = (e.w + (1 << l) - 1) >> l; P.lh[l] = (e.h + (1 << l) - 1) >> l; }
  for (int l = 0; l < atlas.n_levels(); l++) P.level[l] = atlas.level(l);
  P.size = atlas.size();
  P.scratch = glyph_a_.ptr;
  P.ink_block = ink_host_.dev;
  launch_image_import(s, P);
  finish_import(s, atlas, e, P.n_store, P.ink != 0);
}
// an entry's sixteen ink boxes from the folded blocks (fold_ink)
static void set_ink(AtlasEntry& e, const int32_t got[ii::kInkWords]) {
  for (int k = 0; k < kInkLevels; k++) {  // (a box no texel grew: empty, at the origin)
    const int32_t *a = got + 4 * k, *c = got + 32 + 4 * k;
    e.ink_a[k] = a[2] ? InkBox{(int16_t)a[0], (int16_t)a[1], (int16_t)a[2], (int16_t)a[3]} : InkBox{0, 0, 0, 0};
    e.ink_rgb[k] = c[2] ? InkBox{(int16_t)c[0], (int16_t)c[1], (int16_t)c[2], (int16_t)c[3]} : InkBox{0, 0, 0, 0};
  }
  e.has_ink = true;
}
void GlyphMaker::finish_import(hipStream_t s, const Atlas& atlas, AtlasEntry& e, int n_store, bool ink) {
  uint32_t *cur = glyph_a_.ptr, *nxt = glyph_b_.ptr;
  int l = ii::kTileLevels - 1, cw = (e.w + (1 << l) - 1) >> l, ch = (e.h + (1 << l) - 1) >> l;
  const int tiles = cw * ch;
  for (; (cw > ii::kTailMax || ch > ii::kTailMax) && l + 1 < n_store; std::swap(cur, nxt)) {
    launch_minify2(s, cur, nxt, cw, ch);
    l++; cw = (cw + 1) / 2; ch = (ch + 1) / 2;
    launch_atlas_blit(s, atlas.level(l), atlas.size() >> l, e.x >> l, e.y >> l, nxt, cw, ch);
  }
  if (l + 1 < n_store) {
    ii::TailParams T{};
    T.src = cur; T.sw = cw; T.sh = ch; T.l0 = l; T.n_store = n_store;
    T.x = e.x; T.y = e.y; T.size = atlas.size();
    for (int k = 0; k < atlas.n_levels(); k++) T.level[k] = atlas.level(k);
    launch_image_import_tail(s, T);
  }
  FDH_HIP(hipStreamSynchronize(s));
  FDH_HIP(hipGetLastError());
  e.has_ink = ink;
  if (!ink) return;
  int32_t got[ii::kInkWords];
  ii::fold_ink(ink_host_.ptr, tiles, got);
  set_ink(e, got);
}

// ---- batches of device images (the specification: include_glyphs/figdraw_hip_device_images.h).  What n single calls do, in the glyph batches'
// three passes: every image is validated; every image is placed (an update: begun), in order; then the images that are still in the atlas
// get their texels from one launch per format present and one for the tails, over the tables of fdh_image_batch.h.
template <typename Item, typename PlacedAt>  // (pass 2 of every batch; with the glyph batches below)
static std::exception_ptr place_batch(hipStream_t s, Atlas& atlas, int n, int (*out_rects)[4], Stored stored, Item item, PlacedAt placed_at, int* first, int* placed);
struct GlyphMaker::ImageBatch {
  std::vector<ii::BatchImage> tab;    // pass 1: the source as the device addresses it, extents, format, channels, flags, wide; pass 2: the place
  std::vector<AtlasEntry*> entries;   // pass 2: the entries (a placement never moves the ones behind the last growth)
  std::vector<const void*> sources;   // the callers' pointers: what a copy to the host starts from
};
// the source's bytes from `data` to its last element's end
static int64_t source_bytes(const FdhDeviceImage& g) {
  const int64_t element = g.format == FDH_IMAGE_PLANAR_F16 ? 2 : 4;
  const int64_t planes = g.format != FDH_IMAGE_RGBA8 && g.channels > 1 ? g.channels : 1;
  return (planes - 1) * g.plane_bytes + (int64_t)(g.height - 1) * g.pitch_bytes + (int64_t)g.width * element;
}
// Pass 1 of both batches.  Nothing behind it refuses an image.
void GlyphMaker::validate_device_images(const char* who, const Atlas& atlas, int device, const int64_t* keys, const FdhDeviceImage* images, int n, bool update, ImageBatch* B) {
  const Refusal bad{who};
  if (n < 0 || (n > 0 && (!keys || !images))) throw bad("bad image array");
  if (n > ib::kMaxImages) throw bad("at most 65535 images");
  B->tab.assign((size_t)n, ii::BatchImage{});
  B->entries.assign((size_t)n, nullptr);
  B->sources.assign((size_t)n, nullptr);
  std::unordered_set<int64_t> seen;
  int64_t tiles = 0;
  for (int i = 0; i < n; i++) {
    const FdhDeviceImage& g = images[i];
    const bool wide = validate_device_image(bad, &g);
    if (g.width > ii::kBatchMaxExtent || g.height > ii::kBatchMaxExtent) throw bad("an image of a batch is at most 2048 x 2048");
    if (!seen.insert(keys[i]).second) throw bad("a key occurs twice");
    if (update) {
      const AtlasEntry* old = atlas.find(keys[i]);
      if (!old) throw bad("unknown key");
      if (old->w != g.width || old->h != g.height) throw bad("size mismatch");
    }
    tiles += (int64_t)ib::covered_tiles(g.width, g.height);
    ii::BatchImage& t = B->tab[(size_t)i];
    t.data = g.data; t.pitch_bytes = g.pitch_bytes; t.plane_bytes = g.plane_bytes;
    t.w = g.width; t.h = g.height;
    t.format = g.format; t.channels = g.channels; t.flags = g.flags;
    t.wide = wide && g.width >= 4 ? 1 : 0;
    B->sources[(size_t)i] = g.data;
  }
  if (tiles > ib::kMaxTiles) throw bad("at most 2^18 tiles in a batch");
  if (!atlas.has_device()) return;
  for (int i = 0; i < n; i++) {
    ii::BatchImage& t = B->tab[(size_t)i];
    t.data = device_address(bad, device, images[i].data);
    const char *lo = static_cast<const char*>(t.data), *hi = lo + source_bytes(images[i]);
    for (int l = 0; l < atlas.n_levels(); l++) {
      const char* level = reinterpret_cast<const char*>(atlas.level(l));
      if (lo < level + ((size_t)(atlas.size() >> l) * (atlas.size() >> l)) * 4 && level < hi) throw bad("the source lies in the context's own atlas");
    }
  }
}
void GlyphMaker::put_device_images(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhDeviceImage* images, int n, int (*out_rects)[4]) {
  ImageBatch B;
  validate_device_images("put_images_device", atlas, device, keys, images, n, false, &B);
  image_stats_ = FdhImageBatchStats{};
  image_stats_.images = n;
  if (n == 0) return;
  if (atlas.has_device()) reserve_image_batch(B);
  // ---- pass 2: the places (keep mode: room for all images of the batch at once, before any of them has a place)
  if (atlas.keep()) {
    std::vector<int> wh((size_t)n * 2);
    for (int i = 0; i < n; i++) { wh[(size_t)i * 2] = images[i].width; wh[(size_t)i * 2 + 1] = images[i].height; }
    atlas.make_room(s, reinterpret_cast<const int (*)[2]>(wh.data()), n);
  }
  int first = 0, placed = 0;
  std::exception_ptr failed = place_batch(s, atlas, n, out_rects, Stored::chain,
                                          [&](int i, int64_t* key, int* w, int* h) { *key = keys[i]; *w = images[i].width; *h = images[i].height; },
                                          [&](int i, AtlasEntry& e) { B.tab[(size_t)i].x = e.x; B.tab[(size_t)i].y = e.y; B.entries[(size_t)i] = &e; }, &first, &placed);
  image_stats_.written = placed - first;
  image_stats_.dropped_by_growth = first;
  // ---- pass 3: the texels of images first .. placed - 1
  if (placed > first) make_device_images(s, atlas, B, first, placed - first);
  if (failed) std::rethrow_exception(failed);
}
void GlyphMaker::update_device_images(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhDeviceImage* images, int n) {
  ImageBatch B;
  validate_device_images("update_images_device", atlas, device, keys, images, n, true, &B);
  image_stats_ = FdhImageBatchStats{};
  image_stats_.images = n;
  if (n == 0) return;
  if (atlas.has_device()) reserve_image_batch(B);
  for (int i = 0; i < n; i++) {
    AtlasEntry& e = atlas.begin_update("update_images_device", keys[i], images[i].width, images[i].height);
    e.has_ink = false;  // (the old texels' boxes; pass 3 measures the new ones)
    B.tab[(size_t)i].x = e.x; B.tab[(size_t)i].y = e.y;
    B.entries[(size_t)i] = &e;
  }
  image_stats_.written = n;
  make_device_images(s, atlas, B, 0, n);
}
// the buffers of a whole batch, before any placement as every put reserves: the tables whatever atlas the batch ends in, a texel of
// scratch per tile, an ink block per tile of an image that gets ink boxes
void GlyphMaker::reserve_image_batch(const ImageBatch& B) {
  size_t tiles = 0, ink_tiles = 0;
  for (const ii::BatchImage& t : B.tab) {
    const size_t n = ib::table_tiles(t.w, t.h);
    tiles += n;
    if (ib::has_ink(t.w, t.h)) ink_tiles += n;
  }
  glyph_tab_.reserve(ib::table_words(B.tab, kMaxMips));
  glyph_a_.reserve(std::max<size_t>(tiles, 1));
  ink_host_.reserve_exact(std::max<size_t>(ink_tiles, ii::kInkTiles) * ii::kInkWords);
}
// A planar value as the texel's byte, the kernels' import_byte (k_image_import.hip) for the few elements the host converts itself: the one
// row or column of an image 1 texel wide or high, of which nothing is stored and which therefore has no tile in any launch.
static uint32_t host_import_byte(float v) {
  if (v != v) return 0u;
  const float c = std::fmin(std::fmax(v, 0.0f), 1.0f);
  return (uint32_t)std::nearbyint(c * 255.0f);
}
// the texels of such an image from `raw`: its planes one after the other, each n = w * h elements
static void host_import_line(const ii::BatchImage& t, const uint8_t* raw, std::vector<uint32_t>* out) {
  const size_t n = (size_t)t.w * t.h;
  out->resize(n);
  const bool straight = (t.flags & ii::kStraightAlpha) != 0;
  for (size_t i = 0; i < n; i++) {
    uint32_t r, g, b, a;
    if (t.format == ii::kRgba8) {
      uint32_t px;
      std::memcpy(&px, raw + 4 * i, 4);
      r = px & 255u; g = (px >> 8) & 255u; b = (px >> 16) & 255u; a = px >> 24;
    } else {
      auto value = [&](uint32_t plane) {
        if (t.format == ii::kPlanarF32) { float f; std::memcpy(&f, raw + 4 * ((size_t)plane * n + i), 4); return f; }
        uint16_t bits;
        std::memcpy(&bits, raw + 2 * ((size_t)plane * n + i), 2);
        return (float)__builtin_bit_cast(_Float16, bits);
      };
      r = g = b = host_import_byte(value(0)); a = 255u;
      if (t.channels >= 3u) { g = host_import_byte(value(1)); b = host_import_byte(value(2)); }
      if (t.channels == 4u) a = host_import_byte(value(3));
    }
    if (straight) { r = r * a / 255u; g = g * a / 255u; b = b * a / 255u; }
    (*out)[i] = r | (g << 8) | (b << 16) | (a << 24);
  }
}
// Pass 3 of both batches for images first .. first + m - 1, which have their entries: one copy of the tables, at most four launches, one
// wait; then the ink blocks folded per image.  A record-only context counts the tiles and is done.
void GlyphMaker::make_device_images(hipStream_t s, const Atlas& atlas, ImageBatch& B, int first, int m) {
  if (!atlas.has_device()) {
    for (int k = 0; k < m; k++) image_stats_.tiles += (int32_t)ib::table_tiles(B.tab[(size_t)(first + k)].w, B.tab[(size_t)(first + k)].h);
    return;
  }
  ib::Tables T;
  ib::tables(B.tab, first, m, atlas.n_levels(), &T);
  int launches = 0;
  if (T.n_tiles) {
    FDH_HIP(hipMemcpyAsync(glyph_tab_.ptr, T.words.data(), T.words.size() * 4, hipMemcpyHostToDevice, s));
    const ii::BatchImage* d_images = reinterpret_cast<const ii::BatchImage*>(glyph_tab_.ptr);
    const uint32_t* d_owner = glyph_tab_.ptr + T.owner_at;
    ii::BatchAtlas A{};
    for (int l = 0; l < atlas.n_levels(); l++) A.level[l] = atlas.level(l);
    A.size = atlas.size();
    for (int f = 0; f < ib::kFormats; f++) {
      if (!T.tile_count[f]) continue;
      launch_image_import_batch(s, (uint32_t)f, d_images, glyph_tab_.ptr + T.tiles_at + T.tile_first[f], (int)T.tile_count[f], A, glyph_a_.ptr, ink_host_.dev, d_owner);
      launches++;
    }
    if (T.n_tails) {
      launch_image_import_tail_batch(s, d_images, glyph_tab_.ptr + T.tails_at, (int)T.n_tails, A, glyph_a_.ptr, d_owner);
      launches++;
    }
    image_stats_.bytes_copied = (int64_t)(T.words.size() * 4);
  }
  // (an image 1 texel wide or high: its one row or column to the host, plane after plane)
  std::vector<std::vector<uint8_t>> lines((size_t)m);
  for (int k = 0; k < m; k++) {
    const ii::BatchImage& t = B.tab[(size_t)(first + k)];
    if (ib::table_tiles(t.w, t.h) || !ib::has_ink(t.w, t.h)) continue;
    const size_t element = t.format == ii::kPlanarF16 ? 2 : 4, planes = t.format != ii::kRgba8 && t.channels > 1u ? t.channels : 1u;
    const size_t row = (size_t)t.w * element, plane = row * t.h;
    lines[(size_t)k].resize(planes * plane);
    for (size_t c = 0; c < planes; c++)
      FDH_HIP(hipMemcpy2DAsync(lines[(size_t)k].data() + c * plane, row, static_cast<const char*>(B.sources[(size_t)(first + k)]) + (int64_t)c * t.plane_bytes, (size_t)t.pitch_bytes, row, (size_t)t.h,
                               hipMemcpyDefault, s));
  }
  FDH_HIP(hipStreamSynchronize(s));  // (`T` and `lines` stay alive until here)
  FDH_HIP(hipGetLastError());
  image_stats_.tiles = (int32_t)T.n_tiles;
  image_stats_.launches = launches;
  std::vector<uint32_t> texels;
  for (int k = 0; k < m; k++) {
    const ii::BatchImage& t = reinterpret_cast<const ii::BatchImage*>(T.words.data())[k];  // (its offsets are in the tables' copy)
    AtlasEntry& e = *B.entries[(size_t)(first + k)];
    int32_t got[ii::kInkWords];
    if (t.ink) {
      ii::fold_ink(ink_host_.ptr + (size_t)t.ink_off * ii::kInkWords, t.lw[ii::kTileLevels - 1] * t.lh[ii::kTileLevels - 1], got);
    } else if (!lines[(size_t)k].empty()) {
      host_import_line(t, lines[(size_t)k].data(), &texels);
      for (int i = 0; i < ii::kInkWords; i++) got[i] = (i & 2) ? 0 : ii::kInkEmpty;
      for (int i = 0; i < t.w * t.h; i++) {
        const uint32_t px = texels[(size_t)i];
        const int x = t.w == 1 ? 0 : i, y = t.w == 1 ? i : 0;
        const int value[2] = {(int)(px >> 24), (int)std::max(px & 255u, std::max((px >> 8) & 255u, (px >> 16) & 255u))};
        for (int kind = 0; kind < 2; kind++)
          for (int j = 0; j < kInkLevels && value[kind] > 16 * j; j++) {
            int32_t* box = got + 32 * kind + 4 * j;
            box[0] = std::min(box[0], x); box[1] = std::min(box[1], y); box[2] = std::max(box[2], x + 1); box[3] = std::max(box[3], y + 1);
          }
      }
    } else {
      e.has_ink = false;
      continue;
    }
    set_ink(e, got);
  }
}

// ---- decoded video frames (the specification: include_glyphs/figdraw_hip_video_frame.h).  put_device_image's placement, scratch, tail, wait and
// ink boxes; the struct, its rules and the first kernel are its own.
struct GlyphMaker::VideoSource {
  FdhVideoFrame frame;       // the caller's, copied
  const void* planes[2];     // as the device addresses them (a record-only context: null)
  bool wide_y, wide_c;       // a run of four luma samples / of two chroma pairs is one load (vi::Params)
};
// what both calls ask of the struct: no context, no device
static void validate_video_frame(const Refusal& bad, const FdhVideoFrame* f, bool* wide_y, bool* wide_c) {
  if (!f || !f->planes[0]) throw bad("null frame");
  if (f->width <= 0 || f->height <= 0) throw bad("empty frame");
  if (f->format > FDH_VIDEO_P010) throw bad("unknown format");
  if (f->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (f->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (f->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (f->reserved[0] || f->reserved[1]) throw bad("reserved must be 0");
  const bool bgra = f->format == FDH_VIDEO_BGRA8;
  const uint32_t alpha = f->flags & (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA);
  if (bgra) {
    if (f->matrix || f->range) throw bad("matrix and range must be 0 for BGRA8");
    if (f->planes[1] || f->pitch_bytes[1]) throw bad("BGRA8 has one plane");
    if (f->flags & FDH_VIDEO_CHROMA_LINEAR) throw bad("FDH_VIDEO_CHROMA_LINEAR needs a chroma plane");
    if (alpha == (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("FDH_VIDEO_STRAIGHT_ALPHA and FDH_VIDEO_IGNORE_ALPHA exclude each other");
  } else {
    if (!f->planes[1]) throw bad("null chroma plane");
    if (alpha) throw bad("the alpha flags are BGRA8's");
  }
  const int64_t luma = bgra ? 4 : f->format == FDH_VIDEO_P010 ? 2 : 1, pair = 2 * luma;  // the planes' element sizes
  if ((uintptr_t)f->planes[0] % (uintptr_t)luma || f->pitch_bytes[0] % luma) throw bad("planes[0] and pitch_bytes[0] must be multiples of the element size");
  if (f->pitch_bytes[0] < (int64_t)f->width * luma) throw bad("pitch_bytes[0] is below a row's bytes");
  const int64_t cw = ((int64_t)f->width + 1) / 2;
  if (!bgra) {
    if ((uintptr_t)f->planes[1] % (uintptr_t)pair || f->pitch_bytes[1] % pair) throw bad("planes[1] and pitch_bytes[1] must be multiples of a pair's size");
    if (f->pitch_bytes[1] < cw * pair) throw bad("pitch_bytes[1] is below a row's bytes");
  }
  const uintptr_t run = (uintptr_t)(4 * luma);  // four luma samples or texels; two pairs
  *wide_y = (uintptr_t)f->planes[0] % run == 0 && f->pitch_bytes[0] % (int64_t)run == 0 && f->width >= 4;
  *wide_c = !bgra && (uintptr_t)f->planes[1] % run == 0 && f->pitch_bytes[1] % (int64_t)run == 0 && cw >= 2;
}
// on a context with a device: both planes as the device addresses them, neither of them inside the atlas
static void video_planes(const Refusal& bad, int device, const Atlas& atlas, const FdhVideoFrame& f, const void* out[2]) {
  const int64_t cw = ((int64_t)f.width + 1) / 2, ch = ((int64_t)f.height + 1) / 2;
  const int64_t es = f.format == FDH_VIDEO_BGRA8 ? 4 : f.format == FDH_VIDEO_P010 ? 2 : 1;
  const int64_t bytes[2] = {(f.height - 1) * f.pitch_bytes[0] + f.width * es, (ch - 1) * f.pitch_bytes[1] + cw * 2 * es};
  out[0] = out[1] = nullptr;
  for (int p = 0; p < (f.format == FDH_VIDEO_BGRA8 ? 1 : 2); p++) {
    out[p] = device_address(bad, device, f.planes[p]);
    const uintptr_t lo = (uintptr_t)out[p], hi = lo + (uintptr_t)bytes[p];
    for (int l = 0; l < atlas.n_levels(); l++) {
      const uintptr_t a = (uintptr_t)atlas.level(l), side = (uintptr_t)(atlas.size() >> l);
      if (lo < a + side * side * 4 && a < hi) throw bad("a plane lies inside the context's own atlas");
    }
  }
}
void GlyphMaker::put_video_frame(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoFrame* frame, int out_rect[4]) {
  const Refusal bad{"put_video_frame"};
  VideoSource src{};
  validate_video_frame(bad, frame, &src.wide_y, &src.wide_c);
  src.frame = *frame;
  if (atlas.has_device()) {
    video_planes(bad, device, atlas, src.frame, src.planes);
    reserve_import(glyph_a_, glyph_b_, ink_host_, src.frame.width, src.frame.height);
  }
  atlas.make_room(s, src.frame.width, src.frame.height);
  AtlasEntry& e = atlas.place(s, key, src.frame.width, src.frame.height, out_rect);
  if (atlas.has_device()) import_video(s, atlas, e, src);
}
void GlyphMaker::update_video_frame(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoFrame* frame) {
  const Refusal bad{"update_video_frame"};
  VideoSource src{};
  validate_video_frame(bad, frame, &src.wide_y, &src.wide_c);
  src.frame = *frame;
  const AtlasEntry* old = atlas.find(key);  // (ahead of the pointers' check and the buffers; begin_update says the same again)
  if (!old) throw bad("unknown key");
  if (old->w != src.frame.width || old->h != src.frame.height) throw bad("size mismatch");
  if (atlas.has_device()) {
    video_planes(bad, device, atlas, src.frame, src.planes);
    reserve_import(glyph_a_, glyph_b_, ink_host_, src.frame.width, src.frame.height);
  }
  AtlasEntry& e = atlas.begin_update(bad.who, key, src.frame.width, src.frame.height);
  e.has_ink = false;  // (the old texels' boxes; import_video measures the new ones)
  if (atlas.has_device()) import_video(s, atlas, e, src);
}
// k_video_import makes levels 0 .. 5; the rest is import_image's (finish_import)
void GlyphMaker::import_video(hipStream_t s, const Atlas& atlas, AtlasEntry& e, const VideoSource& src) {
  const FdhVideoFrame& f = src.frame;
  vi::Params P{};
  P.luma = src.planes[0]; P.chroma = src.planes[1];
  P.pitch_y = f.pitch_bytes[0]; P.pitch_c = f.pitch_bytes[1];
  P.w = f.width; P.h = f.height; P.cw = (f.width + 1) / 2; P.ch = (f.height + 1) / 2;
  P.format = f.format; P.flags = f.flags;
  P.wide_y = src.wide_y; P.wide_c = src.wide_c;
  if (f.format != FDH_VIDEO_BGRA8) {
    const int32_t* c = vi::kCoefficients[f.format == FDH_VIDEO_P010][f.matrix][f.range];
    P.yoff = c[0]; P.coff = c[1]; P.cy = c[2]; P.crv = c[3]; P.cgu = c[4]; P.cgv = c[5]; P.cbu = c[6];
  }
  P.x = e.x; P.y = e.y;
  atlas.each_level(e.x, e.y, e.w, e.h, [&](int, int, int, int, int) { P.n_store++; });
  P.ink = e.w <= ii::kInkMax && e.h <= ii::kInkMax;
  for (int l = 0; l < ii::kTileLevels; l++) { P.lw[l] = (e.w + (1 << l) - 1) >> l; P.lh[l] = (e.h + (1 << l) - 1) >> l; }
  for (int l = 0; l < atlas.n_levels(); l++) P.level[l] = atlas.level(l);
  P.size = atlas.size();
  P.scratch = glyph_a_.ptr;
  P.ink_block = ink_host_.dev;
  launch_video_import(s, P);
  finish_import(s, atlas, e, P.n_store, P.ink != 0);
}
// fdh_video_coefficients: a row of the table (fdh_video_import.h)
void video_coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[7]) {
  const Refusal bad{"video_coefficients"};
  if (format != FDH_VIDEO_NV12 && format != FDH_VIDEO_P010) throw bad("the format has no conversion: FDH_VIDEO_NV12 or FDH_VIDEO_P010");
  if (matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (!out) throw bad("null pointer");
  std::copy(vi::kCoefficients[format == FDH_VIDEO_P010][matrix][range], vi::kCoefficients[format == FDH_VIDEO_P010][matrix][range] + 7, out);
}

// ---- batches of decoded video frames (the specification: include_glyphs/figdraw_hip_video_frames.h).  put_device_images' three passes: every
// frame is validated; every frame is placed (an update: begun), in order; then the frames that are still in the atlas get their texels from
// one launch per group present (vi::batch_group) and one for the tails, over the tables of fdh_video_batch.h.
struct GlyphMaker::VideoBatch {
  std::vector<vi::BatchFrame> tab;   // pass 1: planes as the device addresses them, pitches, extents, format, flags, wide, the conversion; pass 2: the place
  std::vector<AtlasEntry*> entries;  // pass 2: the entries (a placement never moves the ones behind the last growth)
};
// Pass 1 of both batches.  Nothing behind it refuses a frame.
void GlyphMaker::validate_video_frames(const char* who, const Atlas& atlas, int device, const int64_t* keys, const FdhVideoFrame* frames, int n, bool update, VideoBatch* B) {
  const Refusal bad{who};
  if (n < 0 || (n > 0 && (!keys || !frames))) throw bad("bad frame array");
  if (n > vb::kMaxFrames) throw bad("at most 65535 frames");
  B->tab.assign((size_t)n, vi::BatchFrame{});
  B->entries.assign((size_t)n, nullptr);
  std::unordered_set<int64_t> seen;
  int64_t tiles = 0;
  for (int i = 0; i < n; i++) {
    const FdhVideoFrame& f = frames[i];
    bool wide_y, wide_c;
    validate_video_frame(bad, &f, &wide_y, &wide_c);
    if (f.width > ii::kBatchMaxExtent || f.height > ii::kBatchMaxExtent) throw bad("a frame of a batch is at most 2048 x 2048");
    if (!seen.insert(keys[i]).second) throw bad("a key occurs twice");
    if (update) {
      const AtlasEntry* old = atlas.find(keys[i]);
      if (!old) throw bad("unknown key");
      if (old->w != f.width || old->h != f.height) throw bad("size mismatch");
    }
    tiles += (int64_t)vb::tiles_of(f.width, f.height);
    vi::BatchFrame& t = B->tab[(size_t)i];
    t.pitch_y = f.pitch_bytes[0]; t.pitch_c = f.pitch_bytes[1];
    t.w = f.width; t.h = f.height; t.cw = (f.width + 1) / 2; t.ch = (f.height + 1) / 2;
    t.format = f.format; t.flags = f.flags;
    t.wide_y = wide_y; t.wide_c = wide_c;
    if (f.format != FDH_VIDEO_BGRA8) {
      const int32_t* c = vi::kCoefficients[f.format == FDH_VIDEO_P010][f.matrix][f.range];
      t.yoff = c[0]; t.coff = c[1]; t.cy = c[2]; t.crv = c[3]; t.cgu = c[4]; t.cgv = c[5]; t.cbu = c[6];
    }
  }
  if (tiles > vb::kMaxTiles) throw bad("at most 2^18 tiles in a batch");
  if (!atlas.has_device()) return;
  for (int i = 0; i < n; i++) {
    const void* planes[2];
    video_planes(bad, device, atlas, frames[i], planes);
    B->tab[(size_t)i].luma = planes[0]; B->tab[(size_t)i].chroma = planes[1];
  }
}
void GlyphMaker::put_video_frames(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhVideoFrame* frames, int n, int (*out_rects)[4]) {
  VideoBatch B;
  validate_video_frames("put_video_frames", atlas, device, keys, frames, n, false, &B);
  video_stats_ = FdhVideoBatchStats{};
  video_stats_.frames = n;
  if (n == 0) return;
  if (atlas.has_device()) reserve_video_batch(B);
  // ---- pass 2: the places (keep mode: room for all frames of the batch at once, before any of them has a place)
  if (atlas.keep()) {
    std::vector<int> wh((size_t)n * 2);
    for (int i = 0; i < n; i++) { wh[(size_t)i * 2] = frames[i].width; wh[(size_t)i * 2 + 1] = frames[i].height; }
    atlas.make_room(s, reinterpret_cast<const int (*)[2]>(wh.data()), n);
  }
  int first = 0, placed = 0;
  std::exception_ptr failed = place_batch(s, atlas, n, out_rects, Stored::chain,
                                          [&](int i, int64_t* key, int* w, int* h) { *key = keys[i]; *w = frames[i].width; *h = frames[i].height; },
                                          [&](int i, AtlasEntry& e) { B.tab[(size_t)i].x = e.x; B.tab[(size_t)i].y = e.y; B.entries[(size_t)i] = &e; }, &first, &placed);
  video_stats_.written = placed - first;
  video_stats_.dropped_by_growth = first;
  // ---- pass 3: the texels of frames first .. placed - 1
  if (placed > first) make_video_frames(s, atlas, B, first, placed - first);
  if (failed) std::rethrow_exception(failed);
}
void GlyphMaker::update_video_frames(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhVideoFrame* frames, int n) {
  VideoBatch B;
  validate_video_frames("update_video_frames", atlas, device, keys, frames, n, true, &B);
  video_stats_ = FdhVideoBatchStats{};
  video_stats_.frames = n;
  if (n == 0) return;
  if (atlas.has_device()) reserve_video_batch(B);
  for (int i = 0; i < n; i++) {
    AtlasEntry& e = atlas.begin_update("update_video_frames", keys[i], frames[i].width, frames[i].height);
    e.has_ink = false;  // (the old texels' boxes; pass 3 measures the new ones)
    B.tab[(size_t)i].x = e.x; B.tab[(size_t)i].y = e.y;
    B.entries[(size_t)i] = &e;
  }
  video_stats_.written = n;
  make_video_frames(s, atlas, B, 0, n);
}
// the buffers of a whole batch, before any placement as every put reserves: the tables whatever atlas the batch ends in, a texel of
// scratch per tile, an ink block per tile of a frame that gets ink boxes
void GlyphMaker::reserve_video_batch(const VideoBatch& B) {
  size_t tiles = 0, ink_tiles = 0;
  for (const vi::BatchFrame& t : B.tab) {
    const size_t n = vb::tiles_of(t.w, t.h);
    tiles += n;
    if (vb::has_ink(t.w, t.h)) ink_tiles += n;
  }
  glyph_tab_.reserve(vb::table_words(B.tab, kMaxMips));
  glyph_a_.reserve(std::max<size_t>(tiles, 1));
  ink_host_.reserve_exact(std::max<size_t>(ink_tiles, ii::kInkTiles) * ii::kInkWords);
}
// Pass 3 of both batches for frames first .. first + m - 1, which have their entries: one copy of the tables, at most six launches, one
// wait; then the ink blocks folded per frame.  A record-only context counts the tiles and is done.
void GlyphMaker::make_video_frames(hipStream_t s, const Atlas& atlas, VideoBatch& B, int first, int m) {
  if (!atlas.has_device()) {
    for (int k = 0; k < m; k++) video_stats_.tiles += (int32_t)vb::tiles_of(B.tab[(size_t)(first + k)].w, B.tab[(size_t)(first + k)].h);
    return;
  }
  vb::Tables T;
  vb::tables(B.tab, first, m, atlas.n_levels(), &T);
  FDH_HIP(hipMemcpyAsync(glyph_tab_.ptr, T.words.data(), T.words.size() * 4, hipMemcpyHostToDevice, s));
  const vi::BatchFrame* d_frames = reinterpret_cast<const vi::BatchFrame*>(glyph_tab_.ptr);
  const uint32_t* d_owner = glyph_tab_.ptr + T.owner_at;
  ii::BatchAtlas A{};
  for (int l = 0; l < atlas.n_levels(); l++) A.level[l] = atlas.level(l);
  A.size = atlas.size();
  int launches = 0;
  for (int g = 0; g < vb::kGroups; g++) {
    if (!T.tile_count[g]) continue;
    launch_video_import_batch(s, g, d_frames, glyph_tab_.ptr + T.tiles_at + T.tile_first[g], (int)T.tile_count[g], A, glyph_a_.ptr, ink_host_.dev, d_owner);
    launches++;
  }
  if (T.n_tails) {
    launch_image_import_tail_batch(s, reinterpret_cast<const ii::BatchImage*>(glyph_tab_.ptr + T.tail_records_at), glyph_tab_.ptr + T.tails_at, (int)T.n_tails, A, glyph_a_.ptr, d_owner);
    launches++;
  }
  FDH_HIP(hipStreamSynchronize(s));  // (`T` stays alive until here)
  FDH_HIP(hipGetLastError());
  video_stats_.bytes_copied = (int64_t)(T.words.size() * 4);
  video_stats_.tiles = (int32_t)T.n_tiles;
  video_stats_.launches = launches;
  for (int k = 0; k < m; k++) {
    const vi::BatchFrame& t = B.tab[(size_t)(first + k)];  // (tables() filled in its offsets)
    AtlasEntry& e = *B.entries[(size_t)(first + k)];
    e.has_ink = t.ink != 0;
    if (!t.ink) continue;
    int32_t got[ii::kInkWords];
    ii::fold_ink(ink_host_.ptr + (size_t)t.ink_off * ii::kInkWords, t.lw[ii::kTileLevels - 1] * t.lh[ii::kTileLevels - 1], got);
    set_ink(e, got);
  }
}

// ---- three-plane video frames (the specification: include_video/figdraw_hip_video_planar.h).  put_video_frame's steps; the struct, its
// rules and the first kernel are its own.
struct GlyphMaker::PlanarSource {
  FdhVideoPlanes frame;      // the caller's, copied
  const void* planes[3];     // as the device addresses them (a record-only context: null)
  bool wide[3];              // a run of plane p is one load (vp::InParams)
};
// what both calls ask of the struct: no context, no device
static void validate_video_planes(const Refusal& bad, const FdhVideoPlanes* f, bool wide[3]) {
  if (!f || !f->planes[0] || !f->planes[1] || !f->planes[2]) throw bad("null frame or plane");
  if (f->width <= 0 || f->height <= 0) throw bad("empty frame");
  if (f->format < FDH_VIDEO_I420 || f->format > FDH_VIDEO_I410) throw bad("unknown format");
  if (f->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (f->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (f->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (f->reserved[0] || f->reserved[1]) throw bad("reserved must be 0");
  if (f->flags & (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("the alpha flags are BGRA8's");
  const bool full = vp::full_chroma(f->format);
  if (full && (f->flags & FDH_VIDEO_CHROMA_LINEAR)) throw bad("FDH_VIDEO_CHROMA_LINEAR is for I420 / I010: a 4:4:4 frame has a chroma sample per texel");
  const int64_t es = vp::ten_bit(f->format) ? 2 : 1;  // the sample size
  const int64_t cw = full ? (int64_t)f->width : ((int64_t)f->width + 1) / 2;
  for (int p = 0; p < 3; p++) {
    const int64_t row = p ? cw : (int64_t)f->width, run = (p && !full ? vp::kRun / 2 : vp::kRun) * es;
    if ((uintptr_t)f->planes[p] % (uintptr_t)es || f->pitch_bytes[p] % es) throw bad("planes[" + std::to_string(p) + "] and pitch_bytes[" + std::to_string(p) + "] must be multiples of the sample size");
    if (f->pitch_bytes[p] < row * es) throw bad("pitch_bytes[" + std::to_string(p) + "] is below a row's bytes");
    wide[p] = (uintptr_t)f->planes[p] % (uintptr_t)run == 0 && f->pitch_bytes[p] % run == 0 && row * es >= run;
  }
}
// on a context with a device: the planes as the device addresses them, none of them inside the atlas
static void video_planes_on_device(const Refusal& bad, int device, const Atlas& atlas, const FdhVideoPlanes& f, const void* out[3], bool wide[3]) {
  const bool full = vp::full_chroma(f.format);
  const int64_t es = vp::ten_bit(f.format) ? 2 : 1;
  const int64_t cw = full ? (int64_t)f.width : ((int64_t)f.width + 1) / 2, ch = full ? (int64_t)f.height : ((int64_t)f.height + 1) / 2;
  for (int p = 0; p < 3; p++) {
    const int64_t bytes = ((p ? ch : (int64_t)f.height) - 1) * f.pitch_bytes[p] + (p ? cw : (int64_t)f.width) * es;
    out[p] = device_address(bad, device, f.planes[p]);
    const uintptr_t lo = (uintptr_t)out[p], hi = lo + (uintptr_t)bytes;
    for (int l = 0; l < atlas.n_levels(); l++) {
      const uintptr_t a = (uintptr_t)atlas.level(l), side = (uintptr_t)(atlas.size() >> l);
      if (lo < a + side * side * 4 && a < hi) throw bad("a plane lies inside the context's own atlas");
    }
    // (a page-locked plane's device view need not be aligned as the caller's pointer is: the question is asked of the address the kernel gets)
    wide[p] = wide[p] && lo % (uintptr_t)((p && !full ? vp::kRun / 2 : vp::kRun) * es) == 0;
  }
}
void GlyphMaker::put_video_planes(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame, int out_rect[4]) {
  const Refusal bad{"put_video_planes"};
  PlanarSource src{};
  validate_video_planes(bad, frame, src.wide);
  src.frame = *frame;
  if (atlas.has_device()) {
    video_planes_on_device(bad, device, atlas, src.frame, src.planes, src.wide);
    reserve_import(glyph_a_, glyph_b_, ink_host_, src.frame.width, src.frame.height);
  }
  atlas.make_room(s, src.frame.width, src.frame.height);
  AtlasEntry& e = atlas.place(s, key, src.frame.width, src.frame.height, out_rect);
  if (atlas.has_device()) import_video_planes(s, atlas, e, src);
}
void GlyphMaker::update_video_planes(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame) {
  const Refusal bad{"update_video_planes"};
  PlanarSource src{};
  validate_video_planes(bad, frame, src.wide);
  src.frame = *frame;
  const AtlasEntry* old = atlas.find(key);  // (ahead of the pointers' check and the buffers; begin_update says the same again)
  if (!old) throw bad("unknown key");
  if (old->w != src.frame.width || old->h != src.frame.height) throw bad("size mismatch");
  if (atlas.has_device()) {
    video_planes_on_device(bad, device, atlas, src.frame, src.planes, src.wide);
    reserve_import(glyph_a_, glyph_b_, ink_host_, src.frame.width, src.frame.height);
  }
  AtlasEntry& e = atlas.begin_update(bad.who, key, src.frame.width, src.frame.height);
  e.has_ink = false;  // (the old texels' boxes; import_video_planes measures the new ones)
  if (atlas.has_device()) import_video_planes(s, atlas, e, src);
}
// k_video_planar_import makes levels 0 .. 5; the rest is import_image's (finish_import)
void GlyphMaker::import_video_planes(hipStream_t s, const Atlas& atlas, AtlasEntry& e, const PlanarSource& src) {
  const FdhVideoPlanes& f = src.frame;
  const bool full = vp::full_chroma(f.format);
  vp::InParams P{};
  for (int p = 0; p < 3; p++) { P.plane[p] = src.planes[p]; P.pitch[p] = f.pitch_bytes[p]; P.wide[p] = src.wide[p]; }
  P.w = f.width; P.h = f.height; P.cw = full ? f.width : (f.width + 1) / 2; P.ch = full ? f.height : (f.height + 1) / 2;
  P.format = f.format; P.flags = f.flags;
  const int32_t* c = vi::kCoefficients[vp::ten_bit(f.format)][f.matrix][f.range];  // (the NV12 row for 8 bit, the P010 row for 10)
  P.yoff = c[0]; P.coff = c[1]; P.cy = c[2]; P.crv = c[3]; P.cgu = c[4]; P.cgv = c[5]; P.cbu = c[6];
  P.x = e.x; P.y = e.y;
  atlas.each_level(e.x, e.y, e.w, e.h, [&](int, int, int, int, int) { P.n_store++; });
  P.ink = e.w <= ii::kInkMax && e.h <= ii::kInkMax;
  for (int l = 0; l < ii::kTileLevels; l++) { P.lw[l] = (e.w + (1 << l) - 1) >> l; P.lh[l] = (e.h + (1 << l) - 1) >> l; }
  for (int l = 0; l < atlas.n_levels(); l++) P.level[l] = atlas.level(l);
  P.size = atlas.size();
  P.scratch = glyph_a_.ptr;
  P.ink_block = ink_host_.dev;
  launch_video_planar_import(s, P);
  finish_import(s, atlas, e, P.n_store, P.ink != 0);
}

// ---- 4:2:2 video frames (the specification: include_video/figdraw_hip_video_422.h).  put_video_planes's steps, struct, placement and
// finish_import; the formats, their rules and the first kernel are its own.  A packed format has planes[0] alone.
// what both calls ask of the struct: no context, no device
static void validate_video_422(const Refusal& bad, const FdhVideoPlanes* f, bool wide[3]) {
  if (!f || !f->planes[0]) throw bad("null frame or plane");
  if (f->width <= 0 || f->height <= 0) throw bad("empty frame");
  if (!v2::known(f->format)) throw bad("unknown format");
  if (f->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (f->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (f->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (f->reserved[0] || f->reserved[1]) throw bad("reserved must be 0");
  if (f->flags & (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("the alpha flags are BGRA8's");
  const bool packed = v2::packed(f->format);
  if (packed && (f->planes[1] || f->planes[2] || f->pitch_bytes[1] || f->pitch_bytes[2])) throw bad("planes[1], planes[2] and their pitches must be 0 for YUY2 / UYVY: one plane");
  if (!packed && (!f->planes[1] || !f->planes[2])) throw bad("null frame or plane");
  const int64_t es = v2::element_bytes(f->format), cw = ((int64_t)f->width + 1) / 2;
  for (int p = 0; p < v2::n_planes(f->format); p++) {
    const int64_t row = packed ? 4 * cw : (p ? cw : (int64_t)f->width) * es, run = v2::run_bytes(f->format, p);
    if ((uintptr_t)f->planes[p] % (uintptr_t)es || f->pitch_bytes[p] % es)
      throw bad("planes[" + std::to_string(p) + "] and pitch_bytes[" + std::to_string(p) + "] must be multiples of the " + (packed ? "group size" : "sample size"));
    if (f->pitch_bytes[p] < row) throw bad("pitch_bytes[" + std::to_string(p) + "] is below a row's bytes");
    wide[p] = (uintptr_t)f->planes[p] % (uintptr_t)run == 0 && f->pitch_bytes[p] % run == 0 && row >= run;
  }
}
// on a context with a device: the planes as the device addresses them, none of them inside the atlas
static void video_422_on_device(const Refusal& bad, int device, const Atlas& atlas, const FdhVideoPlanes& f, const void* out[3], bool wide[3]) {
  const bool packed = v2::packed(f.format);
  const int64_t es = v2::element_bytes(f.format), cw = ((int64_t)f.width + 1) / 2;
  for (int p = 0; p < v2::n_planes(f.format); p++) {
    const int64_t bytes = ((int64_t)f.height - 1) * f.pitch_bytes[p] + (packed ? 4 * cw : (p ? cw : (int64_t)f.width) * es);
    out[p] = device_address(bad, device, f.planes[p]);
    const uintptr_t lo = (uintptr_t)out[p], hi = lo + (uintptr_t)bytes;
    for (int l = 0; l < atlas.n_levels(); l++) {
      const uintptr_t a = (uintptr_t)atlas.level(l), side = (uintptr_t)(atlas.size() >> l);
      if (lo < a + side * side * 4 && a < hi) throw bad("a plane lies inside the context's own atlas");
    }
    // (a page-locked plane's device view need not be aligned as the caller's pointer is: the question is asked of the address the kernel gets)
    wide[p] = wide[p] && lo % (uintptr_t)v2::run_bytes(f.format, p) == 0;
  }
}
void GlyphMaker::put_video_422(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame, int out_rect[4]) {
  const Refusal bad{"put_video_422"};
  PlanarSource src{};
  validate_video_422(bad, frame, src.wide);
  src.frame = *frame;
  if (atlas.has_device()) {
    video_422_on_device(bad, device, atlas, src.frame, src.planes, src.wide);
    reserve_import(glyph_a_, glyph_b_, ink_host_, src.frame.width, src.frame.height);
  }
  atlas.make_room(s, src.frame.width, src.frame.height);
  AtlasEntry& e = atlas.place(s, key, src.frame.width, src.frame.height, out_rect);
  if (atlas.has_device()) import_video_422(s, atlas, e, src);
}
void GlyphMaker::update_video_422(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame) {
  const Refusal bad{"update_video_422"};
  PlanarSource src{};
  validate_video_422(bad, frame, src.wide);
  src.frame = *frame;
  const AtlasEntry* old = atlas.find(key);  // (ahead of the pointers' check and the buffers; begin_update says the same again)
  if (!old) throw bad("unknown key");
  if (old->w != src.frame.width || old->h != src.frame.height) throw bad("size mismatch");
  if (atlas.has_device()) {
    video_422_on_device(bad, device, atlas, src.frame, src.planes, src.wide);
    reserve_import(glyph_a_, glyph_b_, ink_host_, src.frame.width, src.frame.height);
  }
  AtlasEntry& e = atlas.begin_update(bad.who, key, src.frame.width, src.frame.height);
  e.has_ink = false;  // (the old texels' boxes; import_video_422 measures the new ones)
  if (atlas.has_device()) import_video_422(s, atlas, e, src);
}
// k_video_422_import makes levels 0 .. 5; the rest is import_image's (finish_import)
void GlyphMaker::import_video_422(hipStream_t s, const Atlas& atlas, AtlasEntry& e, const PlanarSource& src) {
  const FdhVideoPlanes& f = src.frame;
  v2::InParams P{};
  for (int p = 0; p < v2::n_planes(f.format); p++) { P.plane[p] = src.planes[p]; P.pitch[p] = f.pitch_bytes[p]; P.wide[p] = src.wide[p]; }
  P.w = f.width; P.h = f.height; P.cw = (f.width + 1) / 2;
  P.format = f.format; P.flags = f.flags; P.order = f.format == v2::kUYVY;
  const int32_t* c = vi::kCoefficients[v2::ten_bit(f.format)][f.matrix][f.range];  // (the NV12 row for 8 bit, the P010 row for 10)
  P.yoff = c[0]; P.coff = c[1]; P.cy = c[2]; P.crv = c[3]; P.cgu = c[4]; P.cgv = c[5]; P.cbu = c[6];
  P.x = e.x; P.y = e.y;
  atlas.each_level(e.x, e.y, e.w, e.h, [&](int, int, int, int, int) { P.n_store++; });
  P.ink = e.w <= ii::kInkMax && e.h <= ii::kInkMax;
  for (int l = 0; l < ii::kTileLevels; l++) { P.lw[l] = (e.w + (1 << l) - 1) >> l; P.lh[l] = (e.h + (1 << l) - 1) >> l; }
  for (int l = 0; l < atlas.n_levels(); l++) P.level[l] = atlas.level(l);
  P.size = atlas.size();
  P.scratch = glyph_a_.ptr;
  P.ink_block = ink_host_.dev;
  launch_video_422_import(s, P);
  finish_import(s, atlas, e, P.n_store, P.ink != 0);
}

// ---- video frames with an alpha plane (the specification: include_video/figdraw_hip_video_alpha.h).  put_video_422's steps, placement and
// finish_import; the struct has four slots, and the formats, their rules and the first kernel are its own.  UYVA has planes[0] and [3].
struct GlyphMaker::AlphaSource {
  FdhVideoAlphaPlanes frame;      // the caller's, copied
  const void* planes[va::kPlanes];  // as the device addresses them (a record-only context: null)
  bool wide[va::kPlanes];           // a run of plane p is one load (va::InParams)
};
// what both calls ask of the struct: no context, no device
static void validate_video_alpha(const Refusal& bad, const FdhVideoAlphaPlanes* f, bool wide[va::kPlanes]) {
  if (!f || !f->planes[0] || !f->planes[va::kAlpha]) throw bad("null frame or plane");
  if (f->width <= 0 || f->height <= 0) throw bad("empty frame");
  if (!va::known(f->format)) throw bad("unknown format");
  if (f->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (f->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (f->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (f->reserved[0] || f->reserved[1]) throw bad("reserved must be 0");
  if (f->flags & FDH_VIDEO_IGNORE_ALPHA) throw bad("FDH_VIDEO_IGNORE_ALPHA is the sibling call: these formats carry an alpha plane");
  if (va::full_chroma(f->format) && (f->flags & FDH_VIDEO_CHROMA_LINEAR)) throw bad("FDH_VIDEO_CHROMA_LINEAR is for A420 / UYVA: a 4:4:4 frame has a chroma sample per texel");
  const bool packed = va::packed(f->format);
  if (packed && (f->planes[1] || f->planes[2] || f->pitch_bytes[1] || f->pitch_bytes[2])) throw bad("planes[1], planes[2] and their pitches must be 0 for UYVA: a UYVY plane and an alpha plane");
  if (!packed && (!f->planes[1] || !f->planes[2])) throw bad("null frame or plane");
  for (int p = 0; p < va::kPlanes; p++) {
    wide[p] = false;
    if (!va::has_plane(f->format, p)) continue;
    const int64_t es = va::element_bytes(f->format, p), row = va::row_bytes(f->format, p, f->width), run = va::run_bytes(f->format, p);
    if ((uintptr_t)f->planes[p] % (uintptr_t)es || f->pitch_bytes[p] % es)
      throw bad("planes[" + std::to_string(p) + "] and pitch_bytes[" + std::to_string(p) + "] must be multiples of the " + (es == 4 ? "group size" : "sample size"));
    if (f->pitch_bytes[p] < row) throw bad("pitch_bytes[" + std::to_string(p) + "] is below a row's bytes");
    wide[p] = (uintptr_t)f->planes[p] % (uintptr_t)run == 0 && f->pitch_bytes[p] % run == 0 && row >= run;
  }
}
// on a context with a device: the planes as the device addresses them, none of them inside the atlas
static void video_alpha_on_device(const Refusal& bad, int device, const Atlas& atlas, const FdhVideoAlphaPlanes& f, const void* out[va::kPlanes], bool wide[va::kPlanes]) {
  for (int p = 0; p < va::kPlanes; p++) {
    if (!va::has_plane(f.format, p)) continue;
    const int64_t bytes = (va::rows(f.format, p, f.height) - 1) * f.pitch_bytes[p] + va::row_bytes(f.format, p, f.width);
    out[p] = device_view_of(device, f.planes[p]);
    if (!out[p]) throw bad("a plane is neither device memory of the context's device nor page-locked host memory");
    const uintptr_t lo = (uintptr_t)out[p], hi = lo + (uintptr_t)bytes;
    for (int l = 0; l < atlas.n_levels(); l++) {
      const uintptr_t a = (uintptr_t)atlas.level(l), side = (uintptr_t)(atlas.size() >> l);
      if (lo < a + side * side * 4 && a < hi) throw bad("a plane lies inside the context's own atlas");
    }
    // (a page-locked plane's device view need not be aligned as the caller's pointer is: the question is asked of the address the kernel gets)
    wide[p] = wide[p] && lo % (uintptr_t)va::run_bytes(f.format, p) == 0;
  }
}
void GlyphMaker::put_video_alpha(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoAlphaPlanes* frame, int out_rect[4]) {
  const Refusal bad{"put_video_alpha"};
  AlphaSource src{};
  validate_video_alpha(bad, frame, src.wide);
  src.frame = *frame;
  if (atlas.has_device()) {
    video_alpha_on_device(bad, device, atlas, src.frame, src.planes, src.wide);
    reserve_import(glyph_a_, glyph_b_, ink_host_, src.frame.width, src.frame.height);
  }
  atlas.make_room(s, src.frame.width, src.frame.height);
  AtlasEntry& e = atlas.place(s, key, src.frame.width, src.frame.height, out_rect);
  if (atlas.has_device()) import_video_alpha(s, atlas, e, src);
}
void GlyphMaker::update_video_alpha(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoAlphaPlanes* frame) {
  const Refusal bad{"update_video_alpha"};
  AlphaSource src{};
  validate_video_alpha(bad, frame, src.wide);
  src.frame = *frame;
  const AtlasEntry* old = atlas.find(key);  // (ahead of the pointers' check and the buffers; begin_update says the same again)
  if (!old) throw bad("unknown key");
  if (old->w != src.frame.width || old->h != src.frame.height) throw bad("size mismatch");
  if (atlas.has_device()) {
    video_alpha_on_device(bad, device, atlas, src.frame, src.planes, src.wide);
    reserve_import(glyph_a_, glyph_b_, ink_host_, src.frame.width, src.frame.height);
  }
  AtlasEntry& e = atlas.begin_update(bad.who, key, src.frame.width, src.frame.height);
  e.has_ink = false;  // (the old texels' boxes; import_video_alpha measures the new ones)
  if (atlas.has_device()) import_video_alpha(s, atlas, e, src);
}
// k_video_alpha_import makes levels 0 .. 5; the rest is import_image's (finish_import)
void GlyphMaker::import_video_alpha(hipStream_t s, const Atlas& atlas, AtlasEntry& e, const AlphaSource& src) {
  const FdhVideoAlphaPlanes& f = src.frame;
  va::InParams P{};
  for (int p = 0; p < va::kPlanes; p++)
    if (va::has_plane(f.format, p)) { P.plane[p] = src.planes[p]; P.pitch[p] = f.pitch_bytes[p]; P.wide[p] = src.wide[p]; }
  P.w = f.width; P.h = f.height;
  P.cw = va::full_chroma(f.format) ? f.width : (f.width + 1) / 2; P.ch = (int)va::rows(f.format, 1, f.height);
  P.format = f.format; P.flags = f.flags;
  const int32_t* c = vi::kCoefficients[va::ten_bit(f.format)][f.matrix][f.range];  // (the NV12 row for 8 bit, the P010 row for 10)
  P.yoff = c[0]; P.coff = c[1]; P.cy = c[2]; P.crv = c[3]; P.cgu = c[4]; P.cgv = c[5]; P.cbu = c[6];
  P.x = e.x; P.y = e.y;
  atlas.each_level(e.x, e.y, e.w, e.h, [&](int, int, int, int, int) { P.n_store++; });
  P.ink = e.w <= ii::kInkMax && e.h <= ii::kInkMax;
  for (int l = 0; l < ii::kTileLevels; l++) { P.lw[l] = (e.w + (1 << l) - 1) >> l; P.lh[l] = (e.h + (1 << l) - 1) >> l; }
  for (int l = 0; l < atlas.n_levels(); l++) P.level[l] = atlas.level(l);
  P.size = atlas.size();
  P.scratch = glyph_a_.ptr;
  P.ink_block = ink_host_.dev;
  launch_video_alpha_import(s, P);
  finish_import(s, atlas, e, P.n_store, P.ink != 0);
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
// Pass 2 of a batch of glyphs or of images: every item through place(), in order; item(i, &key, &w, &h) names it, placed_at(i, entry) takes its
// place.  A placement that grows the atlas has dropped every entry before it: item i is then the first of the new atlas (*first).  *placed:
// the items that got a place; the exception that ended the loop (FDH_ERR_ATLAS_FULL, or no memory for a larger atlas) is returned: the items
// before that one get their texels, as after single calls.
template <typename Item, typename PlacedAt>
static std::exception_ptr place_batch(hipStream_t s, Atlas& atlas, int n, int (*out_rects)[4], Stored stored, Item item, PlacedAt placed_at, int* first, int* placed) {
  std::exception_ptr failed;
  int f = 0, p = 0;
  for (; p < n; p++) {
    const int before = atlas.size();
    try {
      int64_t key;
      int w, h;
      item(p, &key, &w, &h);
      placed_at(p, atlas.place(s, key, w, h, out_rects ? out_rects[p] : nullptr, stored));
    } catch (...) {
      failed = std::current_exception();
    }
    if (atlas.size() != before) f = p;
    if (failed) break;
  }
  *first = f; *placed = p;
  return failed;
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
