// fdh_atlas.cpp -- class Atlas (fdh_atlas.h), the image atlas: directory and skyline packer, level chains, glyph images and outlines, the Flippy container.
#include "fdh_context.h"
#include "fdh_msdf_host.h"
#include "fdh_msdf_cubic_host.h"

#include <algorithm>
#include <cmath>
#include <climits>
#include <cstring>
#include <exception>
#include <string>

namespace fdh {

// ------------------------------------------------------------------ directory and packer (glcontext.nim:536-641, textures.nim:88-119)
void Atlas::init(int size, bool device, hipStream_t s) {
  device_ = device;
  initial_size_ = size > 0 ? size : 1024;  // newContext default, glcontext.nim:255-261
  alloc(initial_size_, s);
}
// An empty atlas of `size` (rounded up to a power of two) takes the place of this one.  The new levels are allocated FIRST (DeviceBuf::reserve's
// rule): a failing hipMalloc frees what it got and leaves the old atlas whole -- levels, entries, skyline, size and epoch.  For the
// length of a grow both atlases exist: peak memory is the new one plus the old one.
void Atlas::alloc(int size, hipStream_t s) {
  int sz = 1;
  while (sz < size) sz <<= 1;  // the samplers mask coordinates: keep the atlas a power of two
  uint32_t* fresh[kMaxMips] = {};
  int n = 0;
  try {
    for (int ls = sz; ls >= 1 && n < kMaxMips; ls >>= 1) {
      if (device_) {
        FDH_HIP(hipMalloc((void**)&fresh[n], (size_t)ls * ls * 4));
        FDH_HIP(hipMemsetAsync(fresh[n], 0, (size_t)ls * ls * 4, s));
      }
      n++;
    }
    if (device_) FDH_HIP(hipStreamSynchronize(s));  // host uploads (upload_rect) are not ordered behind the stream: the zeros are there first
  } catch (...) {
    for (auto l : fresh) if (l) (void)hipFree(l);
    throw;
  }
  release_levels();
  std::copy(fresh, fresh + kMaxMips, levels_);
  size_ = sz;
  n_levels_ = n;
  heights_.assign((size_t)sz, 0);
  entries_.clear();
  epoch_++;
}
void Atlas::release_levels() {
  for (auto& l : levels_) { if (l) (void)hipFree(l); l = nullptr; }
}
void Atlas::release() {
  release_levels();
  glyph_a_.release(); glyph_b_.release(); glyph_lines_.release(); glyph_acc_.release(); glyph_edges_.release(); glyph_tab_.release();
}
void Atlas::reset(int minimum_size, hipStream_t s) {
  int sz = initial_size_;
  while (sz < minimum_size) sz *= 2;  // plannedAtlasSize
  alloc(sz, s);
}
int64_t Atlas::packed_area() const {
  int64_t a = 0;
  for (auto h : heights_) a += h;
  return a;
}
AtlasView Atlas::view() const {
  AtlasView v{};
  for (int l = 0; l < kMaxMips; l++) v.level[l] = levels_[l];
  v.size = size_; v.n_levels = n_levels_;
  return v;
}
// Every put's way into the directory: the skyline search (glcontext.nim:541-579), growing until the image fits, then the entry, the
// epoch and the caller's out_rect.  The returned entry has no ink boxes.
AtlasEntry& Atlas::place(hipStream_t s, int64_t key, int w, int h, int out_rect[4]) {
  for (;;) {
    const int S = size_, M = margin_;
    const int iw = w + M * 2, ih = h + M * 2;
    int lowest = S, at = 0;
    for (int i = 0; i < S; i++) {
      int v = heights_[i];
      if (v < lowest) {
        bool fit = true;
        for (int j = 0; j <= iw; j++) {
          if (i + j >= S) { fit = false; break; }
          if ((int)heights_[i + j] > v) { fit = false; break; }
        }
        if (fit) { lowest = v; at = i; }
      }
    }
    if (lowest + ih > S) {
      if (S >= 16384) throw Error(FDH_ERR_ATLAS_FULL, "atlas full at 16384^2");
      alloc(S * 2, s);  // grow(): resetImageAtlas(atlasSize * 2) drops every entry (glcontext.nim:536-539)
      continue;
    }
    for (int j = at; j < at + iw; j++) heights_[j] = (uint16_t)(lowest + ih + M * 2);
    const int x = at + M, y = lowest + M;
    AtlasEntry& e = entries_[key] = AtlasEntry{x, y, w, h, false, {}, {}};
    epoch_++;
    if (out_rect) { out_rect[0] = x; out_rect[1] = y; out_rect[2] = w; out_rect[3] = h; }
    return e;
  }
}
void Atlas::upload_rect(int level, int x, int y, int w, int h, const uint8_t* rgba) {
  const int LS = size_ >> level;
  if (x < 0 || y < 0 || x + w > LS || y + h > LS || w <= 0 || h <= 0 || !device_) return;
  FDH_HIP(hipMemcpy2D(levels_[level] + (size_t)y * LS + x, (size_t)LS * 4, rgba, (size_t)w * 4, (size_t)w * 4, h,
                      hipMemcpyHostToDevice));  // synchronous: image uploads are rare and the source is pageable
}
// pixie's Image.minifyBy2 on premultiplied RGBA8 (the arithmetic the reference's data/img1.flippy pins: its stored levels are this
// chain): box SUM div 4; an odd extent rounds the result size up, the extra column / row holding mix(a, b, 0.5) * 0.5 of the last
// source column / row (mix = (127 a + 128 b) div 255, * 0.5 = (128 v) div 255) and the extra corner the last texel * 0.25 =
// (64 v) div 255.  k_minify2 is the device form of the same step.
static void minify_by2_host(const uint8_t* src, int w, int h, uint8_t* dst) {
  const int nw = (w + 1) / 2, nh = (h + 1) / 2;
  auto at = [&](int x, int y, int k) -> unsigned { return src[((size_t)y * w + x) * 4 + k]; };
  for (int y = 0; y < nh; y++) {
    const bool row_pair = 2 * y + 1 < h;
    for (int x = 0; x < nw; x++) {
      const bool col_pair = 2 * x + 1 < w;
      for (int k = 0; k < 4; k++) {
        unsigned v;
        if (col_pair && row_pair) v = (at(2 * x, 2 * y, k) + at(2 * x + 1, 2 * y, k) + at(2 * x + 1, 2 * y + 1, k) + at(2 * x, 2 * y + 1, k)) >> 2;
        else if (row_pair) v = ((at(w - 1, 2 * y, k) * 127u + at(w - 1, 2 * y + 1, k) * 128u) / 255u) * 128u / 255u;
        else if (col_pair) v = ((at(2 * x, h - 1, k) * 127u + at(2 * x + 1, h - 1, k) * 128u) / 255u) * 128u / 255u;
        else v = at(w - 1, h - 1, k) * 64u / 255u;
        dst[((size_t)y * nw + x) * 4 + k] = (uint8_t)v;
      }
    }
  }
}
void Atlas::put_levels(int x, int y, int w, int h, const uint8_t* rgba) {  // the level chain by repeated minifyBy2
  std::vector<uint8_t> cur(rgba, rgba + (size_t)w * h * 4), nxt;
  each_level(x, y, w, h, [&](int level, int lx, int ly, int cw, int ch) {
    upload_rect(level, lx, ly, cw, ch, cur.data());
    nxt.assign((size_t)((cw + 1) / 2) * ((ch + 1) / 2) * 4, 0);
    minify_by2_host(cur.data(), cw, ch, nxt.data());
    cur.swap(nxt);
  });
}
// the ink boxes of an image whose texels the host holds (AtlasEntry): one pass, sixteen running boxes
static void measure_ink(AtlasEntry& e, const uint8_t* rgba) {
  // Glyph- and icon-sized images only (a 48 x 48 MSDF cell, a 20 px glyph): that is where a draw covers a fraction of its quad, and
  // the pass stays in the microseconds.  A photograph is opaque to its edges and would cost a pass over megapixels for nothing.
  e.has_ink = false;
  if (e.w > 128 || e.h > 128) return;
  for (int k = 0; k < kInkLevels; k++) e.ink_a[k] = e.ink_rgb[k] = InkBox{32767, 32767, 0, 0};
  auto grow = [](InkBox& b, int x, int y) {
    b.x0 = (int16_t)std::min<int>(b.x0, x); b.y0 = (int16_t)std::min<int>(b.y0, y);
    b.x1 = (int16_t)std::max<int>(b.x1, x + 1); b.y1 = (int16_t)std::max<int>(b.y1, y + 1);
  };
  for (int y = 0; y < e.h; y++) {
    const uint8_t* row = rgba + (size_t)y * e.w * 4;
    for (int x = 0; x < e.w; x++) {
      const int a = row[4 * x + 3], m = std::max<int>(row[4 * x], std::max<int>(row[4 * x + 1], row[4 * x + 2]));
      // levels the value exceeds: t = 0, 16, .. below it.  The boxes are nested (level k's holds level k + 1's): a texel inside
      // the highest one it counts for is inside them all.
      const int la = std::min((a + 15) >> 4, kInkLevels), lm = std::min((m + 15) >> 4, kInkLevels);
      auto inside = [&](const InkBox& b) { return x >= b.x0 && x < b.x1 && y >= b.y0 && y < b.y1; };
      if (la > 0 && !inside(e.ink_a[la - 1])) for (int k = 0; k < la; k++) grow(e.ink_a[k], x, y);
      if (lm > 0 && !inside(e.ink_rgb[lm - 1])) for (int k = 0; k < lm; k++) grow(e.ink_rgb[k], x, y);
    }
  }
  for (int k = 0; k < kInkLevels; k++) {  // nothing above the level: an empty box at the origin
    if (e.ink_a[k].x1 <= e.ink_a[k].x0) e.ink_a[k] = InkBox{0, 0, 0, 0};
    if (e.ink_rgb[k].x1 <= e.ink_rgb[k].x0) e.ink_rgb[k] = InkBox{0, 0, 0, 0};
  }
  e.has_ink = true;
}
void Atlas::put_image(hipStream_t s, int64_t key, int w, int h, const uint8_t* rgba, int out_rect[4]) {
  if (w <= 0 || h <= 0 || !rgba) throw Error(FDH_ERR_INVALID, "put_image: empty image");
  AtlasEntry& e = place(s, key, w, h, out_rect);
  measure_ink(e, rgba);
  put_levels(e.x, e.y, w, h, rgba);
}
// A rasterised glyph on its way into the atlas, processed on the device: optional LCD filter (applyLcdFilter, common/
// textrasters/pixie_raster.nim:12-43, what renderPixieGlyph does between fillText and loadGlyphImage :83-91), then the
// level chain of updateSubImage (textures.nim:106-119) -- every step a kernel on the context's stream.
void Atlas::put_glyph_image(hipStream_t s, int64_t key, int w, int h, const uint8_t* rgba, uint32_t flags, int out_rect[4]) {
  if (w <= 0 || h <= 0 || !rgba) throw Error(FDH_ERR_INVALID, "put_glyph_image: empty image");
  if (flags & ~(uint32_t)(FDH_GLYPH_LCD_FILTER | FDH_GLYPH_LCD_CONTEXT)) throw Error(FDH_ERR_INVALID, "put_glyph_image: unknown flag");
  const size_t n = (size_t)w * h;
  if (device_) { glyph_a_.reserve(n); glyph_b_.reserve(n); }
  const AtlasEntry& e = place(s, key, w, h, out_rect);
  if (!device_) return;
  FDH_HIP(hipMemcpyAsync(glyph_a_.ptr, rgba, n * 4, hipMemcpyHostToDevice, s));
  glyph_to_atlas(s, glyph_a_.ptr, glyph_b_.ptr, w, h, e.x, e.y, flags);
}
// device image -> (LCD filter) -> atlas level chain, all on the context's stream; waits for it (the caller's buffers are free after)
void Atlas::glyph_to_atlas(hipStream_t s, uint32_t* cur, uint32_t* nxt, int w, int h, int x, int y, uint32_t flags) {
  if (flags & FDH_GLYPH_LCD_FILTER) { launch_lcd_filter(s, cur, nxt, w, h); std::swap(cur, nxt); }
  each_level(x, y, w, h, [&](int level, int lx, int ly, int cw, int ch) {
    launch_atlas_blit(s, levels_[level], size_ >> level, lx, ly, cur, cw, ch);
    launch_minify2(s, cur, nxt, cw, ch);
    std::swap(cur, nxt);
  });
  FDH_HIP(hipStreamSynchronize(s));
  FDH_HIP(hipGetLastError());
}

// generateGlyph's job (common/fontglyphs.nim:61-106) with an own rasteriser in pixie's place: a glyph OUTLINE (quadratic segments in
// pixel units of the w x h image, y down; cx = NaN marks a straight line) becomes coverage on the device and goes into the atlas.
// The curves are flattened here on the host (chord error <= 0.025 px; the same float formula as oracle/figdraw_oracle.c,
// fo_flatten_outline), the area accumulation runs in k_rasterize_lines.  pixie's texels are third-party and unpinned
// (SURVEY.md 8c): parity is defined against the oracle's restatement of the same published algorithm.
static int flatten_count(const float* q) {
  const float ddx = q[0] - 2.0f * q[2] + q[4], ddy = q[1] - 2.0f * q[3] + q[5];
  const float dev = std::sqrt(ddx * ddx + ddy * ddy);
  const int n = (int)std::ceil(std::sqrt(dev * 10.0f));  // error of n chords = dev / (4 n^2) <= 0.025 px
  return n < 1 ? 1 : (n > 64 ? 64 : n);
}
// the lines (x0, y0, x1, y1) of an outline's n segments, appended: the single put's and the coverage batch's
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
void Atlas::put_glyph_outline(hipStream_t s, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]) {
  if (w <= 0 || h <= 0 || w > 4096 || h > 4096) throw Error(FDH_ERR_INVALID, "put_glyph_outline: image size must be in 1..4096");
  if (n < 0 || (n > 0 && !segs)) throw Error(FDH_ERR_INVALID, "put_glyph_outline: bad outline");
  if (flags & ~(uint32_t)(FDH_GLYPH_LCD_FILTER | FDH_GLYPH_LCD_CONTEXT | FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT | FDH_GLYPH_MTSDF_OVERLAP | 0xFF00u)) throw Error(FDH_ERR_INVALID, "put_glyph_outline: unknown flag");
  const uint32_t sdf_range = (flags >> 8) & 255u;
  if (sdf_range && (!(flags & FDH_GLYPH_MTSDF) || sdf_range > 64u)) throw Error(FDH_ERR_INVALID, "put_glyph_outline: a distance range needs FDH_GLYPH_MTSDF and is at most 64");
  if ((flags & FDH_GLYPH_MTSDF_CORRECT) && !(flags & FDH_GLYPH_MTSDF)) throw Error(FDH_ERR_INVALID, "put_glyph_outline: FDH_GLYPH_MTSDF_CORRECT needs FDH_GLYPH_MTSDF");
  if ((flags & FDH_GLYPH_MTSDF_OVERLAP) && !(flags & FDH_GLYPH_MTSDF)) throw Error(FDH_ERR_INVALID, "put_glyph_outline: FDH_GLYPH_MTSDF_OVERLAP needs FDH_GLYPH_MTSDF");
  if (flags & FDH_GLYPH_MTSDF) {
    if (flags & (FDH_GLYPH_LCD_FILTER | FDH_GLYPH_LCD_CONTEXT)) throw Error(FDH_ERR_INVALID, "put_glyph_outline: a distance field takes no LCD filter");
    put_glyph_mtsdf(s, key, w, h, segs, n, sdf_range ? (float)sdf_range : 4.0f, (flags & FDH_GLYPH_MTSDF_CORRECT) != 0, (flags & FDH_GLYPH_MTSDF_OVERLAP) != 0, out_rect);
    return;
  }
  std::vector<float> lines;
  lines.reserve((size_t)n * 16);
  flatten_outline(segs, n, &lines);
  put_glyph_lines(s, key, w, h, lines, flags, out_rect);
}
// a coverage glyph from its flattened outline: packed, rasterised, filtered, its level chain built
void Atlas::put_glyph_lines(hipStream_t s, int64_t key, int w, int h, const std::vector<float>& lines, uint32_t flags, int out_rect[4]) {
  const size_t npx = (size_t)w * h, m = lines.size() / 4;
  if (device_) {
    glyph_a_.reserve(npx);
    glyph_b_.reserve(npx);
    glyph_lines_.reserve(std::max<size_t>(lines.size(), 4));
    glyph_acc_.reserve((size_t)h * (w + 2));
  }
  const AtlasEntry& e = place(s, key, w, h, out_rect);
  if (!device_) return;
  if (m) FDH_HIP(hipMemcpyAsync(glyph_lines_.ptr, lines.data(), lines.size() * sizeof(float), hipMemcpyHostToDevice, s));
  launch_rasterize_lines(s, reinterpret_cast<const float4*>(glyph_lines_.ptr), (int)m, w, h, glyph_acc_.ptr, glyph_a_.ptr);
  glyph_to_atlas(s, glyph_a_.ptr, glyph_b_.ptr, w, h, e.x, e.y, flags);  // (synchronises: `lines` stays alive until then)
}
// fdh_put_glyph_outline with FDH_GLYPH_MTSDF (the specification: include/figdraw_hip.h at that flag).  The host makes contours, the
// orientation and the coloured edges (fdh_msdf_host.h), the device the texels (k_msdf_generate): one copy, one launch, then the level
// chain every glyph image takes.  Nothing is premultiplied and nothing filtered: the four bytes of a texel are four distances.
// `correct` (FDH_GLYPH_MTSDF_CORRECT, step 5): one more launch on the same stream, k_msdf_correct from one glyph buffer into the other.
// `overlap` (FDH_GLYPH_MTSDF_OVERLAP, step 6): the same records and the same launches, by the kernels that combine the contours.
void Atlas::put_glyph_mtsdf(hipStream_t s, int64_t key, int w, int h, const float* segs, int n, float range, bool correct, bool overlap, int out_rect[4]) {
  if (n > msdf::kMaxSegments) throw Error(FDH_ERR_INVALID, "put_glyph_outline: a distance field takes at most 65535 segments");
  msdf::Shape shape;
  if (!msdf::build_shape(segs, n, &shape)) throw Error(FDH_ERR_INVALID, "put_glyph_outline: a distance field needs closed contours");
  std::vector<float> rec;
  if (device_) {
    msdf::edge_records(shape, &rec);
    const size_t npx = (size_t)w * h;
    glyph_a_.reserve(npx);
    glyph_b_.reserve(npx);
    glyph_edges_.reserve(std::max<size_t>(rec.size(), msdf::kEdgeFloats));
  }
  const AtlasEntry& e = place(s, key, w, h, out_rect);
  if (!device_) return;
  const int x = e.x, y = e.y;
  if (!rec.empty()) FDH_HIP(hipMemcpyAsync(glyph_edges_.ptr, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice, s));
  uint32_t *field = glyph_a_.ptr, *spare = glyph_b_.ptr;
  (overlap ? launch_msdf_generate_union : launch_msdf_generate)(s, glyph_edges_.ptr, (int)shape.edges.size(), w, h, (float)shape.orient, range, field);
  if (correct) {
    (overlap ? launch_msdf_correct_union : launch_msdf_correct)(s, glyph_edges_.ptr, (int)shape.edges.size(), w, h, (float)shape.orient, range, field, spare);
    std::swap(field, spare);
  }
  // The level chain (updateSubImage's, textures.nim:106-119) stores nothing of an image 1 texel wide or high, not even level 0.  A field is
  // sampled at level 0 alone, and these texels have no other home: such a field gets that level.
  if (w == 1 || h == 1) launch_atlas_blit(s, levels_[0], size_, x, y, field, w, h);
  glyph_to_atlas(s, field, spare, w, h, x, y, 0u);  // (synchronises: `rec` stays alive until then)
}
// fdh_put_glyph_outline_cubic (the specification: include_glyphs/figdraw_hip_cubic.h): put_glyph_outline for segments of 8 floats.  Without a cubic
// among them it IS that call, on the same segments in its format.  With one: coverage flattens the cubics on the host too and goes the
// coverage put's way; a distance field goes put_glyph_mtsdf's way with the records and the kernels that know cubics (fdh_msdf_cubic_host.h,
// k_msdf_cubic.hip).  Everything is validated before anything is packed.
void Atlas::put_glyph_outline_cubic(hipStream_t s, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]) {
  namespace mc = msdf::cubic;
  if (n < 0 || (n > 0 && !segs)) throw Error(FDH_ERR_INVALID, "put_glyph_outline_cubic: bad outline");
  if (!mc::holds_cubic(segs, n)) {
    std::vector<float> six;
    mc::to_quadratic_format(segs, n, &six);
    static const float none[6] = {};
    put_glyph_outline(s, key, w, h, n > 0 ? six.data() : none, n, flags, out_rect);
    return;
  }
  if (w <= 0 || h <= 0 || w > 4096 || h > 4096) throw Error(FDH_ERR_INVALID, "put_glyph_outline_cubic: image size must be in 1..4096");
  if (flags & ~(uint32_t)(FDH_GLYPH_LCD_FILTER | FDH_GLYPH_LCD_CONTEXT | FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT | FDH_GLYPH_MTSDF_OVERLAP | 0xFF00u)) throw Error(FDH_ERR_INVALID, "put_glyph_outline_cubic: unknown flag");
  const uint32_t sdf_range = (flags >> 8) & 255u;
  if (sdf_range && (!(flags & FDH_GLYPH_MTSDF) || sdf_range > 64u)) throw Error(FDH_ERR_INVALID, "put_glyph_outline_cubic: a distance range needs FDH_GLYPH_MTSDF and is at most 64");
  if ((flags & FDH_GLYPH_MTSDF_CORRECT) && !(flags & FDH_GLYPH_MTSDF)) throw Error(FDH_ERR_INVALID, "put_glyph_outline_cubic: FDH_GLYPH_MTSDF_CORRECT needs FDH_GLYPH_MTSDF");
  if (flags & FDH_GLYPH_MTSDF_OVERLAP) throw Error(FDH_ERR_INVALID, "put_glyph_outline_cubic: FDH_GLYPH_MTSDF_OVERLAP takes no cubic segment");
  const size_t npx = (size_t)w * h;
  if (!(flags & FDH_GLYPH_MTSDF)) {  // coverage: put_glyph_outline's path on the lines of this outline
    std::vector<float> lines;
    lines.reserve((size_t)n * 16);
    mc::flatten_outline(segs, n, &lines);
    put_glyph_lines(s, key, w, h, lines, flags, out_rect);
    return;
  }
  if (flags & (FDH_GLYPH_LCD_FILTER | FDH_GLYPH_LCD_CONTEXT)) throw Error(FDH_ERR_INVALID, "put_glyph_outline_cubic: a distance field takes no LCD filter");
  if (n > msdf::kMaxSegments) throw Error(FDH_ERR_INVALID, "put_glyph_outline_cubic: a distance field takes at most 65535 segments");
  const float range = sdf_range ? (float)sdf_range : 4.0f;
  mc::Shape shape;
  if (!mc::build_shape(segs, n, &shape)) throw Error(FDH_ERR_INVALID, "put_glyph_outline_cubic: a distance field needs closed contours");
  std::vector<float> rec;
  if (device_) {
    mc::edge_records(shape, &rec);
    glyph_a_.reserve(npx);
    glyph_b_.reserve(npx);
    glyph_edges_.reserve(std::max<size_t>(rec.size(), mc::kCubicEdgeFloats));
  }
  const AtlasEntry& e = place(s, key, w, h, out_rect);
  if (!device_) return;
  const int x = e.x, y = e.y;
  if (!rec.empty()) FDH_HIP(hipMemcpyAsync(glyph_edges_.ptr, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice, s));
  uint32_t *field = glyph_a_.ptr, *spare = glyph_b_.ptr;
  launch_msdf_generate_cubic(s, glyph_edges_.ptr, (int)shape.edges.size(), w, h, (float)shape.orient, range, field);
  if (flags & FDH_GLYPH_MTSDF_CORRECT) {
    launch_msdf_correct_cubic(s, glyph_edges_.ptr, (int)shape.edges.size(), w, h, (float)shape.orient, range, field, spare);
    std::swap(field, spare);
  }
  if (w == 1 || h == 1) launch_atlas_blit(s, levels_[0], size_, x, y, field, w, h);  // (as in put_glyph_mtsdf: such a field gets level 0)
  glyph_to_atlas(s, field, spare, w, h, x, y, 0u);  // (synchronises: `rec` stays alive until then)
}
// ---- what the two batch calls share (put_glyph_outlines and put_glyph_coverage_batch below)
constexpr size_t kBatchGlyphWords = sizeof(msdf::BatchGlyph) / 4;
static int level_size(int v, int l) { return (v + (1 << l) - 1) >> l; }
// The 8 x 8 tiles of a glyph.  `thin_tiles`: a glyph 1 texel wide or high has tiles too (a distance field: put_glyph_mtsdf stores its level 0);
// without it such a glyph has none and gets no texel from any launch (a coverage glyph: each_level stores nothing of it).
static size_t batch_tiles(const msdf::BatchGlyph& t, bool thin_tiles) {
  return thin_tiles || (t.w > 1 && t.h > 1) ? (size_t)((t.w + 7) / 8) * ((t.h + 7) / 8) : 0;
}
static size_t owner_bits(const msdf::BatchGlyph& t, int n_levels) {
  size_t bits = 0;
  for (int l = msdf::kOwnerLevel; l < n_levels && level_size(t.w, l) > 1 && level_size(t.h, l) > 1; l++) bits += (size_t)level_size(t.w, l) * level_size(t.h, l);
  return bits;
}
// the words of the tables of a whole batch, whatever atlas it ends in: what glyph_tab_ is reserved for before the first placement
size_t Atlas::batch_table_words(const std::vector<msdf::BatchGlyph>& tab, bool thin_tiles) {
  size_t all_tiles = 0, all_owner_words = 0;
  for (const msdf::BatchGlyph& t : tab) {
    all_tiles += batch_tiles(t, thin_tiles);
    all_owner_words += (owner_bits(t, kMaxMips) + 31) / 32;
  }
  return tab.size() * kBatchGlyphWords + all_tiles + all_owner_words + 1;
}
// Pass 2 of a batch: every glyph through place(), in order; tab[i] takes its place.  A placement that grows the atlas has dropped every entry
// before it: glyph i is then the first of the new atlas (*first).  *placed: the glyphs that got a place; the exception that ended the loop
// (FDH_ERR_ATLAS_FULL, or no memory for a larger atlas) is returned: the glyphs before that one get their texels, as after single calls.
std::exception_ptr Atlas::place_batch(hipStream_t s, const FdhGlyphOutline* glyphs, int n, int (*out_rects)[4], std::vector<msdf::BatchGlyph>& tab, int* first, int* placed) {
  std::exception_ptr failed;
  int f = 0, p = 0;
  for (; p < n; p++) {
    const int before = size_;
    try {
      const AtlasEntry& e = place(s, glyphs[p].key, glyphs[p].width, glyphs[p].height, out_rects ? out_rects[p] : nullptr);
      tab[(size_t)p].x = e.x; tab[(size_t)p].y = e.y;
    } catch (...) {
      failed = std::current_exception();
    }
    if (size_ != before) f = p;
    if (failed) break;
  }
  *first = f; *placed = p;
  return failed;
}
// The tables of glyphs first .. first + m - 1 as the batched kernels read them: the glyph records (their offsets filled in here, edge_off
// made relative to the first glyph's), one word per tile naming its glyph, and the owner bits: level after level from msdf::kOwnerLevel
// on, the rectangles painted in put order into a map of the box they span.
void Atlas::batch_tables(std::vector<msdf::BatchGlyph>& tab, int first, int m, bool thin_tiles, BatchTables* T) const {
  const uint32_t edge_base = tab[(size_t)first].edge_off;
  uint32_t field_off = 0, n_tiles = 0, owner_words = 0, n_edges = 0;
  for (int k = 0; k < m; k++) {
    msdf::BatchGlyph& t = tab[(size_t)(first + k)];
    t.edge_off -= edge_base; t.field_off = field_off; t.first_tile = n_tiles; t.owner_off = owner_words * 32u;
    field_off += (uint32_t)(t.w * t.h);
    n_tiles += (uint32_t)batch_tiles(t, thin_tiles);
    n_edges += (uint32_t)t.n_edges;
    owner_words += (uint32_t)((owner_bits(t, n_levels_) + 31) / 32);
  }
  std::vector<uint32_t>& words = T->words;
  words.assign((size_t)m * kBatchGlyphWords + n_tiles + owner_words + 1, 0u);
  std::memcpy(words.data(), &tab[(size_t)first], (size_t)m * sizeof(msdf::BatchGlyph));
  uint32_t* tile_glyph = words.data() + (size_t)m * kBatchGlyphWords;
  uint32_t* owner = tile_glyph + n_tiles;
  for (int k = 0; k < m; k++) {
    const msdf::BatchGlyph& t = tab[(size_t)(first + k)];
    const uint32_t end = k + 1 < m ? tab[(size_t)(first + k + 1)].first_tile : n_tiles;
    for (uint32_t j = t.first_tile; j < end; j++) tile_glyph[j] = (uint32_t)k;
  }
  std::vector<int32_t> map;
  for (int l = msdf::kOwnerLevel; l < n_levels_; l++) {
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = 0, by1 = 0;
    auto has_level = [&](const msdf::BatchGlyph& t) { return level_size(t.w, l) > 1 && level_size(t.h, l) > 1; };
    for (int k = 0; k < m; k++) {
      const msdf::BatchGlyph& t = tab[(size_t)(first + k)];
      if (!has_level(t)) continue;
      bx0 = std::min(bx0, t.x >> l); by0 = std::min(by0, t.y >> l);
      bx1 = std::max(bx1, (t.x >> l) + level_size(t.w, l)); by1 = std::max(by1, (t.y >> l) + level_size(t.h, l));
    }
    if (bx1 <= bx0) break;  // no glyph reaches this level, nor a deeper one
    const int bw = bx1 - bx0;
    map.assign((size_t)bw * (by1 - by0), -1);
    for (int k = 0; k < m; k++) {
      const msdf::BatchGlyph& t = tab[(size_t)(first + k)];
      if (!has_level(t)) continue;
      for (int j = 0; j < level_size(t.h, l); j++)
        for (int i = 0; i < level_size(t.w, l); i++) map[(size_t)((t.y >> l) + j - by0) * bw + ((t.x >> l) + i - bx0)] = k;
    }
    for (int k = 0; k < m; k++) {
      const msdf::BatchGlyph& t = tab[(size_t)(first + k)];
      if (!has_level(t)) continue;
      uint32_t bit = t.owner_off;
      for (int d = msdf::kOwnerLevel; d < l; d++) bit += (uint32_t)(level_size(t.w, d) * level_size(t.h, d));
      for (int j = 0; j < level_size(t.h, l); j++)
        for (int i = 0; i < level_size(t.w, l); i++, bit++)
          if (map[(size_t)((t.y >> l) + j - by0) * bw + ((t.x >> l) + i - bx0)] == k) owner[bit >> 5] |= 1u << (bit & 31u);
    }
  }
  T->n_tiles = n_tiles; T->n_edges = n_edges;
}
// The level chain of a batch whose tables (T, of m glyphs) are in glyph_tab_ and whose images are in `field`: one blit and one minify per
// level, whatever the glyphs' sizes -- the number of launches, which is returned, is the atlas's alone.
int Atlas::batch_level_chain(hipStream_t s, int m, const BatchTables& T, uint32_t* field, uint32_t* spare) {
  const msdf::BatchGlyph* d_glyphs = reinterpret_cast<const msdf::BatchGlyph*>(glyph_tab_.ptr);
  const uint32_t* d_tiles = glyph_tab_.ptr + (size_t)m * kBatchGlyphWords;
  const uint32_t* d_owner = d_tiles + T.n_tiles;
  int launches = 0;
  for (int l = 0; l < n_levels_; l++) {
    launch_atlas_blit_batch(s, levels_[l], size_ >> l, l, d_glyphs, d_tiles, (int)T.n_tiles, d_owner, field);
    launches++;
    if (l + 1 == n_levels_) break;  // (a single put minifies once more, into a buffer nobody reads)
    launch_minify2_batch(s, l, d_glyphs, d_tiles, (int)T.n_tiles, field, spare);
    std::swap(field, spare);
    launches++;
  }
  return launches;
}
// fdh_put_glyph_outlines (the specification: include_glyphs/figdraw_hip_glyphs.h).  What n calls of put_glyph_mtsdf do, in three passes: every glyph is
// validated and its shape built; every glyph is placed, in order, through place(); then the glyphs that are still in the atlas -- those
// placed since the last growth -- get their texels from a number of launches that does not depend on n: the generator over the tiles of
// all glyphs, the correction, and per atlas level one blit and one minify.
// Single puts overwrite one another where two rectangles meet in a deep level (msdf::kOwnerLevel); one launch has no order, so the host
// paints the rectangles of such a level in put order and gives every glyph the bits of the texels that are still its own.
void Atlas::put_glyph_outlines(hipStream_t s, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  // ---- pass 1: validation.  Nothing below this pass refuses a glyph.
  if (flags & ~(uint32_t)(FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT | FDH_GLYPH_MTSDF_OVERLAP | 0xFF00u))
    throw Error(FDH_ERR_INVALID, "put_glyph_outlines: unknown flag (coverage glyphs and the LCD flags are not batched)");
  if (!(flags & FDH_GLYPH_MTSDF)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: needs FDH_GLYPH_MTSDF");
  const uint32_t flag_range = (flags >> 8) & 255u;
  if (flag_range > 64u) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: a distance range is at most 64");
  if (n < 0 || (n > 0 && !glyphs)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: bad glyph array");
  if (n > 65535) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: at most 65535 glyphs");
  const bool correct = (flags & FDH_GLYPH_MTSDF_CORRECT) != 0, overlap = (flags & FDH_GLYPH_MTSDF_OVERLAP) != 0;
  int64_t texels = 0, segments = 0;
  for (int i = 0; i < n; i++) {
    const FdhGlyphOutline& g = glyphs[i];
    if (g.width <= 0 || g.height <= 0 || g.width > 4096 || g.height > 4096) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: image size must be in 1..4096");
    if (g.n_segs < 0 || (g.n_segs > 0 && !g.segs)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: bad outline");
    if (g.n_segs > msdf::kMaxSegments) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: a distance field takes at most 65535 segments");
    if (g.sdf_range > 64u) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: a distance range is at most 64");
    texels += (int64_t)g.width * g.height;
    segments += g.n_segs;
  }
  if (texels > ((int64_t)1 << 24)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: at most 2^24 texels in a batch");
  if (segments > ((int64_t)1 << 20)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: at most 2^20 segments in a batch");
  std::vector<float> rec, one;           // the records of all glyphs, glyph after glyph (a device context only)
  std::vector<msdf::BatchGlyph> tab((size_t)n);  // edge_off, n_edges, w, h, orient and the range now; the offsets and the place in pass 3
  {
    msdf::Shape shape;
    for (int i = 0; i < n; i++) {
      const FdhGlyphOutline& g = glyphs[i];
      if (!msdf::build_shape(g.segs, g.n_segs, &shape)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines: a distance field needs closed contours");
      const float range = g.sdf_range ? (float)g.sdf_range : (flag_range ? (float)flag_range : 4.0f);
      msdf::BatchGlyph& t = tab[(size_t)i];
      t = msdf::BatchGlyph{};
      t.edge_off = (uint32_t)(rec.size() / msdf::kEdgeFloats); t.n_edges = (int32_t)shape.edges.size();
      t.w = g.width; t.h = g.height;
      t.orient = (float)shape.orient; t.inv_range = 1.0f / range; t.step = range / 255.0f;
      if (device_) { msdf::edge_records(shape, &one); rec.insert(rec.end(), one.begin(), one.end()); }
    }
  }
  field_batch(s, glyphs, n, out_rects, tab, rec, msdf::kEdgeFloats, texels, correct, overlap ? FieldKernels::overlap : FieldKernels::plain);
}
// Passes 2 and 3 of a batch of distance fields, whose pass 1 (the caller's) left `tab` (edge_off in records of `stride` floats, n_edges, w, h,
// orient and the range) and `rec`, the records of all glyphs; `texels`: the sum of w * h.  put_glyph_outlines' and put_glyph_outlines_cubic's:
// the record stride and the two kernels are what differs.
void Atlas::field_batch(hipStream_t s, const FdhGlyphOutline* glyphs, int n, int (*out_rects)[4], std::vector<msdf::BatchGlyph>& tab, const std::vector<float>& rec,
                        size_t stride, int64_t texels, bool correct, FieldKernels kernels) {
  batch_stats_ = FdhGlyphBatchStats{};
  batch_stats_.glyphs = n;
  if (n == 0) return;
  // ---- the device buffers, for the whole batch (pass 3 takes a part of it), before any placement as every put does
  if (device_) {
    glyph_a_.reserve((size_t)texels);
    glyph_b_.reserve((size_t)texels);
    glyph_edges_.reserve(std::max<size_t>(rec.size(), stride));
    glyph_tab_.reserve(batch_table_words(tab, true));
  }
  // ---- pass 2: the places
  int first = 0, placed = 0;
  std::exception_ptr failed = place_batch(s, glyphs, n, out_rects, tab, &first, &placed);
  batch_stats_.written = placed - first;
  batch_stats_.dropped_by_growth = first;
  // ---- pass 3: the texels of glyphs first .. placed - 1
  if (device_ && placed > first) {
    const int m = placed - first;
    const uint32_t edge_base = tab[(size_t)first].edge_off;
    BatchTables T;
    batch_tables(tab, first, m, true, &T);
    const float* rec_first = rec.data() + (size_t)edge_base * stride;
    const size_t rec_floats = rec.size() - (size_t)edge_base * stride;
    if (rec_floats) FDH_HIP(hipMemcpyAsync(glyph_edges_.ptr, rec_first, rec_floats * sizeof(float), hipMemcpyHostToDevice, s));
    FDH_HIP(hipMemcpyAsync(glyph_tab_.ptr, T.words.data(), T.words.size() * 4, hipMemcpyHostToDevice, s));
    const msdf::BatchGlyph* d_glyphs = reinterpret_cast<const msdf::BatchGlyph*>(glyph_tab_.ptr);
    const uint32_t* d_tiles = glyph_tab_.ptr + (size_t)m * kBatchGlyphWords;
    uint32_t *field = glyph_a_.ptr, *spare = glyph_b_.ptr;
    const bool overlap = kernels == FieldKernels::overlap;
    int launches = 1;
    if (kernels == FieldKernels::cubic) launch_msdf_generate_cubic_batch(s, glyph_edges_.ptr, d_glyphs, d_tiles, (int)T.n_tiles, field);
    else launch_msdf_generate_batch(s, overlap, glyph_edges_.ptr, d_glyphs, d_tiles, (int)T.n_tiles, field);
    if (correct) {
      if (kernels == FieldKernels::cubic) launch_msdf_correct_cubic_batch(s, glyph_edges_.ptr, d_glyphs, d_tiles, (int)T.n_tiles, field, spare);
      else launch_msdf_correct_batch(s, overlap, glyph_edges_.ptr, d_glyphs, d_tiles, (int)T.n_tiles, field, spare);
      std::swap(field, spare);
      launches++;
    }
    launches += batch_level_chain(s, m, T, field, spare);
    FDH_HIP(hipStreamSynchronize(s));  // (`rec` and `T` stay alive until here)
    FDH_HIP(hipGetLastError());
    batch_stats_.tiles = (int32_t)T.n_tiles;
    batch_stats_.edges = (int32_t)T.n_edges;
    batch_stats_.launches = launches;
    batch_stats_.bytes_copied = (int64_t)(rec_floats * sizeof(float) + T.words.size() * 4);
  }
  if (failed) std::rethrow_exception(failed);
}
// fdh_put_glyph_outlines_cubic (the specification: include_glyphs/figdraw_hip_cubic_batch.h): put_glyph_outlines for segments of 8 floats.  Without a
// cubic in any glyph it IS that call, on six-float copies of the segments.  With one, every glyph -- those without a cubic too -- goes the cubic
// call's way: mc::build_shape, records of mc::kCubicEdgeFloats floats, and the batched kernels of k_msdf_cubic.hip, in which a line or a
// quadratic runs k_msdf.hip's expressions: such a glyph gets the bytes its single call (put_glyph_mtsdf) gives it.
void Atlas::put_glyph_outlines_cubic(hipStream_t s, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  namespace mc = msdf::cubic;
  // ---- pass 1: validation.  Nothing below this pass refuses a glyph.
  if (flags & ~(uint32_t)(FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT | FDH_GLYPH_MTSDF_OVERLAP | 0xFF00u))
    throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: unknown flag (coverage glyphs are fdh_put_glyph_coverage_batch_cubic's)");
  if (!(flags & FDH_GLYPH_MTSDF)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: needs FDH_GLYPH_MTSDF");
  const uint32_t flag_range = (flags >> 8) & 255u;
  if (flag_range > 64u) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: a distance range is at most 64");
  if (n < 0 || (n > 0 && !glyphs)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: bad glyph array");
  if (n > 65535) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: at most 65535 glyphs");
  int64_t texels = 0, segments = 0;
  bool any_cubic = false;
  for (int i = 0; i < n; i++) {
    const FdhGlyphOutline& g = glyphs[i];
    if (g.width <= 0 || g.height <= 0 || g.width > 4096 || g.height > 4096) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: image size must be in 1..4096");
    if (g.n_segs < 0 || (g.n_segs > 0 && !g.segs)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: bad outline");
    if (g.n_segs > msdf::kMaxSegments) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: a distance field takes at most 65535 segments");
    if (g.sdf_range > 64u) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: a distance range is at most 64");
    texels += (int64_t)g.width * g.height;
    segments += g.n_segs;
    any_cubic = any_cubic || mc::holds_cubic(g.segs, g.n_segs);
  }
  if (texels > ((int64_t)1 << 24)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: at most 2^24 texels in a batch");
  if (segments > ((int64_t)1 << 20)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: at most 2^20 segments in a batch");
  if (!any_cubic) {  // the six-float batch, on copies
    std::vector<std::vector<float>> six((size_t)n);
    std::vector<FdhGlyphOutline> plain(glyphs, glyphs + n);
    for (int i = 0; i < n; i++) {
      mc::to_quadratic_format(glyphs[i].segs, glyphs[i].n_segs, &six[(size_t)i]);
      plain[(size_t)i].segs = six[(size_t)i].data();
    }
    put_glyph_outlines(s, plain.data(), n, flags, out_rects);
    return;
  }
  if (flags & FDH_GLYPH_MTSDF_OVERLAP) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: FDH_GLYPH_MTSDF_OVERLAP takes no cubic segment");
  std::vector<float> rec, one;                   // the records of all glyphs, glyph after glyph (a device context only)
  std::vector<msdf::BatchGlyph> tab((size_t)n);  // edge_off (in records of mc::kCubicEdgeFloats floats), n_edges, w, h, orient and the range now
  {
    mc::Shape shape;
    for (int i = 0; i < n; i++) {
      const FdhGlyphOutline& g = glyphs[i];
      if (!mc::build_shape(g.segs, g.n_segs, &shape)) throw Error(FDH_ERR_INVALID, "put_glyph_outlines_cubic: a distance field needs closed contours");
      const float range = g.sdf_range ? (float)g.sdf_range : (flag_range ? (float)flag_range : 4.0f);
      msdf::BatchGlyph& t = tab[(size_t)i];
      t = msdf::BatchGlyph{};
      t.edge_off = (uint32_t)(rec.size() / mc::kCubicEdgeFloats); t.n_edges = (int32_t)shape.edges.size();
      t.w = g.width; t.h = g.height;
      t.orient = (float)shape.orient; t.inv_range = 1.0f / range; t.step = range / 255.0f;
      if (device_) { mc::edge_records(shape, &one); rec.insert(rec.end(), one.begin(), one.end()); }
    }
  }
  field_batch(s, glyphs, n, out_rects, tab, rec, mc::kCubicEdgeFloats, texels, (flags & FDH_GLYPH_MTSDF_CORRECT) != 0, FieldKernels::cubic);
}
// the two segment formats of a coverage batch: the floats of a segment, its line count, and the flattening of an outline
struct Atlas::OutlineFormat {
  const char* who;          // the call's name in its error messages
  const char* fields_call;  // the batch that takes distance fields of this format: what a refused flag points to
  int floats;
  int (*lines_of)(const float* seg);
  void (*flatten)(const float* segs, int n, std::vector<float>* lines);
};
// fdh_put_glyph_coverage_batch: coverage_batch below on segments of 6 floats
void Atlas::put_glyph_coverage_batch(hipStream_t s, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  static const OutlineFormat six = {"put_glyph_coverage_batch", "fdh_put_glyph_outlines'", 6, [](const float* q) { return q[2] != q[2] ? 1 : flatten_count(q); }, flatten_outline};
  coverage_batch(s, six, glyphs, n, flags, out_rects);
}
// fdh_put_glyph_coverage_batch_cubic (the specification: include_glyphs/figdraw_hip_cubic_batch.h): the same passes and the same launches on the lines
// the single cubic call makes of each outline (msdf::cubic::flatten_outline)
void Atlas::put_glyph_coverage_batch_cubic(hipStream_t s, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  static const OutlineFormat eight = {"put_glyph_coverage_batch_cubic", "fdh_put_glyph_outlines_cubic's", 8,
                                      [](const float* q) {
                                        if (q[2] != q[2]) return 1;
                                        if (q[4] == q[4]) return msdf::cubic::cubic_flatten_count(q);
                                        const float six[6] = {q[0], q[1], q[2], q[3], q[6], q[7]};
                                        return flatten_count(six);
                                      },
                                      msdf::cubic::flatten_outline};
  coverage_batch(s, eight, glyphs, n, flags, out_rects);
}
// The coverage batch in either format (the specifications: include_glyphs/figdraw_hip_coverage.h and figdraw_hip_cubic_batch.h).  What n coverage calls of put_glyph_outline do, in the three
// passes of put_glyph_outlines: every glyph validated and its outline flattened into one array of lines; every glyph placed, in order; then
// the glyphs still in the atlas get their texels: two launches make the coverage of all of them (k_coverage_cells_batch, k_coverage_sum_batch),
// one filters it (k_lcd_filter_batch), and every atlas level takes one blit and one minify.  A glyph 1 texel wide or high is placed
// and has no tiles: a single put stores nothing of it.
void Atlas::coverage_batch(hipStream_t s, const OutlineFormat& fmt, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) {
  auto bad = [&fmt](const std::string& what) { return Error(FDH_ERR_INVALID, std::string(fmt.who) + ": " + what); };
  // ---- pass 1: validation.  Nothing below this pass refuses a glyph.  (FDH_GLYPH_LCD_CONTEXT is resolved by the context.)
  if (flags & ~(uint32_t)(FDH_GLYPH_LCD_FILTER | FDH_GLYPH_LCD_CONTEXT))
    throw bad(std::string("the LCD flags only (distance fields are ") + fmt.fields_call + ")");
  if (n < 0 || (n > 0 && !glyphs)) throw bad("bad glyph array");
  if (n > 65535) throw bad("at most 65535 glyphs");
  std::vector<msdf::BatchGlyph> tab((size_t)n);  // edge_off, n_edges: the glyph's first line and its line count; orient, inv_range, step: unused
  int64_t texels = 0, segments = 0, n_lines = 0;
  for (int i = 0; i < n; i++) {
    const FdhGlyphOutline& g = glyphs[i];
    if (g.width <= 0 || g.height <= 0 || g.width > 4096 || g.height > 4096) throw bad("image size must be in 1..4096");
    if (g.n_segs < 0 || (g.n_segs > 0 && !g.segs)) throw bad("bad outline");
    if (g.sdf_range) throw bad("a coverage glyph has no distance range");
    texels += (int64_t)g.width * g.height;
    segments += g.n_segs;
    if (segments > ((int64_t)1 << 20)) throw bad("at most 2^20 segments in a batch");
    msdf::BatchGlyph& t = tab[(size_t)i];
    t = msdf::BatchGlyph{};
    t.w = g.width; t.h = g.height;
    t.edge_off = (uint32_t)n_lines;
    for (int k = 0; k < g.n_segs; k++) t.n_edges += fmt.lines_of(g.segs + (size_t)fmt.floats * k);
    n_lines += t.n_edges;
  }
  if (texels > ((int64_t)1 << 24)) throw bad("at most 2^24 texels in a batch");
  if (n_lines > ((int64_t)1 << 22)) throw bad("at most 2^22 flattened lines in a batch");
  std::vector<float> lines;  // of all glyphs, glyph after glyph (a device context only)
  if (device_) {
    lines.reserve((size_t)n_lines * 4);
    for (int i = 0; i < n; i++) fmt.flatten(glyphs[i].segs, glyphs[i].n_segs, &lines);
  }
  coverage_stats_ = FdhGlyphBatchStats{};
  coverage_stats_.glyphs = n;
  if (n == 0) return;
  // ---- the device buffers, for the whole batch, before any placement as every put does
  if (device_) {
    glyph_a_.reserve((size_t)texels);
    glyph_b_.reserve((size_t)texels);
    glyph_lines_.reserve(std::max<size_t>(lines.size(), 4));
    glyph_tab_.reserve(batch_table_words(tab, false));
  }
  // ---- pass 2: the places
  int first = 0, placed = 0;
  std::exception_ptr failed = place_batch(s, glyphs, n, out_rects, tab, &first, &placed);
  coverage_stats_.written = placed - first;
  coverage_stats_.dropped_by_growth = first;
  // ---- pass 3: the texels of glyphs first .. placed - 1
  if (device_ && placed > first) {
    const int m = placed - first;
    const size_t line_base = (size_t)tab[(size_t)first].edge_off * 4;
    BatchTables T;
    batch_tables(tab, first, m, false, &T);
    const size_t line_floats = (size_t)T.n_edges * 4;
    if (line_floats) FDH_HIP(hipMemcpyAsync(glyph_lines_.ptr, lines.data() + line_base, line_floats * sizeof(float), hipMemcpyHostToDevice, s));
    FDH_HIP(hipMemcpyAsync(glyph_tab_.ptr, T.words.data(), T.words.size() * 4, hipMemcpyHostToDevice, s));
    const msdf::BatchGlyph* d_glyphs = reinterpret_cast<const msdf::BatchGlyph*>(glyph_tab_.ptr);
    const uint32_t* d_tiles = glyph_tab_.ptr + (size_t)m * kBatchGlyphWords;
    uint32_t *field = glyph_a_.ptr, *spare = glyph_b_.ptr;
    int launches = 0;
    if (T.n_tiles) {
      launch_coverage_batch(s, reinterpret_cast<const float4*>(glyph_lines_.ptr), d_glyphs, d_tiles, (int)T.n_tiles, reinterpret_cast<float*>(spare), field);
      launches += 2;
      if (flags & FDH_GLYPH_LCD_FILTER) {
        launch_lcd_filter_batch(s, d_glyphs, d_tiles, (int)T.n_tiles, field, spare);
        std::swap(field, spare);
        launches++;
      }
      launches += batch_level_chain(s, m, T, field, spare);
    }
    FDH_HIP(hipStreamSynchronize(s));  // (`lines` and `T` stay alive until here)
    FDH_HIP(hipGetLastError());
    coverage_stats_.tiles = (int32_t)T.n_tiles;
    coverage_stats_.edges = (int32_t)T.n_edges;
    coverage_stats_.launches = launches;
    coverage_stats_.bytes_copied = (int64_t)(line_floats * sizeof(float) + T.words.size() * 4);
  }
  if (failed) std::rethrow_exception(failed);
}
// Flippy: figdraw's mip-mapped image container (common/formatflippy.nim:77-149).  Layout: "flip", u32 version (1), then per
// mip level "mip!", u32 width, u32 height, u32 zlen, and a raw-snappy block holding straight RGBA8.  The reference
// converts every texel to pixie's premultiplied ColorRGBX on load and uploads level l at (x >> l, y >> l)
// (putFlippy glcontext.nim:610-620) instead of rebuilding the chain with minifyBy2.
static std::vector<uint8_t> snappy_uncompress(const uint8_t* in, size_t n) {
  size_t i = 0, len = 0;
  for (int shift = 0;; shift += 7) {
    if (i >= n || shift > 35) throw Error(FDH_ERR_INVALID, "flippy: bad snappy length");
    const uint8_t c = in[i++];
    len |= (size_t)(c & 0x7f) << shift;
    if (c < 0x80) break;
  }
  std::vector<uint8_t> out;
  out.reserve(len);
  auto need = [&](size_t k) { if (i + k > n) throw Error(FDH_ERR_INVALID, "flippy: truncated snappy block"); };
  while (i < n) {
    const uint8_t tag = in[i++];
    const int t = tag & 3;
    if (t == 0) {  // literal
      size_t l = tag >> 2;
      if (l < 60) l += 1;
      else {
        const int nb = (int)l - 59;
        need(nb);
        l = 0;
        for (int k = 0; k < nb; k++) l |= (size_t)in[i + k] << (8 * k);
        l += 1;
        i += nb;
      }
      need(l);
      out.insert(out.end(), in + i, in + i + l);
      i += l;
    } else {  // copy with 1-, 2- or 4-byte offset
      size_t l, off;
      if (t == 1) { need(1); l = ((tag >> 2) & 7) + 4; off = ((size_t)(tag >> 5) << 8) | in[i]; i += 1; }
      else if (t == 2) { need(2); l = (tag >> 2) + 1; off = in[i] | ((size_t)in[i + 1] << 8); i += 2; }
      else { need(4); l = (tag >> 2) + 1; off = in[i] | ((size_t)in[i + 1] << 8) | ((size_t)in[i + 2] << 16) | ((size_t)in[i + 3] << 24); i += 4; }
      if (off == 0 || off > out.size()) throw Error(FDH_ERR_INVALID, "flippy: bad snappy copy offset");
      for (size_t k = 0; k < l; k++) out.push_back(out[out.size() - off]);
    }
  }
  if (out.size() != len) throw Error(FDH_ERR_INVALID, "flippy: snappy length mismatch");
  return out;
}
void Atlas::put_mips(hipStream_t s, int64_t key, int n, const int* ws, const int* hs, const uint8_t* const* premul_rgba, int out_rect[4]) {
  // putFlippy glcontext.nim:610-620: level l goes to (x >> l, y >> l) with the size the container stored for it
  if (n <= 0 || !ws || !hs || !premul_rgba) throw Error(FDH_ERR_INVALID, "put_mips: no mip levels");
  for (int l = 0; l < n; l++)
    if (ws[l] <= 0 || hs[l] <= 0 || !premul_rgba[l]) throw Error(FDH_ERR_INVALID, "put_mips: bad mip level");
  const AtlasEntry& e = place(s, key, ws[0], hs[0], out_rect);
  for (int l = 0; l < n && l < n_levels_; l++) upload_rect(l, e.x >> l, e.y >> l, ws[l], hs[l], premul_rgba[l]);
}
void Atlas::put_flippy(hipStream_t s, int64_t key, const uint8_t* data, size_t n, int out_rect[4]) {
  auto u32 = [&](size_t at) { return (uint32_t)data[at] | ((uint32_t)data[at + 1] << 8) | ((uint32_t)data[at + 2] << 16) | ((uint32_t)data[at + 3] << 24); };
  if (!data || n < 8 || std::memcmp(data, "flip", 4) != 0) throw Error(FDH_ERR_INVALID, "Invalid Flippy header");
  if (u32(4) != 1) throw Error(FDH_ERR_INVALID, "Invalid Flippy version");
  std::vector<std::vector<uint8_t>> mips;
  std::vector<int> ws, hs;
  size_t i = 8;
  while (i < n) {
    if (i + 16 > n || std::memcmp(data + i, "mip!", 4) != 0) throw Error(FDH_ERR_INVALID, "Invalid Flippy sub header");
    const int w = (int)u32(i + 4), h = (int)u32(i + 8);
    const size_t z = u32(i + 12);
    i += 16;
    if (i + z > n || w <= 0 || h <= 0) throw Error(FDH_ERR_INVALID, "Flippy read error");
    std::vector<uint8_t> px = snappy_uncompress(data + i, z);
    i += z;
    if (px.size() != (size_t)w * h * 4) throw Error(FDH_ERR_INVALID, "Flippy mip size mismatch");
    for (size_t k = 0; k < (size_t)w * h; k++) {  // ColorRGBA -> premultiplied ColorRGBX
      const unsigned a = px[4 * k + 3];
      px[4 * k + 0] = (uint8_t)((px[4 * k + 0] * a) / 255);
      px[4 * k + 1] = (uint8_t)((px[4 * k + 1] * a) / 255);
      px[4 * k + 2] = (uint8_t)((px[4 * k + 2] * a) / 255);
    }
    mips.push_back(std::move(px));
    ws.push_back(w);
    hs.push_back(h);
  }
  if (mips.empty()) throw Error(FDH_ERR_INVALID, "Flippy has no mip levels");
  std::vector<const uint8_t*> ptrs;
  for (auto& m : mips) ptrs.push_back(m.data());
  put_mips(s, key, (int)mips.size(), ws.data(), hs.data(), ptrs.data(), out_rect);
}
void Atlas::update_image(int64_t key, int w, int h, const uint8_t* rgba) {  // glcontext.nim:591-604
  auto it = entries_.find(key);
  if (it == entries_.end()) throw Error(FDH_ERR_INVALID, "update_image: unknown key");
  if (it->second.w != w || it->second.h != h) throw Error(FDH_ERR_INVALID, "update_image: size mismatch");
  if (!rgba) throw Error(FDH_ERR_INVALID, "update_image: null image");
  measure_ink(it->second, rgba);  // the new texels have bounds of their own (draws shrink to them: shrink_to_ink) ...
  epoch_++;                       // ... and records cached for retained scenes hold the old ones
  put_levels(it->second.x, it->second.y, w, h, rgba);
}

}  // namespace fdh
