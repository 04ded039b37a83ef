// fdh_atlas.cpp -- class Atlas (fdh_atlas.h), the image atlas: directory and skyline packer, level chains, the Flippy container.
#include "fdh_context.h"

#include <algorithm>
#include <chrono>
#include <cstring>
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
int Atlas::alloc_levels(int sz, hipStream_t s, uint32_t* fresh[kMaxMips]) const {
  int n = 0;
  std::fill(fresh, fresh + kMaxMips, nullptr);
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
    for (int l = 0; l < kMaxMips; l++) if (fresh[l]) (void)hipFree(fresh[l]);
    throw;
  }
  return n;
}
void Atlas::alloc(int size, hipStream_t s) {
  int sz = 1;
  while (sz < size) sz <<= 1;  // the samplers mask coordinates: keep the atlas a power of two
  uint32_t* fresh[kMaxMips] = {};
  const int n = alloc_levels(sz, s, fresh);
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
void Atlas::reset(int minimum_size, hipStream_t s) {
  int sz = initial_size_;
  while (sz < minimum_size) sz *= 2;  // plannedAtlasSize
  alloc(sz, s);
  rebuilds_++;
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
bool Atlas::skyline_place(std::vector<uint16_t>& heights, int S, int M, int w, int h, int* x, int* y) {
  const int iw = w + M * 2, ih = h + M * 2;
  int lowest = S, at = 0;
  for (int i = 0; i < S; i++) {
    int v = heights[i];
    if (v < lowest) {
      bool fit = true;
      for (int j = 0; j <= iw; j++) {
        if (i + j >= S) { fit = false; break; }
        if ((int)heights[i + j] > v) { fit = false; break; }
      }
      if (fit) { lowest = v; at = i; }
    }
  }
  if (lowest + ih > S) return false;
  for (int j = at; j < at + iw; j++) heights[j] = (uint16_t)(lowest + ih + M * 2);
  *x = at + M; *y = lowest + M;
  return true;
}
AtlasEntry& Atlas::place(hipStream_t s, int64_t key, int w, int h, int out_rect[4], Stored stored) {
  for (;;) {
    int x, y;
    if (!skyline_place(heights_, size_, margin_, w, h, &x, &y)) {
      if (size_ >= 16384) throw Error(FDH_ERR_ATLAS_FULL, "atlas full at 16384^2");
      alloc(size_ * 2, s);  // grow(): resetImageAtlas(atlasSize * 2) drops every entry (glcontext.nim:536-539)
      rebuilds_++;
      continue;
    }
    AtlasEntry& e = entries_[key] = AtlasEntry{x, y, w, h, false, {}, {}, stored, nullptr};
    epoch_++;
    if (out_rect) { out_rect[0] = x; out_rect[1] = y; out_rect[2] = w; out_rect[3] = h; }
    return e;
  }
}
// ------------------------------------------------------------------ compaction and keep mode (include_glyphs/figdraw_hip_atlas.h)
std::vector<const std::pair<const int64_t, AtlasEntry>*> Atlas::compaction_order() const {
  std::vector<const std::pair<const int64_t, AtlasEntry>*> order;
  order.reserve(entries_.size());
  for (const auto& kv : entries_) order.push_back(&kv);
  std::sort(order.begin(), order.end(), [](const auto* a, const auto* b) {
    if (a->second.h != b->second.h) return a->second.h > b->second.h;
    if (a->second.w != b->second.w) return a->second.w > b->second.w;
    return a->first < b->first;
  });
  return order;
}
void Atlas::compact(hipStream_t s, int size, FdhAtlasMoveStats* out) {
  if (size < 0 || size > 16384) throw Error(FDH_ERR_INVALID, "compact_atlas: size must be 0 (the current size) or in 1..16384");
  int sz = size_;
  if (size) for (sz = 1; sz < size;) sz <<= 1;
  // ---- the trial: every live entry on a scratch skyline, before anything changes
  using clock = std::chrono::steady_clock;
  auto us_since = [](clock::time_point t) { return (int32_t)std::chrono::duration_cast<std::chrono::microseconds>(clock::now() - t).count(); };
  const auto t_pack = clock::now();
  const auto order = compaction_order();
  std::vector<uint16_t> sky((size_t)sz, 0);
  std::unordered_map<int64_t, AtlasEntry> fresh_entries;
  fresh_entries.reserve(order.size());
  std::vector<MovedEntry> moved;
  moved.reserve(order.size());
  for (const auto* kv : order) {
    int x, y;
    if (!skyline_place(sky, sz, margin_, kv->second.w, kv->second.h, &x, &y))
      throw Error(FDH_ERR_ATLAS_FULL, "compact_atlas: the live entries do not fit an atlas of " + std::to_string(sz));
    AtlasEntry& e = fresh_entries[kv->first] = kv->second;
    e.x = x; e.y = y;
    moved.push_back(MovedEntry{&e, kv->second.x, kv->second.y});
  }
  FdhAtlasMoveStats st{};
  st.entries = (int32_t)order.size();
  st.size_before = size_; st.size_after = sz;
  st.packed_before = packed_area();
  st.us_pack = us_since(t_pack);
  // ---- the new levels first (a failed allocation leaves the old atlas whole), the texels, then the old levels go
  uint32_t* fresh[kMaxMips] = {};
  const auto t_alloc = clock::now();
  const int n = alloc_levels(sz, s, fresh);
  st.us_alloc = us_since(t_alloc);
  if (device_) {
    if (!mover_) throw Error(FDH_ERR_INVALID, "compact_atlas: no mover");
    const AtlasView from = view();
    uint32_t* old[kMaxMips];
    std::copy(levels_, levels_ + kMaxMips, old);
    const int old_size = size_, old_levels = n_levels_;
    std::copy(fresh, fresh + kMaxMips, levels_);
    size_ = sz; n_levels_ = n;
    try {
      mover_->move_entries(s, from, *this, moved, st);
    } catch (...) {  // the old atlas is still whole: it takes its place again
      release_levels();
      std::copy(old, old + kMaxMips, levels_);
      size_ = old_size; n_levels_ = old_levels;
      throw;
    }
    const auto t_free = clock::now();
    for (auto l : old) if (l) (void)hipFree(l);
    st.us_alloc += us_since(t_free);
  }
  size_ = sz; n_levels_ = n;
  heights_.swap(sky);
  entries_.swap(fresh_entries);  // (`moved` pointed into it: nothing reads that any more)
  epoch_++;
  compactions_++;
  st.packed_after = packed_area();
  if (out) *out = st;
}
void Atlas::make_room(hipStream_t s, const int (*wh)[2], int n) {
  if (!keep_ || n <= 0) return;
  int x, y;
  auto all_fit = [&](std::vector<uint16_t>& sky, int S) {
    for (int i = 0; i < n; i++) if (!skyline_place(sky, S, margin_, wh[i][0], wh[i][1], &x, &y)) return false;
    return true;
  };
  std::vector<uint16_t> sky = heights_;
  if (all_fit(sky, size_)) return;  // no placement of this call grows the atlas
  const auto order = compaction_order();
  int target = 16384;
  for (int S = size_; S <= 16384; S *= 2) {
    sky.assign((size_t)S, 0);
    bool fits = true;
    for (const auto* kv : order) if (!skyline_place(sky, S, margin_, kv->second.w, kv->second.h, &x, &y)) { fits = false; break; }
    if (fits && all_fit(sky, S)) { target = S; break; }
  }
  try {
    compact(s, target, nullptr);
  } catch (const Error& e) {
    if (e.code != FDH_ERR_ATLAS_FULL) throw;  // (not even the live entries fit 16384 in compaction order: the call goes on as without keep)
  }
}
void Atlas::usage(FdhAtlasUsage* out) const {
  *out = FdhAtlasUsage{};
  out->size = size_;
  out->entries = (int32_t)entries_.size();
  for (const auto& kv : entries_) out->used_area += (int64_t)kv.second.w * kv.second.h;
  out->packed_area = packed_area();
  out->epoch = epoch_;
  out->rebuilds = rebuilds_;
  out->compactions = compactions_;
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
  make_room(s, w, h);
  AtlasEntry& e = place(s, key, w, h, out_rect);
  measure_ink(e, rgba);
  put_levels(e.x, e.y, w, h, rgba);
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
  // what a move of the entry needs (Stored::levels): the sizes, and the texels of levels 1 .. as the caller gave them
  auto kept = std::make_shared<KeptLevels>();
  kept->n = std::min(n, (int)kMaxMips);
  for (int l = 0; l < kept->n; l++) {
    kept->w[l] = ws[l]; kept->h[l] = hs[l];
    if (l == 0 || !device_) continue;
    const size_t at = kept->texels.size(), texels = (size_t)ws[l] * hs[l];
    kept->texels.resize(at + texels);
    std::memcpy(kept->texels.data() + at, premul_rgba[l], texels * 4);
  }
  make_room(s, ws[0], hs[0]);
  AtlasEntry& e = place(s, key, ws[0], hs[0], out_rect, Stored::levels);
  e.kept = std::move(kept);
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
// The first half of every update (fdh_update_image, fdh_update_image_device): the entry of `key`, which must have this size; the epoch moves
// -- records cached for retained scenes hold the old texels' bounds --, and an entry of put_mips gives up its own levels for the chain
// that the caller stores next.  `also_refused`: what else the caller has against the call (or null), said behind the key and the size.
AtlasEntry& Atlas::begin_update(const char* who, int64_t key, int w, int h, const char* also_refused) {
  auto it = entries_.find(key);
  if (it == entries_.end()) throw Error(FDH_ERR_INVALID, std::string(who) + ": unknown key");
  if (it->second.w != w || it->second.h != h) throw Error(FDH_ERR_INVALID, std::string(who) + ": size mismatch");
  if (also_refused) throw Error(FDH_ERR_INVALID, std::string(who) + ": " + also_refused);
  epoch_++;
  if (it->second.stored == Stored::levels) {
    it->second.stored = Stored::chain;
    it->second.kept.reset();
  }
  return it->second;
}
void Atlas::update_image(int64_t key, int w, int h, const uint8_t* rgba) {  // glcontext.nim:591-604
  AtlasEntry& e = begin_update("update_image", key, w, h, rgba ? nullptr : "null image");
  measure_ink(e, rgba);  // the new texels have bounds of their own (draws shrink to them: shrink_to_ink)
  put_levels(e.x, e.y, w, h, rgba);
}

}  // namespace fdh
