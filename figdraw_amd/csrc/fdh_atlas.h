// fdh_atlas.h -- the image atlas (fdh_atlas.cpp): the directory of entries, the skyline packer, the level chains in device memory and
// the scratch buffers of the device glyph pipeline: one member of Context.  The context quiesces its stream (a frame in flight may sample
// the atlas) and hands it over with every call; the atlas does not know the context.
#pragma once
#include <cstdint>
#include <exception>
#include <unordered_map>
#include <vector>

#include "../../include_glyphs/figdraw_hip_cubic_batch.h"  // the two cubic batches; and through it figdraw_hip_cubic.h (fdh_put_glyph_outline_cubic),
                                                            // figdraw_hip_coverage.h (the coverage batch), figdraw_hip_glyphs.h (FdhGlyphOutline, FdhGlyphBatchStats)
#include "fdh_memory.h"  // DeviceBuf
#include "fdh_types.h"   // AtlasView, kMaxMips

namespace fdh {
namespace msdf { struct BatchGlyph; }  // fdh_msdf_host.h: one glyph of a batch as the batched kernels read it

// An atlas entry and, when its level-0 texels were seen on the host (fdh_put_image), the bounds of what is IN it: for eight
// levels t = 0, 16, .. 112 the box (entry-relative texels, x1 / y1 exclusive) of texels whose alpha, and whose largest colour
// channel, exceeds t.  A draw whose coverage is exactly 0 wherever the sampled value is <= t (a glyph image: alpha 0; an MSDF
// image: distance below threshold - 0.5 / screen range) shrinks its pixel bounds to the image of that box: the strips outside
// would blend with alpha 0, which leaves every texel as it is (Recorder::shrink_to_ink).
constexpr int kInkLevels = 8;
struct InkBox { int16_t x0, y0, x1, y1; };
struct AtlasEntry {
  int x, y, w, h;
  bool has_ink = false;
  InkBox ink_a[kInkLevels], ink_rgb[kInkLevels];
};

class Atlas {
 public:
  // ---- directory and packer: no device needed (a record-only context has both)
  void init(int size, bool device, hipStream_t s);  // a context's first atlas; `device`: the levels exist (else only the directory and the packer)
  const AtlasEntry* find(int64_t key) const {       // (the walk pool's threads call this while they record)
    auto it = entries_.find(key);
    return it == entries_.end() ? nullptr : &it->second;
  }
  bool has(int64_t key) const { return entries_.count(key) != 0; }
  void remove(int64_t key) { entries_.erase(key); epoch_++; }
  int size() const { return size_; }
  int n_levels() const { return n_levels_; }
  // moves with every put, update, remove and reset: cached draw records of image nodes carry atlas positions (RetainedRoot::atlas_epoch)
  uint64_t epoch() const { return epoch_; }
  int64_t packed_area() const;
  void reset(int minimum_size, hipStream_t s);
  // ---- what the kernels sample, and level 0 for fdh_debug_read_surface
  AtlasView view() const;
  const uint32_t* level0() const { return levels_[0]; }
  // ---- texel work.  Every put validates, reserves the device buffers it needs and only then takes a place: one that throws before
  // its texels are on their way leaves no entry and no epoch bump behind.  (`flags`: FDH_GLYPH_LCD_CONTEXT is resolved by the context.)
  void put_image(hipStream_t s, int64_t key, int w, int h, const uint8_t* rgba, int out_rect[4]);
  void put_glyph_image(hipStream_t s, int64_t key, int w, int h, const uint8_t* rgba, uint32_t flags, int out_rect[4]);
  void put_glyph_outline(hipStream_t s, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]);
  // fdh_put_glyph_outline_cubic (the specification: include_glyphs/figdraw_hip_cubic.h): put_glyph_outline for segments of 8 floats, cubics among them
  void put_glyph_outline_cubic(hipStream_t s, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]);
  // fdh_put_glyph_outlines (the specification: include_glyphs/figdraw_hip_glyphs.h): n distance fields, validated as a whole, placed in order, made in one go
  void put_glyph_outlines(hipStream_t s, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);
  // fdh_put_glyph_outlines_cubic (the specification: include_glyphs/figdraw_hip_cubic_batch.h): put_glyph_outlines for segments of 8 floats
  void put_glyph_outlines_cubic(hipStream_t s, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);
  const FdhGlyphBatchStats& glyph_batch_stats() const { return batch_stats_; }
  // fdh_put_glyph_coverage_batch (the specification: include_glyphs/figdraw_hip_coverage.h): n coverage glyphs, validated as a whole, placed in order, made in one go
  void put_glyph_coverage_batch(hipStream_t s, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);
  // fdh_put_glyph_coverage_batch_cubic (the specification: include_glyphs/figdraw_hip_cubic_batch.h): put_glyph_coverage_batch for segments of 8 floats
  void put_glyph_coverage_batch_cubic(hipStream_t s, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);
  const FdhGlyphBatchStats& glyph_coverage_batch_stats() const { return coverage_stats_; }
  void put_mips(hipStream_t s, int64_t key, int n, const int* ws, const int* hs, const uint8_t* const* premul_rgba, int out_rect[4]);
  void put_flippy(hipStream_t s, int64_t key, const uint8_t* data, size_t n, int out_rect[4]);
  void update_image(int64_t key, int w, int h, const uint8_t* rgba);
  void release();  // the levels and the scratch buffers (the stream is idle)

 private:
  void alloc(int size, hipStream_t s);  // new levels first, then the old ones go and the empty atlas is committed
  void release_levels();
  AtlasEntry& place(hipStream_t s, int64_t key, int w, int h, int out_rect[4]);  // THE placement: rect (growing as needed), entry, epoch, out_rect
  // updateSubImage's level chain (textures.nim:106-119): step(level, x, y, w, h) for the image minified `level` times, while width > 1 and height > 1
  template <typename Step> void each_level(int x, int y, int w, int h, Step step) const {
    for (int level = 0; w > 1 && h > 1 && level < n_levels_; level++, x /= 2, y /= 2, w = (w + 1) / 2, h = (h + 1) / 2) step(level, x, y, w, h);
  }
  void upload_rect(int level, int x, int y, int w, int h, const uint8_t* rgba);
  void put_levels(int x, int y, int w, int h, const uint8_t* rgba);
  void glyph_to_atlas(hipStream_t s, uint32_t* cur, uint32_t* nxt, int w, int h, int x, int y, uint32_t flags);
  void put_glyph_lines(hipStream_t s, int64_t key, int w, int h, const std::vector<float>& lines, uint32_t flags, int out_rect[4]);
  void put_glyph_mtsdf(hipStream_t s, int64_t key, int w, int h, const float* segs, int n, float range, bool correct, bool overlap, int out_rect[4]);
  // what the two batch calls share (fdh_atlas.cpp): the size of the tables, the placement pass, the tables, the level chain
  struct BatchTables { std::vector<uint32_t> words; uint32_t n_tiles = 0, n_edges = 0; };  // words: glyph records, tile -> glyph, owner bits
  static size_t batch_table_words(const std::vector<msdf::BatchGlyph>& tab, bool thin_tiles);
  std::exception_ptr place_batch(hipStream_t s, const FdhGlyphOutline* glyphs, int n, int (*out_rects)[4], std::vector<msdf::BatchGlyph>& tab, int* first, int* placed);
  void batch_tables(std::vector<msdf::BatchGlyph>& tab, int first, int m, bool thin_tiles, BatchTables* T) const;
  int batch_level_chain(hipStream_t s, int m, const BatchTables& T, uint32_t* field, uint32_t* spare);
  // passes 2 and 3 of the two batches of distance fields (the record stride and the kernels differ); the coverage batch in its two segment formats
  enum class FieldKernels { plain, overlap, cubic };
  void field_batch(hipStream_t s, const FdhGlyphOutline* glyphs, int n, int (*out_rects)[4], std::vector<msdf::BatchGlyph>& tab, const std::vector<float>& rec, size_t stride,
                   int64_t texels, bool correct, FieldKernels kernels);
  struct OutlineFormat;
  void coverage_batch(hipStream_t s, const OutlineFormat& fmt, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);

  bool device_ = false;
  int size_ = 0, initial_size_ = 0, margin_ = 4, n_levels_ = 0;
  uint32_t* levels_[kMaxMips] = {};
  std::vector<uint16_t> heights_;  // the skyline
  std::unordered_map<int64_t, AtlasEntry> entries_;
  uint64_t epoch_ = 1;
  DeviceBuf<uint32_t> glyph_a_, glyph_b_;  // the device glyph pipeline: the raster and its filtered / minified successors
  DeviceBuf<float> glyph_lines_, glyph_acc_, glyph_edges_;  // flattened outline, area accumulators; the edge records of a distance field (fdh_msdf_host.h)
  DeviceBuf<uint32_t> glyph_tab_;  // put_glyph_outlines: the glyph records (msdf::BatchGlyph), the tile -> glyph words, the owner bits of the deep levels
  FdhGlyphBatchStats batch_stats_ = {}, coverage_stats_ = {};  // of the last put_glyph_outlines, of the last put_glyph_coverage_batch (either in either segment format)
};

}  // namespace fdh
