// fdh_glyphs.h -- glyphs made on the device (fdh_glyphs.cpp): class GlyphMaker, one member of Context beside the atlas.  A glyph image, an
// outline (coverage or a distance field, segments of 6 or of 8 floats), a batch of outlines or a coverage image that becomes a distance
// field is validated, gets its scratch buffers and only then a place in the atlas (Atlas::place); its texels are made by kernels on the
// stream the context hands over with every call, the atlas's level chain included.  The maker is also the atlas's mover (fdh_compact_atlas):
// the batches' level chain remakes the moved entries.  It knows neither the context nor how the atlas packs.  Images and video frames from
// device memory are the Importer's (fdh_import.h).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include_glyphs/figdraw_hip_cubic_batch.h"  // the two cubic batches; and through it figdraw_hip_cubic.h (fdh_put_glyph_outline_cubic),
                                                            // figdraw_hip_coverage.h (the coverage batch), figdraw_hip_glyphs.h (FdhGlyphOutline, FdhGlyphBatchStats)
#include "fdh_atlas.h"
#include "fdh_glyph_tables.h"  // BatchTables; and through it fdh_msdf_host.h (msdf::BatchGlyph)
#include "fdh_memory.h"        // DeviceBuf

namespace fdh {

class GlyphMaker final : public AtlasMover {
 public:
  // Every put validates, reserves the device buffers it needs and only then takes a place: one that throws before its texels are on their
  // way leaves no entry and no epoch bump behind.  Each waits for the stream once, at its end.  (`flags`: FDH_GLYPH_LCD_CONTEXT is resolved by the context.)
  void put_glyph_image(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const uint8_t* rgba, uint32_t flags, int out_rect[4]);
  void put_glyph_outline(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]);
  // fdh_put_glyph_outline_cubic (the specification: include_glyphs/figdraw_hip_cubic.h): put_glyph_outline for segments of 8 floats, cubics among them
  void put_glyph_outline_cubic(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]);
  // fdh_put_glyph_outlines (the specification: include_glyphs/figdraw_hip_glyphs.h): n distance fields, validated as a whole, placed in order, made in one go
  void put_glyph_outlines(hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);
  // fdh_put_glyph_outlines_cubic (the specification: include_glyphs/figdraw_hip_cubic_batch.h): put_glyph_outlines for segments of 8 floats
  void put_glyph_outlines_cubic(hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);
  const FdhGlyphBatchStats& glyph_batch_stats() const { return batch_stats_; }
  // fdh_put_glyph_coverage_batch (the specification: include_glyphs/figdraw_hip_coverage.h): n coverage glyphs, validated as a whole, placed in order, made in one go
  void put_glyph_coverage_batch(hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);
  // fdh_put_glyph_coverage_batch_cubic (the specification: include_glyphs/figdraw_hip_cubic_batch.h): put_glyph_coverage_batch for segments of 8 floats
  void put_glyph_coverage_batch_cubic(hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);
  const FdhGlyphBatchStats& glyph_coverage_batch_stats() const { return coverage_stats_; }
  // fdh_put_image_sdf and fdh_put_image_sdf_of (the specification: include_glyphs/figdraw_hip_image_sdf.h): the distance field of a coverage image
  // from the host, or of the texels an entry of the atlas holds
  void put_image_sdf(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const uint8_t* rgba, int channel, int pad, uint32_t flags, int out_rect[4]);
  void put_image_sdf_of(hipStream_t s, Atlas& atlas, int64_t src_key, int64_t key, int channel, int pad, uint32_t flags, int out_rect[4]);
  // fdh_compact_atlas (the specification: include_glyphs/figdraw_hip_atlas.h): the atlas's mover
  void move_entries(hipStream_t s, const AtlasView& from, const Atlas& to, const std::vector<MovedEntry>& moved, FdhAtlasMoveStats& stats) override;
  void release();  // the scratch buffers (the stream is idle)

 private:
  struct SegmentFormat;  // segments of 6 floats or of 8: fdh_glyphs.cpp, where the two instances are
  enum class FieldKernels { plain, overlap, cubic };
  struct Payload;        // what a batch copies to the device beside its tables: edge records or lines
  // the single puts: the call in either format, then a coverage glyph from its lines or a distance field from its outline
  void put_outline(const SegmentFormat& fmt, hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]);
  void put_lines(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const std::vector<float>& lines, uint32_t flags, int out_rect[4]);
  void put_field(const SegmentFormat& fmt, FieldKernels kernels, hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const float* segs, int n, float range, bool correct, int out_rect[4]);
  void glyph_to_atlas(hipStream_t s, const Atlas& atlas, uint32_t* cur, uint32_t* nxt, int w, int h, int x, int y, uint32_t flags);
  // the two image-field puts behind their validation: `rgba` from the host, or null and the w x h texels at (from_x, from_y) of the atlas's level 0
  void put_image_field(hipStream_t s, Atlas& atlas, int64_t key, int w, int h, const uint8_t* rgba, int from_x, int from_y, int channel, int pad, int range, int out_rect[4]);
  // the batches: pass 1 in either format, then passes 2 and 3 of all four (the placement, the tables, the copies, `middle`'s launches, the level chain)
  void put_fields(const SegmentFormat& fmt, hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);
  void put_coverage(const SegmentFormat& fmt, hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]);
  template <typename Middle>
  void place_and_make(hipStream_t s, Atlas& atlas, const FdhGlyphOutline* glyphs, int n, int (*out_rects)[4], std::vector<msdf::BatchGlyph>& tab, const Payload& payload,
                      int64_t texels, bool thin_tiles, FdhGlyphBatchStats& stats, Middle middle);
  int batch_level_chain(hipStream_t s, const Atlas& atlas, int m, const BatchTables& T, uint32_t* field, uint32_t* spare);

  DeviceBuf<uint32_t> glyph_a_, glyph_b_;  // the device glyph pipeline: the raster and its filtered / minified successors
  DeviceBuf<uint32_t> glyph_src_;          // the source texels of an image's distance field (put_image_field)
  DeviceBuf<float> glyph_lines_, glyph_acc_, glyph_edges_;  // flattened outline, area accumulators; the edge records of a distance field (fdh_msdf_host.h)
  DeviceBuf<uint32_t> glyph_tab_;  // the batches: the glyph records (msdf::BatchGlyph), the tile -> glyph words, the owner bits of the deep levels (fdh_glyph_tables.h)
  DeviceBuf<uint32_t> move_tab_;   // fdh_compact_atlas: the tables of its k_atlas_move launches (fdh_atlas_move.h)
  FdhGlyphBatchStats batch_stats_ = {}, coverage_stats_ = {};  // of the last put_glyph_outlines, of the last put_glyph_coverage_batch (either in either segment format)
};

}  // namespace fdh
