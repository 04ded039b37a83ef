// fdh_video_alpha.h -- the parameter blocks of k_video_alpha_import (k_video_alpha_import.hip), the kernel behind fdh_put_video_alpha and
// fdh_update_video_alpha, and of k_video_alpha_export (k_video_alpha_export.hip), the kernel behind fdh_read_video_alpha (the
// specification: include_video/figdraw_hip_video_alpha.h).  Plain C++, no HIP, no atlas and no context: GlyphMaker fills the first block
// (fdh_glyphs.cpp), fdh_video_out.cpp the second; tests/video_alpha_in_emu and tests/video_alpha_out_emu compile them as they stand, with
// the kernels beside them.  The coefficients are the siblings' tables (fdh_video_import.h, fdh_video_export.h): the NV12 row for an 8-bit
// format, the P010 row for A410.  The way in's tile, ink blocks and tail are k_image_import's (fdh_image_import.h).
#pragma once
#include <cstdint>

#include "fdh_image_import.h"

namespace fdh {
namespace video_alpha {

enum : uint32_t { kA420 = 11, kA444 = 12, kA410 = 13, kUYVA = 14 };  // FdhVideoAlphaPlanes::format, FdhVideoAlphaPlanesTarget::format
enum : uint32_t { kChromaLinear = 1, kStraightAlpha = 2 };           // ... ::flags
constexpr int kPlanes = 4, kAlpha = 3;                               // Y, Cb, Cr, A: the alpha plane is planes[3] in every format
constexpr bool known(uint32_t format) { return format >= kA420 && format <= kUYVA; }
constexpr bool ten_bit(uint32_t format) { return format == kA410; }
constexpr bool full_chroma(uint32_t format) { return format == kA444 || format == kA410; }  // 4:4:4: a chroma sample per texel
constexpr bool packed(uint32_t format) { return format == kUYVA; }                          // planes[0] is UYVY's four-byte groups
constexpr bool has_plane(uint32_t format, int p) { return !packed(format) || p == 0 || p == kAlpha; }
// the bytes of the unit that plane p's pointer and pitch are multiples of: a sample, or the UYVY plane's group
constexpr int element_bytes(uint32_t format, int p) { return packed(format) && p == 0 ? 4 : ten_bit(format) ? 2 : 1; }
// plane p of a w x h frame (or rectangle): a row's bytes, and the rows
constexpr int64_t row_bytes(uint32_t format, int p, int64_t w) {
  return packed(format) && p == 0 ? 4 * ((w + 1) / 2) : ((p == 1 || p == 2) && !full_chroma(format) ? (w + 1) / 2 : w) * element_bytes(format, p);
}
constexpr int64_t rows(uint32_t format, int p, int64_t h) { return (p == 1 || p == 2) && format == kA420 ? (h + 1) / 2 : h; }

// Both kernels: a lane takes a run of kRun texels of a row -- eight luma and eight alpha samples, the four (A420) or eight (A444, A410)
// samples of either chroma plane under them, or the four groups of the UYVY plane.
constexpr int kRun = 8;
// the bytes of plane p that go with a run: one wide access
constexpr int run_bytes(uint32_t format, int p) {
  return packed(format) && p == 0 ? 16 : ((p == 1 || p == 2) && !full_chroma(format) ? kRun / 2 : kRun) * element_bytes(format, p);
}

// ---- the way in.  A workgroup of kInGroup lanes per 32 x 32 tile of the image (image_import::kTile): four runs across, 32 rows down.
constexpr int kInGroup = 128;

struct InParams {
  const void* plane[kPlanes];  // Y, Cb, Cr, A as the device addresses them; UYVA: plane[0] (the groups) and plane[3] alone
  int64_t pitch[kPlanes];      // between rows of each plane, bytes
  int32_t w, h;                // of the luma and of the alpha plane
  int32_t cw, ch;              // of either chroma plane: ceil(w / 2) x ceil(h / 2) for A420, w x h for A444 / A410; UYVA: ceil(w / 2) groups x h
  uint32_t format;             // kA420 .. kUYVA: with the two flags, which build of k_video_alpha_import takes the launch
  uint32_t flags;
  int32_t wide[kPlanes];       // plane p and pitch[p] are multiples of run_bytes(format, p) and the row has a whole run: a run is one load
  int32_t yoff, coff, cy, crv, cgu, cgv, cbu;  // the conversion (a row of video_import::kCoefficients)
  int32_t x, y;                // the entry's place in level 0; level l's rectangle lies at (x >> l, y >> l)
  int32_t n_store;             // the levels of the chain that are stored: 0 .. n_store - 1 (Atlas::each_level; 0: nothing of the image is)
  int32_t ink;                 // measure the ink boxes: every tile leaves its block in ink_block
  int32_t lw[image_import::kTileLevels], lh[image_import::kTileLevels];  // the image's extent at levels 0 .. 5
  uint32_t* level[image_import::kLevels];                                // the atlas
  int32_t size;                                                          // ... of size x size texels at level 0
  uint32_t* scratch;           // takes the level-5 image, lw[5] x lh[5] texels, rows packed: a texel per tile (image_import::TailParams::src)
  int32_t* ink_block;          // image_import::kInkWords words per tile, as the device addresses them
};

// ---- the way out.  A workgroup of kOutGroup lanes per tile of the rectangle, 32 runs across.  A420 pairs rows (a chroma sample averages
// both): a lane takes its run in two rows, 8 row pairs down a 256 x 16 tile.  A444, A410 and UYVA pair none: a lane takes one row, 8 rows
// down a 256 x 8 tile.
constexpr int kOutGroup = 256, kOutTileW = 256;
constexpr int out_rows(uint32_t format) { return format == kA420 ? 2 : 1; }  // rows of a lane
constexpr int out_tile_h(uint32_t format) { return 8 * out_rows(format); }

struct OutParams {
  const uint32_t* src;         // texel (0, 0) of the rectangle in the frame surface, premultiplied RGBA8
  int64_t src_pitch;           // between rows of the surface, texels
  int32_t w, h;                // of the rectangle = of the luma and of the alpha plane
  void* plane[kPlanes];        // Y, Cb, Cr, A as the device addresses them; UYVA: plane[0] (the groups) and plane[3] alone
  int64_t pitch[kPlanes];      // between rows of each plane, bytes
  uint32_t format;             // kA420 .. kUYVA: with the two flags, which build of k_video_alpha_export takes the launch
  uint32_t flags;
  int32_t wide_src;            // src and src_pitch are multiples of 16 bytes and w >= 8: a whole run is two 16-byte loads
  int32_t wide[kPlanes];       // plane p and pitch[p] are multiples of run_bytes(format, p) and the row has a whole run: a run is one store
  int32_t yoff, coff;          // the conversion (a row of video_export::kCoefficients)
  int32_t ky[3], ku[3], kv[3];  // the rows of R, G, B
};

}  // namespace video_alpha
}  // namespace fdh
