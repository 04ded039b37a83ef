// fdh_video_422.h -- the parameter blocks of k_video_422_import (k_video_422_import.hip), the kernel behind fdh_put_video_422 and
// fdh_update_video_422, and of k_video_422_export (k_video_422_export.hip), the kernel behind fdh_read_video_422 (the specification:
// include_video/figdraw_hip_video_422.h).  Plain C++, no HIP, no atlas and no context: GlyphMaker fills the first block (fdh_glyphs.cpp),
// fdh_video_out.cpp the second; tests/video_422_in_emu and tests/video_422_out_emu compile them as they stand, with the kernels beside
// them.  The coefficients are the siblings' tables (fdh_video_import.h, fdh_video_export.h): the NV12 row for an 8-bit format, the P010
// row for I210.  The way in's tile, ink blocks and tail are k_image_import's (fdh_image_import.h).
#pragma once
#include <cstdint>

#include "fdh_image_import.h"

namespace fdh {
namespace video_422 {

enum : uint32_t { kI422 = 7, kI210 = 8, kYUY2 = 9, kUYVY = 10 };  // FdhVideoPlanes::format, FdhVideoPlanesTarget::format
enum : uint32_t { kChromaLinear = 1 };                            // ... ::flags
constexpr bool known(uint32_t format) { return format >= kI422 && format <= kUYVY; }
constexpr bool ten_bit(uint32_t format) { return format == kI210; }
constexpr bool packed(uint32_t format) { return format == kYUY2 || format == kUYVY; }  // one plane of four-byte groups
constexpr int n_planes(uint32_t format) { return packed(format) ? 1 : 3; }
// the bytes of the unit that pointers and pitches are multiples of: a sample, or a packed format's group
constexpr int element_bytes(uint32_t format) { return packed(format) ? 4 : ten_bit(format) ? 2 : 1; }

// Both kernels: a lane takes a run of kRun texels of one row -- eight luma samples and the four samples of either chroma plane under
// them, or the four groups of a packed row: no access of a lane is narrower than four bytes where pointers and pitches allow the wide form.
constexpr int kRun = 8;
// the bytes of plane p that go with a run: one wide access (16 for a packed row: four groups)
constexpr int run_bytes(uint32_t format, int p) { return packed(format) ? 16 : (p ? kRun / 2 : kRun) * (ten_bit(format) ? 2 : 1); }

// ---- the way in.  A workgroup of kInGroup lanes per 32 x 32 tile of the image (image_import::kTile): four runs across, 32 rows down.
constexpr int kInGroup = 128;

struct InParams {
  const void* plane[3];  // Y, Cb, Cr as the device addresses them; a packed format: plane[0] alone
  int64_t pitch[3];      // between rows of each plane, bytes
  int32_t w, h;          // of the luma plane
  int32_t cw;            // chroma samples of a row, and groups of a packed row: ceil(w / 2); there are h chroma rows
  uint32_t format;       // kI422 .. kUYVY: with kChromaLinear, which build of k_video_422_import takes the launch
  uint32_t flags;
  int32_t order;         // a packed group's bytes: 0 = Y0 Cb Y1 Cr (YUY2), 1 = Cb Y0 Cr Y1 (UYVY)
  int32_t wide[3];       // plane p and pitch[p] are multiples of run_bytes(format, p) and the row has a whole run: a run is one load
  int32_t yoff, coff, cy, crv, cgu, cgv, cbu;  // the conversion (a row of video_import::kCoefficients)
  int32_t x, y;          // the entry's place in level 0; level l's rectangle lies at (x >> l, y >> l)
  int32_t n_store;       // the levels of the chain that are stored: 0 .. n_store - 1 (Atlas::each_level; 0: nothing of the image is)
  int32_t ink;           // measure the ink boxes: every tile leaves its block in ink_block
  int32_t lw[image_import::kTileLevels], lh[image_import::kTileLevels];  // the image's extent at levels 0 .. 5
  uint32_t* level[image_import::kLevels];                                // the atlas
  int32_t size;                                                          // ... of size x size texels at level 0
  uint32_t* scratch;     // takes the level-5 image, lw[5] x lh[5] texels, rows packed: a texel per tile (image_import::TailParams::src)
  int32_t* ink_block;    // image_import::kInkWords words per tile, as the device addresses them
};

// ---- the way out.  A workgroup of kOutGroup lanes per kOutTileW x kOutTileH texels of the rectangle, a lane per run of eight texels of
// ONE row -- 32 runs across, 8 rows down; a wave covers two rows of the tile's whole width.
constexpr int kOutGroup = 256, kOutTileW = 256, kOutTileH = 8;

struct OutParams {
  const uint32_t* src;   // texel (0, 0) of the rectangle in the frame surface, RGBA8
  int64_t src_pitch;     // between rows of the surface, texels
  int32_t w, h;          // of the rectangle = of the luma plane
  void* plane[3];        // Y, Cb, Cr as the device addresses them; a packed format: plane[0] alone
  int64_t pitch[3];      // between rows of each plane, bytes
  uint32_t format;       // kI422 .. kUYVY: with kChromaLinear, which build of k_video_422_export takes the launch
  uint32_t flags;
  int32_t order;         // a packed group's bytes: 0 = Y0 Cb Y1 Cr (YUY2), 1 = Cb Y0 Cr Y1 (UYVY)
  int32_t wide_src;      // src and src_pitch are multiples of 16 bytes and w >= 8: a whole run is two 16-byte loads
  int32_t wide[3];       // plane p and pitch[p] are multiples of run_bytes(format, p) and the row has a whole run: a run is one store
  int32_t yoff, coff;    // the conversion (a row of video_export::kCoefficients)
  int32_t ky[3], ku[3], kv[3];  // the rows of R, G, B
};

}  // namespace video_422
}  // namespace fdh
