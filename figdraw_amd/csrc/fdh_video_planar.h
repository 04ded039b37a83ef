// fdh_video_planar.h -- the parameter blocks of k_video_planar_import (k_video_planar_import.hip), the kernel behind fdh_put_video_planes
// and fdh_update_video_planes, and of k_video_planar_export (k_video_planar_export.hip), the kernel behind fdh_read_video_planes (the
// specification: include_video/figdraw_hip_video_planar.h).  Plain C++, no HIP, no atlas and no context: GlyphMaker fills the first
// block (fdh_glyphs.cpp), fdh_video_out.cpp the second; tests/video_planar_in_emu and tests/video_planar_out_emu compile them as they
// stand, with the kernels beside them.  The coefficients are the siblings' tables (fdh_video_import.h, fdh_video_export.h): the NV12 row
// for an 8-bit format, the P010 row for a 10-bit one.  The way in's tile, ink blocks and tail are k_image_import's (fdh_image_import.h).
#pragma once
#include <cstdint>

#include "fdh_image_import.h"

namespace fdh {
namespace video_planar {

enum : uint32_t { kI420 = 3, kI010 = 4, kI444 = 5, kI410 = 6 };  // FdhVideoPlanes::format, FdhVideoPlanesTarget::format
enum : uint32_t { kChromaLinear = 1 };                          // ... ::flags
constexpr bool ten_bit(uint32_t format) { return format == kI010 || format == kI410; }
constexpr bool full_chroma(uint32_t format) { return format == kI444 || format == kI410; }  // 4:4:4: a chroma sample per texel

// Both kernels: a lane takes a run of kRun texels -- eight luma samples, and the four (4:2:0) or eight (4:4:4) samples of either chroma
// plane that go with them: no access of a lane is narrower than four bytes where pointers and pitches allow the wide form.
constexpr int kRun = 8;

// ---- the way in.  A workgroup of kInGroup lanes per 32 x 32 tile of the image (image_import::kTile): four runs across, 32 rows down.
constexpr int kInGroup = 128;

struct InParams {
  const void* plane[3];  // Y, Cb, Cr as the device addresses them
  int64_t pitch[3];      // between rows of each plane, bytes
  int32_t w, h;          // of the luma plane
  int32_t cw, ch;        // of either chroma plane: ceil(w / 2) x ceil(h / 2) for 4:2:0, w x h for 4:4:4
  uint32_t format;       // kI420 .. kI410: with kChromaLinear, which build of k_video_planar_import takes the launch
  uint32_t flags;
  int32_t wide[3];       // plane p and pitch[p] are multiples of a run's bytes in that plane and the plane has a whole run: a run is one
                         // load -- eight samples of luma or of a 4:4:4 chroma plane, four of a 4:2:0 chroma plane
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

// ---- the way out.  A workgroup of kOutGroup lanes per kOutTileW x kOutTileH texels of the rectangle, a lane per run of eight texels by
// two rows -- 32 runs across, 8 row pairs down; a wave covers two row pairs of the tile's whole width.
constexpr int kOutGroup = 256, kOutTileW = 256, kOutTileH = 16;

struct OutParams {
  const uint32_t* src;   // texel (0, 0) of the rectangle in the frame surface, RGBA8
  int64_t src_pitch;     // between rows of the surface, texels
  int32_t w, h;          // of the rectangle = of the luma plane
  void* plane[3];        // Y, Cb, Cr as the device addresses them
  int64_t pitch[3];      // between rows of each plane, bytes
  uint32_t format;       // kI420 .. kI410: with kChromaLinear, which build of k_video_planar_export takes the launch
  uint32_t flags;
  int32_t wide_src;      // src and src_pitch are multiples of 16 bytes and w >= 8: a whole run is two 16-byte loads
  int32_t wide[3];       // plane p and pitch[p] are multiples of a run's bytes in that plane and the plane has a whole run: a run is one store
  int32_t yoff, coff;    // the conversion (a row of video_export::kCoefficients)
  int32_t ky[3], ku[3], kv[3];  // the rows of R, G, B
};

}  // namespace video_planar
}  // namespace fdh
