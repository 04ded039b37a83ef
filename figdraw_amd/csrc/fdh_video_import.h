// fdh_video_import.h -- the parameter block of k_video_import (k_video_import.hip), the kernel behind fdh_put_video_frame and
// fdh_update_video_frame (the specification: include_glyphs/figdraw_hip_video_frame.h), and the table of the conversion's coefficients.
// Plain C++, no HIP and no atlas: GlyphMaker fills the block (fdh_glyphs.cpp), tests/video_frame_emu compiles it as it stands, with the
// kernel beside it.  The tile, the ink blocks and the tail are k_image_import's (fdh_image_import.h).
// At the end: what the batched kernel reads (fdh_put_video_frames, fdh_update_video_frames).
#pragma once
#include <cstdint>

#include "fdh_image_import.h"

namespace fdh {
namespace video_import {

enum : uint32_t { kBgra8 = 0, kNv12 = 1, kP010 = 2 };                     // FdhVideoFrame::format
enum : uint32_t { kChromaLinear = 1, kStraightAlpha = 2, kIgnoreAlpha = 4 };  // FdhVideoFrame::flags

// Yoff, Coff, cY, cRV, cGU, cGV, cBU: round-to-nearest-even of 255 * 2^14 times the terms of the specification, derived there with exact
// rationals (tests/test_video_frame_host.py derives them again).  Rows: matrix (BT601, BT709, BT2020) x range (limited, full), 8 bit then 10.
constexpr int32_t kCoefficients[2][3][2][7] = {
    {{{16, 128, 19077, 26149, 6419, 13320, 33050}, {0, 128, 16384, 22970, 5638, 11700, 29032}},
     {{16, 128, 19077, 29372, 3494, 8731, 34610}, {0, 128, 16384, 25802, 3069, 7670, 30402}},
     {{16, 128, 19077, 27503, 3069, 10657, 35091}, {0, 128, 16384, 24160, 2696, 9361, 30825}}},
    {{{64, 512, 4769, 6537, 1605, 3330, 8263}, {0, 512, 4084, 5726, 1405, 2917, 7237}},
     {{64, 512, 4769, 7343, 873, 2183, 8652}, {0, 512, 4084, 6431, 765, 1912, 7578}},
     {{64, 512, 4769, 6876, 767, 2664, 8773}, {0, 512, 4084, 6022, 672, 2333, 7684}}}};

struct Params {
  const void* luma;      // planes[0] as the device addresses it: the luma samples, or the BGRA texels
  const void* chroma;    // planes[1]: the Cb, Cr pairs (BGRA8: unused)
  int64_t pitch_y, pitch_c;  // between rows of either plane, bytes
  int32_t w, h;          // of the luma plane
  int32_t cw, ch;        // of the chroma plane, pairs: ceil(w / 2), ceil(h / 2)
  uint32_t format;       // kBgra8, kNv12, kP010: with kChromaLinear, which build of k_video_import takes the launch
  uint32_t flags;
  int32_t wide_y;        // luma and pitch_y are multiples of a run's bytes (NV12 4, P010 8, BGRA8 16) and w >= 4: a whole run is one load
  int32_t wide_c;        // chroma and pitch_c are multiples of two pairs' bytes (NV12 4, P010 8) and cw >= 2: two pairs are one load
  int32_t yoff, coff, cy, crv, cgu, cgv, cbu;  // the conversion (a row of kCoefficients)
  int32_t x, y;          // the entry's place in level 0; level l's rectangle lies at (x >> l, y >> l)
  int32_t n_store;       // the levels of the chain that are stored: 0 .. n_store - 1 (Atlas::each_level; 0: nothing of the image is)
  int32_t ink;           // measure the ink boxes: every tile leaves its block in ink_block
  int32_t lw[image_import::kTileLevels], lh[image_import::kTileLevels];  // the image's extent at levels 0 .. 5
  uint32_t* level[image_import::kLevels];                                // the atlas
  int32_t size;                                                          // ... of size x size texels at level 0
  uint32_t* scratch;     // takes the level-5 image, lw[5] x lh[5] texels, rows packed: a texel per tile (image_import::TailParams::src)
  int32_t* ink_block;    // image_import::kInkWords words per tile, as the device addresses them
};

// ---- the batches: fdh_put_video_frames and fdh_update_video_frames (the specification: include_glyphs/figdraw_hip_video_frames.h).
// k_video_import_batch<format, linear> runs over the tiles of all frames of one group of a batch; what Params holds per frame is a record
// in device memory, the atlas stays a launch argument (image_import::BatchAtlas), a tile's word is image_import::batch_tile_word.  The host
// builds the records, the tile words, the tails' records and the owner bits in fdh_video_batch.h.
constexpr int kBatchGroups = 5;  // the builds of k_video_import: BGRA8, then NV12, NV12 linear, P010, P010 linear
inline int batch_group(uint32_t format, uint32_t flags) { return format == kBgra8 ? 0 : 1 + 2 * (format == kP010) + (int)(flags & kChromaLinear); }
struct BatchFrame {
  const void* luma;      // as Params's, field for field
  const void* chroma;
  int64_t pitch_y, pitch_c;
  int32_t w, h, cw, ch;
  uint32_t format, flags;
  int32_t wide_y, wide_c;
  int32_t yoff, coff, cy, crv, cgu, cgv, cbu;
  int32_t x, y, n_store, ink;
  int32_t lw[image_import::kTileLevels], lh[image_import::kTileLevels];
  uint32_t scratch_off;  // the frame's level-5 image in the batch's scratch, in texels
  uint32_t ink_off;      // the frame's first ink block in the batch's blocks, in blocks (a frame with ink boxes only)
  uint32_t owner_off;    // the frame's first owner bit, as image_import::BatchImage's
};
static_assert(sizeof(BatchFrame) == 168, "the records are copied to the device as words");

}  // namespace video_import
}  // namespace fdh
