// fdh_image_import.h -- the parameter blocks of k_image_import and k_image_import_tail (k_image_import.hip), the kernels behind
// fdh_put_image_device and fdh_update_image_device (the specification: include_glyphs/figdraw_hip_device_image.h).  Plain C++, no HIP and no
// atlas: GlyphMaker fills the blocks (fdh_glyphs.cpp), tests/device_image_emu compiles them as they stand, with the kernels beside them.
// At the end: what the batched kernels read (fdh_put_images_device, fdh_update_images_device).
#pragma once
#include <cstdint>

namespace fdh {
namespace image_import {

constexpr int kLevels = 14;      // of an atlas (kMaxMips)
constexpr int kTile = 32;        // a workgroup's tile of the image, kTile x kTile texels; the tile grid starts at the image's own origin
constexpr int kTileLevels = 6;   // the levels a tile makes of itself: 0 (32 x 32) .. 5 (one texel)
constexpr int kGroup = 256;      // lanes of a workgroup of either kernel: four texels of level 0 each
constexpr int kTailMax = 64;     // the tail's source is at most kTailMax x kTailMax texels
constexpr int kInkMax = 128;     // images up to kInkMax x kInkMax get ink boxes (measure_ink, fdh_atlas.cpp)
// The ink blocks, one per tile, tile after tile in page-locked host memory: for k = 0 .. 7 the box {x0, y0, x1, y1} (image texels, x1 / y1
// exclusive) of the tile's texels whose alpha exceeds 16 k (words 4 k ..), then the same of the largest colour channel (words 32 + 4 k ..);
// a box with no texel is {kInkEmpty, kInkEmpty, 0, 0}.  A workgroup stores its block whole: nothing has to be cleared ahead of the launch
// and nothing copied back behind it.  The host folds the tiles' blocks (fold_ink); a box whose x1 is still 0 has no texel.
constexpr int kInkWords = 64;
constexpr int kInkEmpty = 32767;
constexpr int kInkTiles = (kInkMax / kTile) * (kInkMax / kTile);  // of an image that gets ink boxes, at most
inline void fold_ink(const int32_t* blocks, int tiles, int32_t out[kInkWords]) {
  for (int i = 0; i < kInkWords; i++) out[i] = (i & 2) ? 0 : kInkEmpty;
  for (int t = 0; t < tiles; t++)
    for (int i = 0; i < kInkWords; i++) {
      const int32_t v = blocks[t * kInkWords + i];
      if ((i & 2) ? v > out[i] : v < out[i]) out[i] = v;
    }
}

enum : uint32_t { kRgba8 = 0, kPlanarF32 = 1, kPlanarF16 = 2 };  // FdhDeviceImage::format
enum : uint32_t { kStraightAlpha = 1 };                          // FdhDeviceImage::flags

struct Params {
  const void* data;      // the source: device memory, or page-locked host memory as the device addresses it
  int64_t pitch_bytes;   // between rows (of one plane)
  int64_t plane_bytes;   // between planes
  int32_t w, h;
  uint32_t format;       // kRgba8, kPlanarF32, kPlanarF16: which build of k_image_import takes the launch
  uint32_t channels;     // planar: 1, 3 or 4
  uint32_t flags;        // kStraightAlpha
  int32_t wide;          // data, pitch_bytes and plane_bytes are multiples of 16 and w >= 4: a whole run of four texels is one load (per plane)
  int32_t x, y;          // the entry's place in level 0; level l's rectangle lies at (x >> l, y >> l)
  int32_t n_store;       // the levels of the chain that are stored: 0 .. n_store - 1 (Atlas::each_level; 0: nothing of the image is)
  int32_t ink;           // measure the ink boxes: every tile leaves its block in ink_block
  int32_t lw[kTileLevels], lh[kTileLevels];  // the image's extent at levels 0 .. 5: ceil(w / 2^l), ceil(h / 2^l)
  uint32_t* level[kLevels];                  // the atlas
  int32_t size;                              // ... of size x size texels at level 0
  uint32_t* scratch;     // takes the level-5 image, lw[5] x lh[5] texels, rows packed: a texel per tile
  int32_t* ink_block;    // kInkWords words per tile, as the device addresses them
};

// The rest of the chain: `src` holds the image at level l0 (sw x sh texels, rows packed, at most kTailMax each way), which is stored
// already; levels l0 + 1 .. n_store - 1 follow.
struct TailParams {
  const uint32_t* src;
  int32_t sw, sh, l0, n_store;
  int32_t x, y, size;
  uint32_t* level[kLevels];
};

// ---- the batches: fdh_put_images_device and fdh_update_images_device (the specification: include_glyphs/figdraw_hip_device_images.h).
// k_image_import_batch<format> runs over the tiles of all images of one format, k_image_import_tail_batch over the images whose chain
// goes beyond level 5.  What Params holds per image is a record in device memory; the atlas stays a launch argument.  The host builds the
// records, the tile words and the owner bits in fdh_image_batch.h.
constexpr int kOwnerLevel = 4;        // msdf::kOwnerLevel (fdh_image_batch.h asserts it): from this level on two rectangles of a batch can meet
constexpr int kBatchMaxExtent = 2048; // of an image of a batch: its level-5 image is what the tail's workgroup holds (kTailMax)
// a tile's word: the image's index in the records | the tile's column << 16 | its row << 22 (64 tiles each way at the most)
inline uint32_t batch_tile_word(uint32_t image, uint32_t tx, uint32_t ty) { return image | (tx << 16) | (ty << 22); }
struct BatchImage {
  const void* data;      // as Params::data
  int64_t pitch_bytes, plane_bytes;
  int32_t w, h;
  uint32_t format, channels, flags;
  int32_t wide;
  int32_t x, y, n_store, ink;
  int32_t lw[kTileLevels], lh[kTileLevels];
  uint32_t scratch_off;  // the image's level-5 image in the batch's scratch, in texels
  uint32_t ink_off;      // the image's first ink block in the batch's blocks, in blocks (an image with ink boxes only)
  uint32_t owner_off;    // the image's first owner bit: per level from kOwnerLevel on lw x lh bits, rows packed; set: the texel is this image's
  uint32_t reserved;
};
static_assert(sizeof(BatchImage) == 128, "the records are copied to the device as words");
struct BatchAtlas {
  uint32_t* level[kLevels];
  int32_t size;
};

}  // namespace image_import
}  // namespace fdh
