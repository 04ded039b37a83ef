// fdh_image_batch.h -- the tables a batch of device images hands to the batched kernels of k_image_import.hip (Importer::put_device_images,
// fdh_import.cpp): the image records (image_import::BatchImage, fdh_image_import.h, beside the single kernels' blocks), one word per 32 x 32
// tile naming its image and the tile's place in it, grouped by format -- a launch per format runs over its group --, the indices of the
// images whose chain goes beyond level 5, and the owner bits that give a batch the painter's order of single puts.  Plain C++, no HIP and
// no atlas: the placed images and the atlas's level count in, words out (tests/image_batch_tables_emu compiles it as it stands).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fdh_glyph_tables.h"  // level_size, owner_bits, paint_owner_bits
#include "fdh_image_import.h"

namespace fdh {
namespace image_batch {
namespace ii = image_import;

static_assert(ii::kOwnerLevel == msdf::kOwnerLevel, "one level from which the rectangles of a batch can meet, for glyphs and for images");
constexpr size_t kImageWords = sizeof(ii::BatchImage) / 4;
constexpr int kFormats = 3;                       // kRgba8, kPlanarF32, kPlanarF16
constexpr int kMaxImages = 65535;                 // a tile word holds the image's index in 16 bits
constexpr int64_t kMaxTiles = (int64_t)1 << 18;   // of a batch: a tile table of 1 MB, ink blocks of 64 MB at the most

// the 32 x 32 tiles an image of w x h covers (the batch's limit counts these)
inline size_t covered_tiles(int w, int h) { return (size_t)((w + ii::kTile - 1) / ii::kTile) * ((h + ii::kTile - 1) / ii::kTile); }
// ... and those it has in the table: none where it is 1 texel wide or high -- nothing of such an image is stored
inline size_t table_tiles(int w, int h) { return w > 1 && h > 1 ? covered_tiles(w, h) : 0; }
inline bool has_ink(int w, int h) { return w <= ii::kInkMax && h <= ii::kInkMax; }

struct Tables {
  std::vector<uint32_t> words;                            // the records, the tile words, the tail indices, the owner bits
  uint32_t tile_first[kFormats] = {}, tile_count[kFormats] = {};  // a format's group among the tile words
  uint32_t n_tiles = 0, n_tails = 0, ink_blocks = 0;
  size_t tiles_at = 0, tails_at = 0, owner_at = 0;        // where the three tables begin, in words
};
// the words of the tables of a whole batch in an atlas of at most `n_levels` levels: what the table buffer is reserved for before the
// first placement, whatever atlas the batch ends in
inline size_t table_words(const std::vector<ii::BatchImage>& tab, int n_levels) {
  size_t tiles = 0, owner_words = 0;
  for (const ii::BatchImage& t : tab) {
    tiles += table_tiles(t.w, t.h);
    owner_words += (owner_bits(t.w, t.h, n_levels) + 31) / 32;
  }
  return tab.size() * (kImageWords + 1) + tiles + owner_words + 1;
}
// The tables of images first .. first + m - 1, which have their places (x, y) and their sources: the rest of each record is filled in
// here -- n_store, ink, the lw / lh rows and the offsets into the scratch (a texel per tile), the ink blocks (a block per tile of an image
// that gets ink boxes) and the owner bits.
inline void tables(std::vector<ii::BatchImage>& tab, int first, int m, int n_levels, Tables* T) {
  *T = Tables{};
  uint32_t scratch = 0, owner_words = 0;
  for (int k = 0; k < m; k++) {
    ii::BatchImage& t = tab[(size_t)(first + k)];
    t.n_store = 0;
    for (int l = 0; l < n_levels && level_size(t.w, l) > 1 && level_size(t.h, l) > 1; l++) t.n_store++;
    for (int l = 0; l < ii::kTileLevels; l++) { t.lw[l] = level_size(t.w, l); t.lh[l] = level_size(t.h, l); }
    const uint32_t tiles = (uint32_t)table_tiles(t.w, t.h);
    t.ink = tiles && has_ink(t.w, t.h);
    t.scratch_off = scratch; t.ink_off = T->ink_blocks; t.owner_off = owner_words * 32u;
    scratch += tiles;
    if (t.ink) T->ink_blocks += tiles;
    owner_words += (uint32_t)((owner_bits(t.w, t.h, n_levels) + 31) / 32);
    if (t.format < (uint32_t)kFormats) T->tile_count[t.format] += tiles;
    if (t.n_store > ii::kTileLevels) T->n_tails++;
  }
  T->n_tiles = scratch;
  for (int f = 1; f < kFormats; f++) T->tile_first[f] = T->tile_first[f - 1] + T->tile_count[f - 1];
  T->tiles_at = (size_t)m * kImageWords;
  T->tails_at = T->tiles_at + T->n_tiles;
  T->owner_at = T->tails_at + T->n_tails;
  std::vector<uint32_t>& words = T->words;
  words.assign(T->owner_at + owner_words + 1, 0u);
  std::memcpy(words.data(), &tab[(size_t)first], (size_t)m * sizeof(ii::BatchImage));
  uint32_t next[kFormats], tail = 0;
  for (int f = 0; f < kFormats; f++) next[f] = T->tile_first[f];
  for (int k = 0; k < m; k++) {
    const ii::BatchImage& t = tab[(size_t)(first + k)];
    if (t.n_store > ii::kTileLevels) words[T->tails_at + tail++] = (uint32_t)k;
    if (!table_tiles(t.w, t.h) || t.format >= (uint32_t)kFormats) continue;
    for (int ty = 0; ty < t.lh[ii::kTileLevels - 1]; ty++)
      for (int tx = 0; tx < t.lw[ii::kTileLevels - 1]; tx++) words[T->tiles_at + next[t.format]++] = ii::batch_tile_word((uint32_t)k, (uint32_t)tx, (uint32_t)ty);
  }
  paint_owner_bits(&tab[(size_t)first], m, n_levels, words.data() + T->owner_at);
}

}  // namespace image_batch
}  // namespace fdh
