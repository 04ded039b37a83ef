// fdh_video_batch.h -- the tables a batch of decoded video frames hands to the batched kernels (Importer::put_video_frames, fdh_import.cpp):
// the frame records (video_import::BatchFrame, fdh_video_import.h, beside the single kernel's block), one word per 32 x 32 tile naming its
// frame and the tile's place in it, grouped by the five builds of k_video_import_batch (video_import::batch_group) -- a launch per group
// runs over its words --, the records and indices k_image_import_tail_batch reads of the frames whose chain goes beyond level 5
// (image_import::BatchImage, the fields the tail reads), and the owner bits that give a batch the painter's order of single puts.  Plain
// C++, no HIP and no atlas: the placed frames and the atlas's level count in, words out (tests/video_batch_tables_emu compiles it as it
// stands).  The sibling of fdh_image_batch.h for five groups; one difference: a frame 1 texel wide or high keeps its tiles in the table --
// nothing of it is stored (n_store == 0), its ink blocks are made -- so that the conversion is stated on the device alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fdh_glyph_tables.h"  // level_size, owner_bits, paint_owner_bits
#include "fdh_video_import.h"  // and through it fdh_image_import.h

namespace fdh {
namespace video_batch {
namespace ii = image_import;
namespace vi = video_import;

static_assert(ii::kOwnerLevel == msdf::kOwnerLevel, "one level from which the rectangles of a batch can meet, for glyphs, images and frames");
static_assert(sizeof(vi::BatchFrame) % 8 == 0, "the tails' records lie behind the frames' and hold a pointer");
constexpr size_t kFrameWords = sizeof(vi::BatchFrame) / 4;
constexpr size_t kTailWords = sizeof(ii::BatchImage) / 4;
constexpr int kGroups = vi::kBatchGroups;
constexpr int kMaxFrames = 65535;                 // a tile word holds the frame's index in 16 bits
constexpr int64_t kMaxTiles = (int64_t)1 << 18;   // of a batch: a tile table of 1 MB, ink blocks of 64 MB at the most

// the 32 x 32 tiles a frame of w x h covers: the batch's limit counts these, and all of them are in the table
inline size_t tiles_of(int w, int h) { return (size_t)((w + ii::kTile - 1) / ii::kTile) * ((h + ii::kTile - 1) / ii::kTile); }
inline bool has_ink(int w, int h) { return w <= ii::kInkMax && h <= ii::kInkMax; }
// the levels of a frame's chain that are stored in an atlas of n_levels levels (Atlas::each_level)
inline int stored_levels(int w, int h, int n_levels) {
  int n = 0;
  for (int l = 0; l < n_levels && level_size(w, l) > 1 && level_size(h, l) > 1; l++) n++;
  return n;
}

struct Tables {
  std::vector<uint32_t> words;                                 // the records, the tails' records, the tile words, the tail indices, the owner bits
  uint32_t tile_first[kGroups] = {}, tile_count[kGroups] = {};  // a group's words among the tile words
  uint32_t n_tiles = 0, n_tails = 0, ink_blocks = 0;
  size_t tail_records_at = 0, tiles_at = 0, tails_at = 0, owner_at = 0;  // where the four tables behind the records begin, in words
};
// the words of the tables of a whole batch in an atlas of at most `n_levels` levels: what the table buffer is reserved for before the
// first placement, whatever atlas the batch ends in
inline size_t table_words(const std::vector<vi::BatchFrame>& tab, int n_levels) {
  size_t tiles = 0, owner_words = 0, tails = 0;
  for (const vi::BatchFrame& t : tab) {
    tiles += tiles_of(t.w, t.h);
    owner_words += (owner_bits(t.w, t.h, n_levels) + 31) / 32;
    if (stored_levels(t.w, t.h, n_levels) > ii::kTileLevels) tails++;
  }
  return tab.size() * kFrameWords + tails * (kTailWords + 1) + tiles + owner_words + 1;
}
// The tables of frames first .. first + m - 1, which have their places (x, y), their planes and their conversion: the rest of each record
// is filled in here -- n_store, ink, the lw / lh rows and the offsets into the scratch (a texel per tile), the ink blocks (a block per tile
// of a frame that gets ink boxes) and the owner bits.
inline void tables(std::vector<vi::BatchFrame>& tab, int first, int m, int n_levels, Tables* T) {
  *T = Tables{};
  uint32_t scratch = 0, owner_words = 0;
  for (int k = 0; k < m; k++) {
    vi::BatchFrame& t = tab[(size_t)(first + k)];
    t.n_store = stored_levels(t.w, t.h, n_levels);
    for (int l = 0; l < ii::kTileLevels; l++) { t.lw[l] = level_size(t.w, l); t.lh[l] = level_size(t.h, l); }
    const uint32_t tiles = (uint32_t)tiles_of(t.w, t.h);
    t.ink = has_ink(t.w, t.h);
    t.scratch_off = scratch; t.ink_off = T->ink_blocks; t.owner_off = owner_words * 32u;
    scratch += tiles;
    if (t.ink) T->ink_blocks += tiles;
    owner_words += (uint32_t)((owner_bits(t.w, t.h, n_levels) + 31) / 32);
    T->tile_count[vi::batch_group(t.format, t.flags)] += tiles;
    if (t.n_store > ii::kTileLevels) T->n_tails++;
  }
  T->n_tiles = scratch;
  for (int g = 1; g < kGroups; g++) T->tile_first[g] = T->tile_first[g - 1] + T->tile_count[g - 1];
  T->tail_records_at = (size_t)m * kFrameWords;
  T->tiles_at = T->tail_records_at + T->n_tails * kTailWords;
  T->tails_at = T->tiles_at + T->n_tiles;
  T->owner_at = T->tails_at + T->n_tails;
  std::vector<uint32_t>& words = T->words;
  words.assign(T->owner_at + owner_words + 1, 0u);
  std::memcpy(words.data(), &tab[(size_t)first], (size_t)m * sizeof(vi::BatchFrame));
  uint32_t next[kGroups], tail = 0;
  for (int g = 0; g < kGroups; g++) next[g] = T->tile_first[g];
  for (int k = 0; k < m; k++) {
    const vi::BatchFrame& t = tab[(size_t)(first + k)];
    if (t.n_store > ii::kTileLevels) {  // what k_image_import_tail_batch reads of an image
      ii::BatchImage r{};
      r.w = t.w; r.h = t.h; r.x = t.x; r.y = t.y; r.n_store = t.n_store;
      for (int l = 0; l < ii::kTileLevels; l++) { r.lw[l] = t.lw[l]; r.lh[l] = t.lh[l]; }
      r.scratch_off = t.scratch_off; r.owner_off = t.owner_off;
      std::memcpy(words.data() + T->tail_records_at + tail * kTailWords, &r, sizeof r);
      words[T->tails_at + tail] = tail;
      tail++;
    }
    uint32_t& at = next[vi::batch_group(t.format, t.flags)];
    for (int ty = 0; ty < t.lh[ii::kTileLevels - 1]; ty++)
      for (int tx = 0; tx < t.lw[ii::kTileLevels - 1]; tx++) words[T->tiles_at + at++] = ii::batch_tile_word((uint32_t)k, (uint32_t)tx, (uint32_t)ty);
  }
  paint_owner_bits(&tab[(size_t)first], m, n_levels, words.data() + T->owner_at);
}

}  // namespace video_batch
}  // namespace fdh
