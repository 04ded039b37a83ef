// fdh_glyph_tables.h -- the tables a batch of glyphs hands to the batched kernels (GlyphMaker, fdh_glyphs.cpp): the glyph records, one word per
// 8 x 8 tile naming its glyph, and the owner bits that give a batch the painter's order of single puts.  Plain C++, no HIP and no atlas:
// the placed glyphs and the atlas's level count in, words out (tests/glyph_tables_emu compiles it as it stands).
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fdh_msdf_host.h"  // msdf::BatchGlyph, msdf::kOwnerLevel

namespace fdh {

constexpr size_t kBatchGlyphWords = sizeof(msdf::BatchGlyph) / 4;
struct BatchTables { std::vector<uint32_t> words; uint32_t n_tiles = 0, n_edges = 0; };  // words: glyph records, tile -> glyph, owner bits

inline int level_size(int v, int l) { return (v + (1 << l) - 1) >> l; }
// The 8 x 8 tiles of a glyph.  `thin_tiles`: a glyph 1 texel wide or high has tiles too (a distance field: its single put stores its level 0);
// without it such a glyph has none and gets no texel from any launch (a coverage glyph: the level chain stores nothing of it).
inline size_t batch_tiles(const msdf::BatchGlyph& t, bool thin_tiles) {
  return thin_tiles || (t.w > 1 && t.h > 1) ? (size_t)((t.w + 7) / 8) * ((t.h + 7) / 8) : 0;
}
inline size_t owner_bits(int w, int h, int n_levels) {
  size_t bits = 0;
  for (int l = msdf::kOwnerLevel; l < n_levels && level_size(w, l) > 1 && level_size(h, l) > 1; l++) bits += (size_t)level_size(w, l) * level_size(h, l);
  return bits;
}
inline size_t owner_bits(const msdf::BatchGlyph& t, int n_levels) { return owner_bits(t.w, t.h, n_levels); }
// the words of the tables of a whole batch in an atlas of at most `n_levels` levels: what the table buffer is reserved for before the
// first placement, whatever atlas the batch ends in
inline size_t batch_table_words(const std::vector<msdf::BatchGlyph>& tab, bool thin_tiles, int n_levels) {
  size_t all_tiles = 0, all_owner_words = 0;
  for (const msdf::BatchGlyph& t : tab) {
    all_tiles += batch_tiles(t, thin_tiles);
    all_owner_words += (owner_bits(t, n_levels) + 31) / 32;
  }
  return tab.size() * kBatchGlyphWords + all_tiles + all_owner_words + 1;
}
// The owner bits of m placed rectangles r[0 .. m - 1] (records with x, y, w, h and owner_off, the record's first bit; a batch of glyphs here, a
// batch of images in fdh_image_batch.h): level after level from msdf::kOwnerLevel on, the level rectangles painted in array order into a
// map of the box they span; a record gets the bits of the texels that are still its own.  `owner`: zeroed words.
template <typename Rect>
inline void paint_owner_bits(const Rect* r, int m, int n_levels, uint32_t* owner) {
  // (A level's rectangles are taken into locals first and the map is walked row by row: written as loops over r[k]'s own fields, whose
  // stores into the map may alias them, a 1920 x 1080 rectangle cost 40 us here -- more than the launch it was painted for.)
  struct LevelRect { int k, x, y, w, h; uint32_t bit; };
  std::vector<LevelRect> at;
  std::vector<int32_t> map;
  for (int l = msdf::kOwnerLevel; l < n_levels; l++) {
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = 0, by1 = 0;
    at.clear();
    for (int k = 0; k < m; k++) {
      const Rect& t = r[k];
      const int w = level_size(t.w, l), h = level_size(t.h, l);
      if (!(w > 1 && h > 1)) continue;
      uint32_t bit = t.owner_off;
      for (int d = msdf::kOwnerLevel; d < l; d++) bit += (uint32_t)(level_size(t.w, d) * level_size(t.h, d));
      at.push_back(LevelRect{k, t.x >> l, t.y >> l, w, h, bit});
      bx0 = std::min(bx0, t.x >> l); by0 = std::min(by0, t.y >> l);
      bx1 = std::max(bx1, (t.x >> l) + w); by1 = std::max(by1, (t.y >> l) + h);
    }
    if (bx1 <= bx0) break;  // no rectangle reaches this level, nor a deeper one
    const int bw = bx1 - bx0;
    map.assign((size_t)bw * (by1 - by0), -1);
    for (const LevelRect& t : at)
      for (int j = 0; j < t.h; j++) std::fill_n(map.data() + (size_t)(t.y + j - by0) * bw + (t.x - bx0), t.w, t.k);
    for (const LevelRect& t : at) {
      uint32_t bit = t.bit, word = 0u;  // (the bits of a word are gathered in a register: a read-modify-write of owner[] per texel waits for the last)
      for (int j = 0; j < t.h; j++) {
        const int32_t* row = map.data() + (size_t)(t.y + j - by0) * bw + (t.x - bx0);
        for (int i = 0; i < t.w; i++, bit++) {
          word |= (uint32_t)(row[i] == t.k) << (bit & 31u);
          if ((bit & 31u) == 31u) { owner[bit >> 5] |= word; word = 0u; }
        }
      }
      if (bit & 31u) owner[bit >> 5] |= word;
    }
  }
}
// The tables of glyphs first .. first + m - 1 as the batched kernels read them: the glyph records (their offsets filled in here, edge_off
// made relative to the first glyph's), one word per tile naming its glyph, and the owner bits: level after level from msdf::kOwnerLevel
// on, the rectangles painted in put order into a map of the box they span.
inline void batch_tables(std::vector<msdf::BatchGlyph>& tab, int first, int m, bool thin_tiles, int n_levels, BatchTables* T) {
  const uint32_t edge_base = tab[(size_t)first].edge_off;
  uint32_t field_off = 0, n_tiles = 0, owner_words = 0, n_edges = 0;
  for (int k = 0; k < m; k++) {
    msdf::BatchGlyph& t = tab[(size_t)(first + k)];
    t.edge_off -= edge_base; t.field_off = field_off; t.first_tile = n_tiles; t.owner_off = owner_words * 32u;
    field_off += (uint32_t)(t.w * t.h);
    n_tiles += (uint32_t)batch_tiles(t, thin_tiles);
    n_edges += (uint32_t)t.n_edges;
    owner_words += (uint32_t)((owner_bits(t, n_levels) + 31) / 32);
  }
  std::vector<uint32_t>& words = T->words;
  words.assign((size_t)m * kBatchGlyphWords + n_tiles + owner_words + 1, 0u);
  std::memcpy(words.data(), &tab[(size_t)first], (size_t)m * sizeof(msdf::BatchGlyph));
  uint32_t* tile_glyph = words.data() + (size_t)m * kBatchGlyphWords;
  uint32_t* owner = tile_glyph + n_tiles;
  for (int k = 0; k < m; k++) {
    const msdf::BatchGlyph& t = tab[(size_t)(first + k)];
    const uint32_t end = k + 1 < m ? tab[(size_t)(first + k + 1)].first_tile : n_tiles;
    for (uint32_t j = t.first_tile; j < end; j++) tile_glyph[j] = (uint32_t)k;
  }
  paint_owner_bits(&tab[(size_t)first], m, n_levels, owner);
  T->n_tiles = n_tiles; T->n_edges = n_edges;
}

}  // namespace fdh
