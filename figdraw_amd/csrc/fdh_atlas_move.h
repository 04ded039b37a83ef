// fdh_atlas_move.h -- the tables of k_atlas_move (k_atlas_move.hip), the kernel that carries rectangles of texels from the levels of one atlas
// into the levels of another for fdh_compact_atlas (include_glyphs/figdraw_hip_atlas.h): one record per rectangle, one word per tile
// naming its record, and owner bits for the texels that two rectangles of the destination share.  Plain C++, no HIP and no atlas: the
// rectangles in, words out (tests/atlas_move_emu compiles it as it stands, with the kernel beside it).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace fdh {
namespace move {

constexpr int kLevels = 14;                  // of an atlas (kMaxMips)
constexpr int kBuffer = -1;                  // as a record's level: the launch's dense buffer instead of an atlas level
constexpr uint32_t kNoOwner = 0xFFFFFFFFu;   // as a record's owner_off: the record stores every texel

// the two atlases (and the dense buffers) as they travel in the kernel arguments
struct Views {
  const uint32_t* from[kLevels];
  uint32_t* to[kLevels];
  int from_size, from_levels, to_size, to_levels;
  const uint32_t* buf_in;   // where records with src_level == kBuffer read: rows packed, w texels from row to row, sx = the first word
  uint32_t* buf_out;        // ... with dst_level == kBuffer write: dx = the first word
};
// one rectangle as the kernel reads it, 12 words
struct Record {
  int32_t src_level, sx, sy;
  int32_t dst_level, dx, dy;
  int32_t w, h;
  uint32_t first_tile;
  uint32_t owner_off;   // the record's first bit in the owner words, one bit per texel, rows packed; kNoOwner: none
  uint32_t wide;        // the record's tiles are 64 x 4 (a lane per texel of a row of 64, four rows one after the other), else 8 x 8
  uint32_t pad;
};
static_assert(sizeof(Record) == 48, "Record is 12 words");
constexpr size_t kRecordWords = sizeof(Record) / 4;
// A rectangle of at least this width gets wide tiles: a wave then stores whole 256-byte runs of a row.  An 8 x 8 tile stores 32 bytes per
// row: right for glyphs (12 x 20), a sixteenth of a cache line's worth of lanes for an image a thousand texels wide.
constexpr int kWideFrom = 64;
inline bool is_wide(int w) { return w >= kWideFrom; }
inline uint32_t tiles_of(int w, int h) {
  return is_wide(w) ? (uint32_t)((w + 63) / 64) * (uint32_t)((h + 3) / 4) : (uint32_t)((w + 7) / 8) * (uint32_t)((h + 7) / 8);
}

// A rectangle for the builder, in the painter's order of the DESTINATION: a later rectangle of the same destination level owns the texels
// it shares with an earlier one.  `copy` false: the rectangle takes part in that order and is not copied (somebody else writes it).
struct Rect {
  int src_level, sx, sy, dst_level, dx, dy, w, h;
  bool copy;
};
struct Tables {
  std::vector<uint32_t> words;  // the records, the tile words, the owner words (+ 1: never empty)
  uint32_t n_records = 0, n_tiles = 0, owner_words = 0;
  int64_t texels = 0;           // of the copied rectangles
  int owner_level = -1;         // the lowest destination level at which a copied rectangle shares a texel with a later one (-1: none does)
};

inline bool meet(const Rect& a, const Rect& b, int* x0, int* y0, int* x1, int* y1) {
  *x0 = a.dx > b.dx ? a.dx : b.dx; *y0 = a.dy > b.dy ? a.dy : b.dy;
  *x1 = a.dx + a.w < b.dx + b.w ? a.dx + a.w : b.dx + b.w; *y1 = a.dy + a.h < b.dy + b.h ? a.dy + a.h : b.dy + b.h;
  return *x0 < *x1 && *y0 < *y1;
}
// The tables of the copied rectangles of `rects`.  Owner bits exist for the records that need them alone: a record that no later
// rectangle of its level touches stores every texel.  No map of a level is painted: a record's bits start all set and lose the texels of
// each later rectangle it meets.  (Rectangles of one level are compared pair by pair: a few thousand rectangles at the most.)
inline void build_tables(const std::vector<Rect>& rects, Tables* T) {
  std::vector<size_t> by_level[kLevels];
  for (size_t i = 0; i < rects.size(); i++)
    if (rects[i].dst_level >= 0 && rects[i].dst_level < kLevels) by_level[rects[i].dst_level].push_back(i);
  std::vector<Record> recs;
  std::vector<std::vector<uint32_t>> bits;  // per record: empty, or its owner bits
  uint32_t n_tiles = 0, owner_words = 0;
  T->texels = 0; T->owner_level = -1;
  for (size_t i = 0; i < rects.size(); i++) {
    const Rect& r = rects[i];
    if (!r.copy || r.w <= 0 || r.h <= 0) continue;
    Record d{};
    d.src_level = r.src_level; d.sx = r.sx; d.sy = r.sy; d.dst_level = r.dst_level; d.dx = r.dx; d.dy = r.dy; d.w = r.w; d.h = r.h;
    d.first_tile = n_tiles; d.owner_off = kNoOwner; d.wide = is_wide(r.w) ? 1u : 0u;
    n_tiles += tiles_of(r.w, r.h);
    T->texels += (int64_t)r.w * r.h;
    std::vector<uint32_t> own;
    if (r.dst_level >= 0 && r.dst_level < kLevels) {
      for (size_t j : by_level[r.dst_level]) {
        if (j <= i) continue;
        int x0, y0, x1, y1;
        if (!meet(r, rects[j], &x0, &y0, &x1, &y1)) continue;
        if (own.empty()) {
          const size_t n = (size_t)r.w * r.h;
          own.assign((n + 31) / 32, 0xFFFFFFFFu);
          if (n & 31) own.back() = (1u << (n & 31)) - 1u;
        }
        for (int y = y0; y < y1; y++)
          for (int x = x0; x < x1; x++) {
            const size_t b = (size_t)(y - r.dy) * r.w + (x - r.dx);
            own[b >> 5] &= ~(1u << (b & 31));
          }
        if (T->owner_level < 0 || r.dst_level < T->owner_level) T->owner_level = r.dst_level;
      }
    }
    if (!own.empty()) { d.owner_off = owner_words * 32u; owner_words += (uint32_t)own.size(); }
    recs.push_back(d);
    bits.push_back(std::move(own));
  }
  std::vector<uint32_t>& words = T->words;
  words.assign(recs.size() * kRecordWords + n_tiles + owner_words + 1, 0u);
  uint32_t* w = words.data();
  if (!recs.empty()) std::memcpy(w, recs.data(), recs.size() * sizeof(Record));
  uint32_t* tile_rec = w + recs.size() * kRecordWords;
  for (size_t k = 0; k < recs.size(); k++) {
    const uint32_t end = k + 1 < recs.size() ? recs[k + 1].first_tile : n_tiles;
    for (uint32_t t = recs[k].first_tile; t < end; t++) tile_rec[t] = (uint32_t)k;
  }
  uint32_t* owner = tile_rec + n_tiles;
  for (size_t k = 0; k < recs.size(); k++)
    for (size_t q = 0; q < bits[k].size(); q++) owner[recs[k].owner_off / 32u + q] = bits[k][q];
  T->n_records = (uint32_t)recs.size(); T->n_tiles = n_tiles; T->owner_words = owner_words;
}

}  // namespace move
}  // namespace fdh
