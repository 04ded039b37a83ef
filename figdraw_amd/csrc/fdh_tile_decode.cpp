// fdh_tile_decode.cpp -- the host-only decoder of a coded read, both stream versions (fdh_tile_decode.h).  No HIP, no context: what a
// receiver on any machine runs, and what a stand-alone program under a sanitizer links.
#include "fdh_tile_decode.h"

#include <cstring>
#include <vector>

namespace fdh {

namespace {
inline uint32_t load32(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline uint16_t load16(const uint8_t* p) { uint16_t v; std::memcpy(&v, p, 2); return v; }
inline int pal_bits(int n) { return n <= 2 ? 1 : n <= 4 ? 2 : n <= 16 ? 4 : 8; }
inline int copy_dx(const FdhCodedTile& t) { return (int16_t)(uint16_t)(t.solid & 0xFFFFu); }
inline int copy_dy(const FdhCodedTile& t) { return (int16_t)(uint16_t)(t.solid >> 16); }

// what (mode, n, w, h) give as the payload's size; the tile's fields are in range when this is called
inline uint32_t coded_size(const FdhCodedTile& t) {
  const uint32_t px = (uint32_t)t.w * (uint32_t)t.h;
  switch (t.mode) {
    case FDH_TILE_PAL: return 4u * t.n + 4u * ((px * (uint32_t)pal_bits(t.n) + 31u) / 32u);
    case FDH_TILE_RUNS: return 4u * ((6u * t.n + 3u) / 4u);
    case FDH_TILE_RAW: return 4u * px;
    default: return 0;
  }
}
// nullptr, or why tile t of a w x h image with payload_bytes of payload cannot be decoded
const char* coded_tile_fault(const FdhCodedTile& t, int version, int w, int h, const uint8_t* payload, int64_t payload_bytes) {
  if (!tile_in_image(t.x, t.y, t.w, t.h, w, h)) return "is not a bin inside the image";
  const uint32_t px = (uint32_t)t.w * (uint32_t)t.h;
  if (t.mode > (version >= 2 ? FDH_TILE_COPY : FDH_TILE_RAW)) return "has an unknown mode";
  if (t.mode == FDH_TILE_COPY) {
    if (t.bits != 0 || t.n != 0 || t.offset != 0 || t.size != 0) return "is a COPY with a field it does not use";
    if (!tile_in_image((int64_t)t.x + copy_dx(t), (int64_t)t.y + copy_dy(t), t.w, t.h, w, h)) return "is a COPY whose source is not inside the image";
    return nullptr;
  }
  if (t.mode == FDH_TILE_PAL) {
    if (t.n < 1 || t.n > 256) return "has a palette of no or of more than 256 colours";
    if (t.bits != pal_bits(t.n)) return "has bits that do not match its palette's size";
  } else if (t.bits != 0) return "has bits outside PAL";
  if (t.mode == FDH_TILE_RUNS && (t.n < 1 || t.n > px)) return "has no runs, or more runs than pixels";
  if ((t.mode == FDH_TILE_SOLID || t.mode == FDH_TILE_RAW) && t.n != 0) return "has a count its mode does not use";
  if (t.mode != FDH_TILE_SOLID && t.solid != 0) return "has a colour outside SOLID";
  if (t.size != coded_size(t)) return "has a size that is not its mode's";
  if (t.mode == FDH_TILE_SOLID) return t.offset != 0 ? "has an offset without a payload" : nullptr;
  if (t.offset % 16 != 0) return "has an offset that is not a multiple of 16";
  if ((int64_t)t.offset + (int64_t)t.size > payload_bytes) return "reaches beyond the payload";
  const uint8_t* p = payload + t.offset;
  if (t.mode == FDH_TILE_PAL) {
    const uint8_t* idx = p + 4 * (size_t)t.n;
    const uint32_t mask = (1u << t.bits) - 1u;
    for (uint32_t i = 0; i < px; i++) {
      const uint32_t at = i * t.bits;
      if (((load32(idx + 4 * (size_t)(at >> 5)) >> (at & 31u)) & mask) >= t.n) return "has a palette index beyond its palette";
    }
  } else if (t.mode == FDH_TILE_RUNS) {
    const uint8_t* len = p + 4 * (size_t)t.n;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < t.n; k++) sum += (uint64_t)load16(len + 2 * (size_t)k) + 1u;
    if (sum != px) return "has run lengths that do not sum to its pixels";
  }
  return nullptr;
}
}  // namespace

bool decode_tiles(const char* who, int version, uint8_t* image, int64_t pitch_bytes, int w, int h, const FdhCodedTile* tiles, int n_tiles,
                  const uint8_t* payload, int64_t payload_bytes, std::string* why) {
  const auto refuse = [&](const std::string& what) { *why = std::string(who) + ": " + what; return false; };
  if (n_tiles < 0) return refuse("negative tile count");
  if (payload_bytes < 0) return refuse("negative payload size");
  if (w < 0 || h < 0 || pitch_bytes < (int64_t)4 * w) return refuse("the pitch is shorter than a row");
  if (n_tiles == 0) return true;
  if (!image || !tiles || (!payload && payload_bytes > 0)) return refuse("null image, tiles or payload");
  size_t copied_px = 0;
  for (int i = 0; i < n_tiles; i++) {  // every tile is checked, its payload included, before any byte is written
    if (const char* fault = coded_tile_fault(tiles[i], version, w, h, payload, payload_bytes)) return refuse("tile " + std::to_string(i) + " " + fault);
    if (tiles[i].mode == FDH_TILE_COPY) copied_px += (size_t)tiles[i].w * (size_t)tiles[i].h;
  }
  // Every COPY source is the image as it was before this call, and a source may overlap tiles this call writes: the sources are staged
  // first, tight, in directory order.
  std::vector<uint32_t> staged(copied_px);
  size_t at_px = 0;
  for (int i = 0; i < n_tiles; i++) {
    const FdhCodedTile& t = tiles[i];
    if (t.mode != FDH_TILE_COPY) continue;
    const int64_t sx = (int64_t)t.x + copy_dx(t), sy = (int64_t)t.y + copy_dy(t);
    for (int r = 0; r < t.h; r++, at_px += (size_t)t.w) std::memcpy(staged.data() + at_px, image + (sy + r) * pitch_bytes + 4 * sx, (size_t)4 * t.w);
  }
  at_px = 0;
  uint32_t px[FDH_TILE_PX * FDH_TILE_PX];  // a tile, tight
  for (int i = 0; i < n_tiles; i++) {
    const FdhCodedTile& t = tiles[i];
    const uint32_t n_px = (uint32_t)t.w * (uint32_t)t.h;
    const uint8_t* p = (t.mode == FDH_TILE_SOLID || t.mode == FDH_TILE_COPY) ? nullptr : payload + t.offset;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(px);
    if (t.mode == FDH_TILE_SOLID) {
      for (uint32_t k = 0; k < n_px; k++) px[k] = t.solid;
    } else if (t.mode == FDH_TILE_PAL) {
      uint32_t pal[256];
      std::memcpy(pal, p, 4 * (size_t)t.n);
      const uint8_t* idx = p + 4 * (size_t)t.n;
      const uint32_t bits = t.bits, mask = (1u << bits) - 1u, per = 32u / bits;
      for (uint32_t k = 0; k < n_px; k += per) {  // a word of indices at a time
        uint32_t v = load32(idx + 4 * (size_t)(k / per));
        const uint32_t m = n_px - k < per ? n_px - k : per;
        for (uint32_t j = 0; j < m; j++, v >>= bits) px[k + j] = pal[v & mask];
      }
    } else if (t.mode == FDH_TILE_RUNS) {
      const uint8_t* len = p + 4 * (size_t)t.n;
      uint32_t at = 0;
      for (uint32_t k = 0; k < t.n; k++) {
        const uint32_t c = load32(p + 4 * (size_t)k), m = (uint32_t)load16(len + 2 * (size_t)k) + 1u;
        for (uint32_t j = 0; j < m; j++) px[at + j] = c;
        at += m;
      }
    } else if (t.mode == FDH_TILE_COPY) {
      src = reinterpret_cast<const uint8_t*>(staged.data() + at_px);
      at_px += n_px;
    } else {
      src = p;
    }
    for (int r = 0; r < t.h; r++) std::memcpy(image + (int64_t)(t.y + r) * pitch_bytes + (int64_t)4 * t.x, src + (size_t)r * 4 * t.w, (size_t)4 * t.w);
  }
  return true;
}

}  // namespace fdh
