// fdh_stream.cpp -- coded damage readback (include/figdraw_hip_stream.h, which specifies the format): the host side of k_damage_encode's
// launch over damage readback's pending set (fdh_context.cpp keeps the set), and the host-only decoder.
#include "fdh_context.h"
#include "fdh_damage.h"

#include <cstring>

namespace fdh {

int64_t coded_damage_bound(int w, int h) {
  if (w <= 0 || h <= 0) return 0;
  return (int64_t)((w + FDH_TILE_PX - 1) / FDH_TILE_PX) * ((h + FDH_TILE_PX - 1) / FDH_TILE_PX) * FDH_TILE_BYTES;
}

void Context::read_damage_coded(const FdhCodedTile** tiles, const uint8_t** payload, int* n_tiles, int64_t* payload_bytes, int* frame_w,
                                int* frame_h, int* full) {
  bool all = false;
  const int n = readback_pending("fdh_read_damage_coded", &all);
  const int W = job_.W, H = job_.H, gx = job_.bins_x, gy = job_.bins_y, nb = gx * gy;
  if (W > INT16_MAX || H > INT16_MAX || coded_damage_bound(W, H) > (int64_t)UINT32_MAX)
    throw Error(FDH_ERR_INVALID, "fdh_read_damage_coded: a directory entry holds coordinates up to 32767 and offsets of 32 bits");
  int64_t bytes = 0;
  if (n > 0) {
    const size_t need = (size_t)coded_damage_bound(W, H);
    if (h_rb_code_.cap < need || h_rb_dir_.cap < (size_t)nb) {  // the whole grid's worst case, exactly (as fdh_read_damage sizes its buffer)
      h_rb_code_.release(); h_rb_code_dev_ = nullptr; h_rb_dir_dev_ = nullptr;
      FDH_HIP(hipHostMalloc((void**)&h_rb_code_.ptr, need, hipHostMallocDefault));
      h_rb_code_.cap = need;
      h_rb_dir_.reserve((size_t)nb);
      d_rb_cursor_.reserve(2);
      FDH_HIP(hipHostGetDevicePointer((void**)&h_rb_code_dev_, h_rb_code_.ptr, 0));
      FDH_HIP(hipHostGetDevicePointer((void**)&h_rb_dir_dev_, h_rb_dir_.ptr, 0));
    }
    DamageEncodeParams P;
    P.surf = fb_; P.stamp = d_rb_stamp_.ptr;  // (`all`: the stamps are not read, and may not exist yet)
    P.payload = h_rb_code_dev_;
    P.dir = reinterpret_cast<uint2*>(h_rb_dir_dev_);
    P.n_tiles = const_cast<uint32_t*>(rb_count_host_) + 1;
    P.payload_bytes = const_cast<uint32_t*>(rb_count_host_) + 2;
    P.cursor = reinterpret_cast<unsigned long long*>(d_rb_cursor_.ptr);
    P.epoch = rb_epoch_; P.n_pending = (uint32_t)n; P.W = W; P.H = H; P.bins_x = gx; P.bins_y = gy; P.all = all ? 1 : 0;
    rb_count_host_[1] = rb_count_host_[2] = 0xFFFFFFFFu;
    FDH_HIP(hipMemsetAsync(d_rb_cursor_.ptr, 0, 2 * sizeof(uint32_t), stream_));
    launch_damage_encode(stream_, P);
    FDH_HIP(hipGetLastError());
    FDH_HIP(hipStreamSynchronize(stream_));
    if (rb_count_host_[1] != (uint32_t)n) throw Error(FDH_ERR_HIP, "fdh_read_damage_coded: the encoder's tile count differs from the pending count");
    bytes = (int64_t)rb_count_host_[2];  // (the directory is not read here: the CPU's loads from page-locked memory are slow)
    if (bytes > (int64_t)need || bytes % 16 != 0) throw Error(FDH_ERR_HIP, "fdh_read_damage_coded: the encoder left no valid payload size");
    readback_consumed();
  }
  if (tiles) *tiles = h_rb_dir_.ptr;
  if (payload) *payload = h_rb_code_.ptr;
  if (n_tiles) *n_tiles = n;
  if (payload_bytes) *payload_bytes = bytes;
  if (frame_w) *frame_w = W;
  if (frame_h) *frame_h = H;
  if (full) *full = (nb > 0 && n == nb) ? 1 : 0;
}

namespace {
inline uint32_t load32(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline uint16_t load16(const uint8_t* p) { uint16_t v; std::memcpy(&v, p, 2); return v; }
inline int pal_bits(int n) { return n <= 2 ? 1 : n <= 4 ? 2 : n <= 16 ? 4 : 8; }

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
const char* coded_tile_fault(const FdhCodedTile& t, int w, int h, const uint8_t* payload, int64_t payload_bytes) {
  if (t.w < 1 || t.w > FDH_TILE_PX || t.h < 1 || t.h > FDH_TILE_PX || t.x < 0 || t.y < 0 || (int)t.x + t.w > w || (int)t.y + t.h > h) return "is not a bin inside the image";
  const uint32_t px = (uint32_t)t.w * (uint32_t)t.h;
  if (t.mode > FDH_TILE_RAW) return "has an unknown mode";
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

void decode_damage(uint8_t* image, int64_t pitch_bytes, int w, int h, const FdhCodedTile* tiles, int n_tiles, const uint8_t* payload, int64_t payload_bytes) {
  if (n_tiles < 0) throw Error(FDH_ERR_INVALID, "fdh_decode_damage: negative tile count");
  if (payload_bytes < 0) throw Error(FDH_ERR_INVALID, "fdh_decode_damage: negative payload size");
  if (w < 0 || h < 0 || pitch_bytes < (int64_t)4 * w) throw Error(FDH_ERR_INVALID, "fdh_decode_damage: the pitch is shorter than a row");
  if (n_tiles == 0) return;
  if (!image || !tiles || (!payload && payload_bytes > 0)) throw Error(FDH_ERR_INVALID, "fdh_decode_damage: null image, tiles or payload");
  for (int i = 0; i < n_tiles; i++)  // every tile is checked, its payload included, before any byte is written
    if (const char* why = coded_tile_fault(tiles[i], w, h, payload, payload_bytes))
      throw Error(FDH_ERR_INVALID, "fdh_decode_damage: tile " + std::to_string(i) + " " + why);
  uint32_t px[FDH_TILE_PX * FDH_TILE_PX];  // a tile, tight
  for (int i = 0; i < n_tiles; i++) {
    const FdhCodedTile& t = tiles[i];
    const uint32_t n_px = (uint32_t)t.w * (uint32_t)t.h;
    const uint8_t* p = t.mode == FDH_TILE_SOLID ? nullptr : payload + t.offset;
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
    } else {
      src = p;
    }
    for (int r = 0; r < t.h; r++) std::memcpy(image + (int64_t)(t.y + r) * pitch_bytes + (int64_t)4 * t.x, src + (size_t)r * 4 * t.w, (size_t)4 * t.w);
  }
}

}  // namespace fdh
