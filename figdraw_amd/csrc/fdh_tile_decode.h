// fdh_tile_decode.h -- the receiver's side of a coded read (fdh_tile_decode.cpp): the one decoder behind fdh_decode_damage (stream
// version 1: include/figdraw_hip_stream.h) and fdh_decode_damage_moved (version 2, mode COPY: include_readback/figdraw_hip_moves.h).
// Host only and self-contained -- the two public headers and the C++ library, no HIP -- so a stand-alone program links it as it is.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/figdraw_hip_readback.h"        // FDH_TILE_PX
#include "../../include_readback/figdraw_hip_moves.h"  // FdhCodedTile, FDH_TILE_SOLID .. FDH_TILE_COPY

namespace fdh {

// is (x, y, tw, th) a bin clipped to an image of w x h pixels?
inline bool tile_in_image(int64_t x, int64_t y, int64_t tw, int64_t th, int w, int h) {
  return tw >= 1 && tw <= FDH_TILE_PX && th >= 1 && th <= FDH_TILE_PX && x >= 0 && y >= 0 && x + tw <= w && y + th <= h;
}
// Decodes the tiles into the image; `version`: 1 or 2.  Everything is validated before the first byte is written.  false: the stream is
// refused, *why says why (it begins with `who`), and the image is as it was.
bool decode_tiles(const char* who, int version, uint8_t* image, int64_t pitch_bytes, int w, int h, const FdhCodedTile* tiles, int n_tiles,
                  const uint8_t* payload, int64_t payload_bytes, std::string* why);

}  // namespace fdh
