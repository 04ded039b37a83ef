// fdh_damage_move.h -- moved damage readback's kernels (k_damage_move.hip; include_readback/figdraw_hip_moves.h is the specification):
// their parameter blocks.  Like fdh_damage_read.h, which it builds on, it names nothing but kBin, the vector types and hipStream_t, so the
// host shim of tests/move_emu compiles against this very file.
#pragma once
#include "fdh_damage_read.h"

namespace fdh {

constexpr int kDamageMovesMax = 8;                         // FDH_DAMAGE_MOVES_MAX
constexpr int kDamageShiftMax = 256;                       // FDH_DAMAGE_SHIFT_MAX
constexpr int kDamageVoteSpan = 2 * kDamageShiftMax + 1;   // a counter per d in [-256, 256], at d + 256

// the caller's moves, in its order: tile (x, y) now holds what (x + dx, y + dy) held
struct DamageMoveList {
  int n;
  int16_t dx[kDamageMovesMax], dy[kDamageMovesMax];
};

// k_damage_move_match: the launch in front of k_damage_filter in a moved read (the filter overwrites the mirror in place: the image the
// receiver holds exists only until then).  k_damage_pack's shape; a pending bin's workgroup compares its tile, as the surface holds it,
// with the mirror's rectangle at each move whose source lies inside the frame, and leaves moved[bin] = the first matching move's
// index + 1, or 0.  It writes nothing else.
struct DamageMoveMatchParams {
  const uint32_t* surf;    // the frame surface, pitch W pixels
  const uint32_t* mirror;  // [bin][64][64]
  const uint32_t* stamp;   // [bin]
  uint8_t* moved;          // [bin]
  DamageMoveList moves;
  uint32_t epoch;
  int W, H, bins_x, bins_y, all;
};
void launch_damage_move_match(hipStream_t s, const DamageMoveMatchParams& P);

// k_damage_encode_moved: k_damage_encode for a moved read.  A pending bin with moved[bin] != 0 whose tile is not one colour stores a COPY
// entry and claims no payload space; every other bin is coded as k_damage_encode codes it.  *cursor (one 64-bit word, zeroed in stream
// order before the launch) takes ONE add per workgroup: the bytes claimed so far / 16 in bits 0 .. 27, the COPY tiles in bits 28 .. 45,
// the arrivals in bits 46 .. 63 (a grid has fewer than 2^18 bins and a blob fewer than 2^32 bytes: fdh_read_damage_coded's limits).
// Whoever arrives last of the n_pending leaves *payload_bytes and *n_copied.
struct DamageEncodeMovedParams {
  DamageEncodeParams enc;
  const uint8_t* moved;    // [bin]: k_damage_move_match's
  DamageMoveList moves;
  uint32_t* n_copied;
};
void launch_damage_encode_moved(hipStream_t s, const DamageEncodeMovedParams& P);

// k_damage_move_votes: the mover.  Workgroups walk the pending bins whose tile is whole; each such bin's row 32 and column 32 of the
// surface are compared with the mirror's rows / columns at every shift d in [-max_shift, max_shift], d != 0, that stays inside the frame
// (a probe whose 64 pixels are all equal does not vote).  votes[0][d + 256] counts the bins whose vertical probe equals the mirror's row
// y0 + 32 + d, votes[1][d + 256] those whose horizontal probe equals its column x0 + 32 + d.  Accumulated in LDS per workgroup, then
// added to `votes` (device memory, zeroed in stream order before the launch).  Reads only.
struct DamageMoveVotesParams {
  const uint32_t* surf;
  const uint32_t* mirror;
  const uint32_t* stamp;
  uint32_t* votes;         // [2][kDamageVoteSpan]
  uint32_t epoch;
  int W, H, bins_x, bins_y, all, max_shift;
};
void launch_damage_move_votes(hipStream_t s, const DamageMoveVotesParams& P);

#if defined(__device__)
// pixel (x, y) of the frame the mirror holds (inside the frame: the words past a clipped tile's edge are not pixels)
__device__ __forceinline__ uint32_t mirror_px(const uint32_t* __restrict__ mirror, int bins_x, int x, int y) {
  return mirror[((size_t)((y >> 6) * bins_x + (x >> 6)) << 12) + (size_t)(((y & 63) << 6) + (x & 63))];
}
#endif

}  // namespace fdh
