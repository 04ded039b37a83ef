// fdh_damage_read.h -- damage readback's read kernels (k_damage_pack in k_damage.hip, k_damage_encode in k_damage_codec.hip, and
// k_damage_filter in k_damage_filter.hip, which runs in front of either): their parameter blocks, and the device code they share.  Included through fdh_damage.h; it names nothing but kBin, the vector types and
// hipStream_t, so the host shim of tests/codec_emu compiles against this very file.
#pragma once
#include <stdint.h>
#if defined(__HIP__)  // (the library's build; the host shim defines kBin, the vector types and hipStream_t itself before it includes this file)
#include <hip/hip_runtime.h>

#include "fdh_types.h"
#endif

namespace fdh {

// k_damage_pack: a workgroup per bin.  A pending bin's rank among the pending bins in row-major order is its slot: tiles[rank] = the
// bin clipped to the frame (x, y, w, h), slot rank of `pixels` (16 KB: 64 rows of 256 bytes) = its pixels, zeros past the tile's edge.
// `all`: every bin is pending whatever its stamp.  The last bin's workgroup leaves the number of tiles in *n_tiles.
struct DamagePackParams {
  const uint32_t* surf;    // the frame surface, pitch W pixels
  const uint32_t* stamp;   // [bin]
  uint8_t* pixels;         // [tile][64][256], 16-byte aligned
  int4* tiles;             // [tile]
  uint32_t* n_tiles;
  uint32_t epoch;
  int W, H, bins_x, bins_y, all;
};
void launch_damage_pack(hipStream_t s, const DamagePackParams& P);
// k_damage_encode (include/figdraw_hip_stream.h is the format): k_damage_pack's shape, but a pending bin's workgroup codes its tile in
// the cheapest of the four modes, claims the payload's space (its size rounded up to 16 bytes) with one atomic add on *cursor (device
// memory, zeroed in stream order before the launch) and stores entry and payload.  The workgroup that makes the last of the n_pending
// claims leaves the blob's size in *payload_bytes.
struct DamageEncodeParams {
  const uint32_t* surf;    // the frame surface, pitch W pixels
  const uint32_t* stamp;   // [bin]
  uint8_t* payload;        // bins * 16384 bytes, 16-byte aligned
  uint2* dir;              // [tile] FdhCodedTile, 24 bytes each
  uint32_t* n_tiles;
  uint32_t* payload_bytes;
  unsigned long long* cursor;
  uint32_t epoch, n_pending;
  int W, H, bins_x, bins_y, all;
};
void launch_damage_encode(hipStream_t s, const DamageEncodeParams& P);
// k_damage_filter (k_damage_filter.hip; include/figdraw_hip_exact.h): the launch in front of either read when exact damage readback is
// on.  k_damage_pack's shape; a pending bin's workgroup compares its tile with the mirror's -- the frame as the application last read it,
// tile-major: slot `bin` is k_damage_pack's slot of that bin, zeros past the tile's edge -- and leaves the bin pending (stamp = epoch)
// with the mirror updated when they differ, not pending (stamp = epoch - 1) when they are equal.  Each workgroup reads and writes its
// own stamp only.  `all`: every bin is pending whatever its stamp, and every bin's stamp is written.  The workgroup that is the last of
// the n_pending to arrive at *arrivals (device memory, zeroed in stream order before the launch) leaves the number of bins that stay
// pending in *n_changed.  `fill`: no compare, no stamp, no count -- every tile is stored into the mirror (with `all`: a fresh read).
struct DamageFilterParams {
  const uint32_t* surf;    // the frame surface, pitch W pixels
  uint32_t* mirror;        // [bin][64][64], 16-byte aligned
  uint32_t* stamp;         // [bin]
  unsigned long long* arrivals;
  uint32_t* n_changed;
  uint32_t epoch, n_pending;
  int W, H, bins_x, bins_y, all, fill;
};
void launch_damage_filter(hipStream_t s, const DamageFilterParams& P);

#if defined(__device__)  // (a macro under hipcc and under the shim)
// the workgroup's sum of v (every thread gets it); part holds a word per wave.  kReuse: the caller writes part again afterwards, so a
// barrier follows the reads
template <bool kReuse>
__device__ __forceinline__ uint32_t workgroup_sum(uint32_t v, uint32_t* part) {
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) v += __shfl_xor(v, sh, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t sum = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); w++) sum += part[w];
  if (kReuse) __syncthreads();
  return sum;
}

// A read's workgroup finds its slot: the pending bins ahead of `bin` in row-major order (`all`: every bin is pending whatever its
// stamp).  The last bin's workgroup stores the number of tiles.  False: the bin is not pending, the workgroup leaves.
template <int kThreads, bool kReuse>
__device__ __forceinline__ bool pending_slot(const uint32_t* __restrict__ stamp, uint32_t epoch, int all, int bin, int nb, uint32_t* n_tiles,
                                             uint32_t* part, uint32_t& slot) {
  const int t = (int)threadIdx.x;
  const bool last = bin == nb - 1;
  const bool mine = all || stamp[bin] == epoch;
  if (!mine && !last) return false;
  slot = (uint32_t)bin;
  if (!all) {
    uint32_t c = 0;
    for (int b = t; b < bin; b += kThreads) c += stamp[b] == epoch ? 1u : 0u;
    slot = workgroup_sum<kReuse>(c, part);
  }
  if (last && t == 0) n_tiles[0] = slot + (mine ? 1u : 0u);
  return mine;
}

// a bin clipped to the frame
struct TileBox { int x0, y0, w, h; };
__device__ __forceinline__ TileBox tile_box(int bin, int bins_x, int W, int H) {
  const int by = bin / bins_x, bx = bin - by * bins_x;
  const int x0 = bx * kBin, y0 = by * kBin;
  return TileBox{x0, y0, min(kBin, W - x0), min(kBin, H - y0)};
}

// The walk both kernels load a tile by: 64 rows of 16 16-byte words, kBin * kBin / 4 / kThreads per thread; consecutive threads take consecutive
// words of a surface row.  word(i, r, c, inside, src): word i = pixels c .. c + 3 of row r, the first of them at src; `inside`: the tile
// holds that one at least (else src is not to be read).
template <int kThreads, typename Word>
__device__ __forceinline__ void tile_walk(const uint32_t* __restrict__ surf, int W, const TileBox b, Word word) {
#pragma unroll
  for (int k = 0; k < kBin * kBin / 4 / kThreads; k++) {
    const int i = (int)threadIdx.x + k * kThreads;
    const int r = i >> 4, c = (i & 15) * 4;
    word(i, r, c, r < b.h && c < b.w, surf + (size_t)(b.y0 + r) * W + b.x0 + c);
  }
}
#endif

}  // namespace fdh
