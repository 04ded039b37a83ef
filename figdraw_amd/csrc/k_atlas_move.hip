// k_atlas_move.hip -- fdh_compact_atlas (the specification: include_glyphs/figdraw_hip_atlas.h): rectangles of texels from the levels of the
// old atlas into the levels of the new one, ONE launch for all rectangles of all levels, whatever their number.  The two atlases travel in
// the kernel arguments (move::Views); the grid is 1-D over the tile table (fdh_atlas_move.h), a workgroup is one wave, and a tile is a part
// of one record's rectangle: 8 x 8 texels, or for a rectangle at least move::kWideFrom wide 64 x 4 -- a lane per texel of a row, so that a
// wave stores 256 contiguous bytes per row, four rows one after the other.  A record that shares texels with a later rectangle of its
// destination level has owner bits, and stores only where its bit is set.  Either end of a record may be the launch's dense buffer in
// place of a level: level 0 of every image goes there for the level chain, the kept levels of fdh_put_image_mips entries come from there.
// Source and destination are different allocations: nothing overlaps.  No LDS, no cross-lane operation: a lane reads a word and stores it.
#include "fdh_device.h"
#include "fdh_atlas_move.h"

namespace fdh {

__device__ __forceinline__ void atlas_move_texel(const move::Views& V, const move::Record& r, const uint32_t* __restrict__ owner, int i, int j) {
  if (i >= r.w || j >= r.h) return;
  if (r.owner_off != move::kNoOwner) {
    const uint32_t bit = r.owner_off + (uint32_t)(j * r.w + i);
    if (!((owner[bit >> 5] >> (bit & 31u)) & 1u)) return;
  }
  // a texel outside either level is dropped, as every blit into the atlas drops it
  const uint32_t* src;
  if (r.src_level == move::kBuffer) {
    src = V.buf_in + (size_t)(uint32_t)r.sx + (size_t)j * r.w + i;
  } else {
    const int LS = V.from_size >> r.src_level, x = r.sx + i, y = r.sy + j;
    if (r.src_level < 0 || r.src_level >= V.from_levels || x < 0 || y < 0 || x >= LS || y >= LS) return;
    src = V.from[r.src_level] + (size_t)y * LS + x;
  }
  uint32_t* dst;
  if (r.dst_level == move::kBuffer) {
    dst = V.buf_out + (size_t)(uint32_t)r.dx + (size_t)j * r.w + i;
  } else {
    const int LS = V.to_size >> r.dst_level, x = r.dx + i, y = r.dy + j;
    if (r.dst_level < 0 || r.dst_level >= V.to_levels || x < 0 || y < 0 || x >= LS || y >= LS) return;
    dst = V.to[r.dst_level] + (size_t)y * LS + x;
  }
  *dst = *src;
}
__global__ __launch_bounds__(64) void k_atlas_move(move::Views V, const move::Record* __restrict__ records, const uint32_t* __restrict__ tile_record,
                                                   const uint32_t* __restrict__ owner) {
  const move::Record r = records[tile_record[blockIdx.x]];
  const int tile = (int)(blockIdx.x - r.first_tile), lane = (int)threadIdx.x;
  if (r.wide) {
    const int tiles_x = (r.w + 63) / 64, ty = tile / tiles_x, tx = tile - ty * tiles_x;
#pragma unroll
    for (int k = 0; k < 4; k++) atlas_move_texel(V, r, owner, tx * 64 + lane, ty * 4 + k);
  } else {
    const int tiles_x = (r.w + 7) / 8, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    atlas_move_texel(V, r, owner, tx * 8 + (lane & 7), ty * 8 + (lane >> 3));
  }
}
void launch_atlas_move(hipStream_t s, const move::Views& V, const move::Record* records, const uint32_t* tile_record, int n_tiles, const uint32_t* owner) {
  if (n_tiles > 0) FDH_LAUNCH(k_atlas_move, dim3(n_tiles), dim3(64), 0, s, V, records, tile_record, owner);
}

}  // namespace fdh
