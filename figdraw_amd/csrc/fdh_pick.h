// fdh_pick.h -- the hit-testing kernels' parameter block and launchers (k_pick.hip; include/figdraw_hip_pick.h is the public side).
#pragma once
#include <hip/hip_runtime.h>

#include "fdh_types.h"

namespace fdh {

// A pick launch: one 256-thread workgroup per 16 x 16-pixel tile.  Region queries: a tile of the rectangle per workgroup, one thread per
// pixel.  Point queries: the points sorted by tile on the host, one workgroup per tile that holds any, one thread per point.
constexpr int kPickTile = 16;
constexpr int kPickThreads = kPickTile * kPickTile;  // 256: four waves
constexpr int kPickDepth = 16;                       // clip levels kept per thread in LDS; deeper ones go to `spill`
constexpr int kPickWindow = 512;                     // 64-record chunks whose survivor masks a workgroup holds at once (4 KB of LDS)
constexpr uint32_t kPickShadows = 1u;                // FDH_PICK_SHADOWS
struct PickParams {
  const DrawRec* draws;      // the frame's records, painter's order (the frame block the frame left on the device)
  const QuadExt* exts;
  const int* phase_first;    // [n_phases + 1]: the clip stack starts empty at every phase (open clips are re-emitted)
  int n_phases, n_recs;
  AtlasView atlas;
  int W, H;                  // the frame
  int threshold;             // a hit: rint(255 a) >= threshold
  uint32_t flags;            // kPickShadows
  // region queries (region_out != null): pixels [x0, x0 + w) x [y0, y0 + h), tiles_x tiles per row; out[h][w] = the front-most hit, -1
  int x0, y0, w, h, tiles_x;
  int32_t* region_out;
  // point queries: pts[i] = pixel (x, y) (x < 0: outside the frame), sorted by tile; workgroup b takes pts[tile_first[b] .. tile_first[b + 1])
  // (at most 256 per entry: the host splits fuller tiles) and the 16 x 16 tile at tile_xy[b]
  const int2* pts;
  const int* tile_first;
  const int2* tile_xy;
  int max_hits;
  uint2* hits;               // [point][max_hits]: a ring of the last max_hits hits in painter's order, {draw, alpha | mode << 8}
  int* hit_count;            // [point]: hits seen (the ring holds the last min(count, max_hits))
  uint8_t* spill;            // clip levels >= kPickDepth: [level - kPickDepth][workgroup * 256 + thread], or null
};
void launch_pick(hipStream_t s, const PickParams& P, int n_groups, int spill_levels);  // spill_levels: levels `spill` holds

}  // namespace fdh
