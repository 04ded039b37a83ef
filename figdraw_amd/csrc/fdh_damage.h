// fdh_damage.h -- damage tracking (fdh_set_damage_tracking) and damage readback: the blur rule, ONE definition for the host
// (fdh_damage_closure, the CPU tests) and the device (k_damage_resolve, k_damage.hip), the parameter blocks and launchers of the tracking
// launches, the pending set's rule, and the host-only functions of fdh_damage.cpp.  The read kernels' blocks are fdh_damage_read.h's.
//
// A bin's pixels are a function of its (phase, bin) lists, the content of every listed draw and the frame-level state the host hashes
// into its frame key -- except where a backdrop blur reads them: a blurred pixel depends on the PHASE-k intermediate over the node's
// footprint F grown by the tap reach r, and outside the damage that intermediate is not rebuilt.  So the damage must be closed under
// the blur's reads: a node whose bin-rounded F (+) r meets a damaged bin turns all of F (+) r into damage, to a fixed point over the
// frame's nodes (one node's region can reach another's).  The closure is the LEAST set that contains the changed bins and is closed
// under that rule, so the host's serial walk and the device's parallel one reach the same set whatever order they visit nodes in.
#pragma once
#include <stdint.h>

#include "fdh_kernels.h"
#include "fdh_damage_read.h"  // the read kernels: k_damage_pack, k_damage_encode
#include "fdh_damage_move.h"  // moved damage readback: k_damage_move_match, k_damage_encode_moved, k_damage_move_votes

struct FdhDamageTile;  // include/figdraw_hip_readback.h
struct FdhCodedTile;   // include/figdraw_hip_stream.h

#if defined(__HIPCC__)
#define FDH_HD __host__ __device__
#else
#define FDH_HD
#endif

namespace fdh {

constexpr int kDamageMaxNodes = 64;   // blur nodes a tracked frame may hold (more: the frame is rendered in full)
constexpr int kDamageMaxPhases = BinParams::kBinSubs;  // (k_damage_sign reads phase boxes of the bin launch's sub-grids)

struct DamageRegion { int bx0, by0, bx1, by1; };  // bins [bx0, bx1) x [by0, by1) of the grid; empty when bx1 <= bx0 or by1 <= by0

FDH_HD inline int damage_floor_div(int v, int d) { return v >= 0 ? v / d : -((-v + d - 1) / d); }

// The bins a blur node's output depends on: its footprint [x0, x1) x [y0, y1) (pixels) grown by the tap reach on every side, rounded
// out to whole bins and clipped to the bins_x x bins_y grid.  An empty footprint reads nothing (the launch skips such a node).
FDH_HD inline DamageRegion damage_region(int x0, int y0, int x1, int y1, int reach, int bins_x, int bins_y) {
  DamageRegion r{0, 0, 0, 0};
  if (x1 <= x0 || y1 <= y0) return r;
  const int bx0 = damage_floor_div(x0 - reach, kBin), by0 = damage_floor_div(y0 - reach, kBin);
  const int bx1 = damage_floor_div(x1 + reach - 1, kBin) + 1, by1 = damage_floor_div(y1 + reach - 1, kBin) + 1;
  r.bx0 = bx0 < 0 ? 0 : bx0; r.by0 = by0 < 0 ? 0 : by0;
  r.bx1 = bx1 > bins_x ? bins_x : bx1; r.by1 = by1 > bins_y ? bins_y : by1;
  if (r.bx1 <= r.bx0 || r.by1 <= r.by0) r = DamageRegion{0, 0, 0, 0};
  return r;
}

// The rule, ONE definition for both sides: mask (bins_y x bins_x, row-major, 0 / 1) is closed in place; run[k] = 1 for every node whose
// region took damage (the caller zeroes run[0 .. n)).  `team` is who runs it: on the host one thread (DamageHostTeam), in
// k_damage_resolve the workgroup (its members split each region's bins; any() is the workgroup's vote, sync() its barrier).  The order the
// nodes are visited in does not change the result: it is the least set that holds the changed bins and is closed under the rule.
template <typename Team>
FDH_HD inline void damage_close(uint8_t* mask, int bins_x, const DamageRegion* reg, int n, uint8_t* run, const Team& team) {
  bool grew = true;
  while (grew) {
    grew = false;
    for (int k = 0; k < n; k++) {
      if (run[k]) continue;
      const DamageRegion r = reg[k];
      const int rw = r.bx1 - r.bx0, rn = rw * (r.by1 - r.by0);
      int any = 0;
      for (int i = team.rank(); i < rn; i += team.size()) any |= mask[(r.by0 + i / rw) * bins_x + r.bx0 + i % rw];
      if (!team.any(any)) continue;
      for (int i = team.rank(); i < rn; i += team.size()) mask[(r.by0 + i / rw) * bins_x + r.bx0 + i % rw] = 1;
      if (team.rank() == 0) run[k] = 1;
      grew = true;
      team.sync();
    }
  }
}
struct DamageHostTeam {
  int rank() const { return 0; }
  int size() const { return 1; }
  bool any(int v) const { return v != 0; }
  void sync() const {}
};

// k_damage_sign: one wave per bin folds an order-dependent 64-bit signature of the bin's lists over every phase -- per entry its
// phase, its position, its two words and the content of what the compositor reads for it (the 128-byte DrawRec and, for a general
// quad, its 208-byte QuadExt) --, compares it with the bin's signature of the previous frame and replaces it.
struct DamageSignParams {
  const uint2* lists;      // [phase][bin][stride]
  const uint32_t* counts;  // [phase][bin]
  const DrawRec* draws;
  const QuadExt* exts;
  uint64_t* sig;           // [bin]: the previous frame's signatures in, this frame's out
  uint8_t* changed;        // [bin]: 1 where the signature differs (every bin when `force`)
  int n_phases, bins_x, bins_y, stride, n_draws, n_exts, force;
  // the bins each phase's lists are valid for (k_bin_draws' sub-grids); sub_n = 0: every phase has the whole grid
  int sub_n;
  int sub_x0[kDamageMaxPhases], sub_y0[kDamageMaxPhases], sub_nx[kDamageMaxPhases], sub_ny[kDamageMaxPhases];
  // The frame's blur nodes: a node whose V pass composites its quad itself has no entry in any list, so every bin of its (bin-rounded)
  // footprint also folds in the node's key (its phase, footprint, radius, route) -- a node that moves, changes or vanishes changes the
  // signatures of the bins it covered and of those it covers.
  int n_nodes;
  DamageRegion foot[kDamageMaxNodes];
  uint64_t node_key[kDamageMaxNodes];
};
// k_damage_resolve: ONE workgroup.  changed -> mask (the blur rule), the compact list of damaged bins and its length, run[] per node.
struct DamageResolveParams {
  const uint8_t* changed;
  uint8_t* mask;           // [bin] 0 / 1: what fdh_damage_bins reports
  int* list;               // [bin]: the damaged bins (row-major index), count[0] of them, in no particular order
  uint32_t* count;
  uint8_t* run;            // [node]
  int bins_x, bins_y, n_nodes;
  DamageRegion reg[kDamageMaxNodes];
};

void launch_damage_sign(hipStream_t s, const DamageSignParams& P);
void launch_damage_resolve(hipStream_t s, const DamageResolveParams& P);
// A node whose V pass composites its quad straight into the frame surface (BlurJob::fuse_draw >= 0) runs whether its region took
// damage or not; when it did not, these two bracket it: save copies the footprint rows [y0, y1) x [x0, x1) of `surf` to `keep`, restore
// copies them back -- both return at once when run[node] is set.
void launch_damage_guard(hipStream_t s, const uint8_t* run, int node, bool restore, uint32_t* surf, uint32_t* keep, int pitch, int x0, int y0,
                         int x1, int y1);
// The compositor launch of a tracked frame (k_composite_damage, k_composite.hip): P as launch_composite takes it, its waves walk the
// strips of list[0 .. count[0]) that lie in P's bin box; `grid` waves in all (one per strip of the frame: those beyond the list exit).
void launch_composite_damage(hipStream_t s, const DrawRec* draws, const QuadExt* exts, CompositeParams P, const int* list, const uint32_t* count,
                             int grid);

// Damage readback (include/figdraw_hip_readback.h).  The pending set is a stamp per bin: a bin is pending when stamp[bin] == epoch, the
// number of the read that will fetch it.  A read moves the epoch on, which empties the set without a store (no launch clears a mask that
// other workgroups of the pack are still counting).
// k_damage_accumulate: ONE workgroup, after k_damage_resolve: stamps the bins of the frame's mask and leaves the number of pending bins
// in *n_pending (page-locked host memory: the host reads it after the stream's synchronise and launches nothing when it is 0).
void launch_damage_accumulate(hipStream_t s, const uint8_t* mask, uint32_t* stamp, uint32_t epoch, int bins, uint32_t* n_pending);

// Host only (fdh_damage.cpp; the decoder itself is fdh_tile_decode.cpp): what fdh_damage_closure, fdh_apply_damage, fdh_decode_damage,
// fdh_decode_damage_moved and fdh_coded_damage_bound run.
void damage_closure(const uint8_t* changed, int bins_x, int bins_y, const int* rects, const float* radii, int n_nodes, uint8_t* out);
void apply_damage(uint8_t* image, int64_t pitch_bytes, int w, int h, const FdhDamageTile* tiles, const uint8_t* pixels, int n_tiles);
void decode_damage(uint8_t* image, int64_t pitch_bytes, int w, int h, const FdhCodedTile* tiles, int n_tiles, const uint8_t* payload, int64_t payload_bytes);
void decode_damage_moved(uint8_t* image, int64_t pitch_bytes, int w, int h, const FdhCodedTile* tiles, int n_tiles, const uint8_t* payload, int64_t payload_bytes);
int64_t coded_damage_bound(int w, int h);

}  // namespace fdh
