// fdh_damage_host.h -- the host side of damage tracking and damage readback (fdh_damage.cpp): two components of a device context, each one
// member of Context.  The context hands them its stream, the frame's LaunchJob and surface, and profile mode's bracket around a launch
// of the bin kind (span(true) before it, span(false) after); they do not know the context.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/figdraw_hip_readback.h"  // FdhDamageTile
#include "../../include/figdraw_hip_stream.h"    // FdhCodedTile
#include "../../include_readback/figdraw_hip_moves.h"  // FdhDamageMove
#include "fdh_frame.h"    // LaunchJob
#include "fdh_kernels.h"  // BinParams, CompositeParams
#include "fdh_memory.h"   // DeviceBuf, PinnedBuf

namespace fdh {

using LaunchSpan = std::function<void(bool)>;
struct DamageReadback;
struct DamageMoveList;  // fdh_damage_move.h
// Damage tracking (include/figdraw_hip_damage.h; submission side but for `on`): the per-bin signatures of the last tracked frame, what its
// resolve left, and the footprint a fused V pass of a node that did not run writes over (k_damage_guard).
struct DamageTracker {
  bool on = false;                   // (calling thread: fdh_set_damage_tracking)
  bool valid = false, last = false;  // the surface holds the frame of key `key` and the signatures are that frame's; the last launch was tracked
  uint64_t key = 0;
  int bins_x = 0, bins_y = 0;        // the grid the mask belongs to
  DeviceBuf<uint64_t> sig;
  DeviceBuf<uint8_t> changed, mask, run;
  DeviceBuf<int> list;
  DeviceBuf<uint32_t> count, keep;
  // a frame's sign + resolve launches, behind its bin launch (B); its mask joins rb's pending set.  true: a partial frame
  bool launch(hipStream_t s, const LaunchJob& J, const BinParams& B, DamageReadback& rb, const LaunchSpan& span);
  void launched_whole(const LaunchJob& J);  // every launch of the frame is enqueued: the signatures are its
  // the pair around the fused V pass of J's blur node `node` in a partial frame (rows y0 .. y1 of its footprint, in `surf`)
  void guard(hipStream_t s, const LaunchJob& J, int node, bool restore, uint32_t* surf, int y0, int y1) const;
  void composite(hipStream_t s, const LaunchJob& J, const CompositeParams& C) const;  // a partial frame's compositor launch, over the list
  std::vector<uint8_t> bins(int gx, int gy, bool changed_only) const;  // fdh_damage_bins' mask of the last frame (the stream is idle)
  void release();
};
// what a read needs of the context, whose stream is idle: the surface, size and grid of the last frame
struct ReadFrame { hipStream_t stream; const uint32_t* surf; int W, H, bins_x, bins_y; };
// Damage readback (include/figdraw_hip_readback.h, figdraw_hip_stream.h, figdraw_hip_exact.h): the pending set (fdh_damage.h), the
// page-locked buffers the reads return and, in exact mode, the device mirror of what the application holds.  `all`, `epoch`, `w`, `h`: written by whoever launches a frame (the submit thread, or replay's caller after a drain)
// and by a read, which runs after the context's drain.
struct DamageReadback {
  bool on = false;     // (calling thread: fdh_set_damage_readback)
  bool all = true;     // every bin is pending whatever the stamps say
  uint32_t epoch = 1;  // the stamp of a pending bin
  int w = 0, h = 0;    // the frame size the stamps describe
  DeviceBuf<uint32_t> stamp, cursor;   // [bin]; k_damage_encode's claim counter
  volatile uint32_t* count = nullptr;  // pinned words: pending bins after the last k_damage_accumulate; tiles of the last read; a coded read's payload bytes; [3] the filter's count; [4] a moved read's COPY tiles
  PinnedBuf<uint8_t> pixels, code;     // what the reads return: [tile][64][256] with its tiles; the coded payload with its directory
  PinnedBuf<FdhDamageTile> tiles;
  PinnedBuf<FdhCodedTile> dir;
  // exact mode (fdh_set_damage_exact; acts while `on`): the frame as of the last read, tile-major [bin][64][64], valid for a frame of
  // mirror_w x mirror_h; k_damage_filter's arrival counter; what fdh_damage_exact_stats tells of the last read
  bool exact = false, mirror_valid = false, have_stats = false;
  int mirror_w = 0, mirror_h = 0;
  DeviceBuf<uint32_t> mirror;
  DeviceBuf<unsigned long long> arrivals;
  int stat_pending = 0, stat_changed = 0, stat_fresh = 0;
  // moved reads (include_readback/figdraw_hip_moves.h; need exact mode): k_damage_move_match's answer per bin; the mover's counters
  DeviceBuf<uint8_t> moved;
  DeviceBuf<uint32_t> votes;
  void turn(bool on_now, hipStream_t s);
  void turn_exact(bool on_now, hipStream_t s);
  void exact_stats(int* n_pending, int* n_changed, int* fresh) const;
  void frame_whole() { if (on) all = true; }  // the frame composited every bin: no mask to accumulate, and no launch
  void accumulate(hipStream_t s, const LaunchJob& J, const uint8_t* mask, const LaunchSpan& span);  // a tracked frame's mask joins the set
  int pending(const char* who, const ReadFrame& F, bool* every) const;  // what a read starts with: this many bins of F are pending
  void consumed(const ReadFrame& F);  // ... and ends with: the set is empty, the stamps are laid out for F's grid
  // exact mode's step between pending() and fetch(): n bins of F are pending (`*every`: all of them, whatever the stamps say) -> the
  // number that stay pending, which the stamps then hold (*every = false).  A fresh read fills the mirror and returns n.  Mode off: n.
  int filter(const char* who, const ReadFrame& F, int n, bool* every);
  void lost();  // exact mode: a read failed after the filter ran -- the mirror is invalid, every bin is pending
  // the one read routine: pending(), filter(), fetch().  Returns the tile count.
  int read(const char* who, const ReadFrame& F, int64_t* payload_bytes);
  // its last step, over n > 0 pending bins: k_damage_pack into pixels / tiles, or (`payload_bytes`) k_damage_encode into code / dir; consumed()
  // (`moves`: a moved read -- k_damage_encode_moved against moved[], and count[4] = the COPY tiles)
  int fetch(const char* who, const ReadFrame& F, int n, bool every, int64_t* payload_bytes, const DamageMoveList* moves = nullptr);
  // fdh_read_damage_moved: the coded read with k_damage_move_match in front of the filter and k_damage_encode_moved behind it -- one launch
  // more than a coded exact read, and no synchronise more
  void read_moved(const ReadFrame& F, const FdhDamageMove* moves, int n_moves, const FdhCodedTile** t, const uint8_t** payload, int* n_tiles,
                  int64_t* payload_bytes, int* frame_w, int* frame_h, int* full, int* n_copied);
  // fdh_find_damage_moves: k_damage_move_votes over the pending set as it stands, and the sort of its counters
  void find_moves(const ReadFrame& F, int max_shift, FdhDamageMove* out_moves, int* out_votes, int cap, int* n_out);
  // fdh_read_damage, fdh_read_damage_coded, fdh_read_damage_into
  void read_raw(const ReadFrame& F, const FdhDamageTile** t, const uint8_t** px, int* n_tiles, int* frame_w, int* frame_h, int* full);
  void read_coded(const ReadFrame& F, const FdhCodedTile** t, const uint8_t** payload, int* n_tiles, int64_t* payload_bytes, int* frame_w, int* frame_h, int* full);
  void read_into(const ReadFrame& F, uint8_t* image, int64_t pitch_bytes, int iw, int ih, int* n_tiles);
  void release();  // (the stream is idle)
};

}  // namespace fdh
