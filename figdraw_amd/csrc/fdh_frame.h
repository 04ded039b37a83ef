// fdh_frame.h -- the recorded frame and its launch description: a phase and its blur node, the lane one thread records into, the pieces
// that put the lanes' records into painter's order, the layout of the frame's device block, and the LaunchJob the submit side works from.
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>
#include <vector>

#include "fdh_kernels.h"
#include "fdh_plain.h"   // PhaseFlags, PhaseSum, PickTag
#include "fdh_memory.h"

namespace fdh {

struct Phase : PhaseFlags {  // (fdh_plain.h: has_masks, has_atlas, has_slow, has_slow_atlas, has_rot)
  int first = 0, count = 0;
  int blur = -1;  // index into blurs: executed before this phase's composite
  int bin_x0 = 0, bin_y0 = 0, bin_x1 = 0, bin_y1 = 0;  // bins touched by the phase's draws
};
struct BlurJob {
  float radius;
  int x0, y0, x1, y1;  // footprint: the mode-17 quad's pixel bounds
  int fuse_draw;       // record index of the consuming mode-17 quad when k_blur_v composites it, else -1
  BlurTaps taps;
};

// ------------------------------------------------------------------ the recorded frame
// A frame's draw records are produced in their FINAL form while the calls arrive -- the 128-byte DrawRec the compositor reads,
// the 32-byte BinRec the bin kernel reads (pixel bounds, saturated core, list-entry flags), the quad extensions: nothing is
// built a second time at submit.  A LANE is what one thread records: lane 0 belongs to the thread that calls the context,
// lanes 1.. to the walk pool's threads (fdh_frontend.cpp: large sibling groups of the scene tree are decomposed in parallel).
// (PickTag, a record's tag in a picking frame: fdh_plain.h)
// The frame in painter's order is a list of PIECES, each a run of consecutive records of one lane.  A finished piece is
// PUBLISHED -- copied, by the thread that recorded it, into the lane's pinned mirror arrays -- and the upload kernel gathers the
// published pieces into the dense device arrays (k_upload_frame).
struct Lane {
  HostVec<DrawRec> recs;
  HostVec<BinRec> bins;   // bins[i].box IS the bounds of record i (clip pushes: the union of their content, final at the pop)
  HostVec<QuadExt> exts;  // DrawRec::ext of an F_GENERAL record indexes THIS array; the upload re-bases it
  HostVec<uint32_t> boxes;  // the records' 4-byte bin boxes (what k_bin_draws scans; the device derives its own from the BinRecs):
                            // kept here for the chunk boxes -- the union box of every 256 draws -- which Context::build_misc builds over the pieces
  HostVec<DrawRec> up_recs;  // pinned mirrors (device contexts): what the GPU reads; element i = element i of the array above
  HostVec<BinRec> up_bins;
  HostVec<QuadExt> up_exts;
  HostVec<PickTag> tags;    // picking frames only: tags[i] = the tag of record i (host memory, never uploaded)
  bool device = false;
  const uint8_t *d_recs = nullptr, *d_bins = nullptr, *d_exts = nullptr;  // the mirrors as the device sees them (taken when a mirror is allocated)
  size_t pub_recs = 0, pub_exts = 0;  // elements below these may have been published this frame (kept across a mirror's growth)
  // List stride (the largest number of list entries any bin of any phase can receive: it sizes the bin lists): a 2-D difference
  // array over the bin grid, four updates per record when its bounds are final, evaluated per phase (count_close).
  std::vector<int> diff;
  int dw = 0, dh = 0;
  int tx0 = 0, ty0 = 0, tx1 = 0, ty1 = 0;
  bool touched = false;
  uint64_t stamp = 0;  // the frame a pool thread's lane was last cleared for
  void set_pinned(bool on, int dev) {
    device = on;
    up_recs.pinned = up_bins.pinned = up_exts.pinned = on;
    up_recs.vram = up_bins.vram = up_exts.vram = on && vram_staging(dev);
    up_recs.dev = up_bins.dev = up_exts.dev = dev;
  }
  void clear() { recs.clear(); bins.clear(); exts.clear(); boxes.clear(); tags.clear(); pub_recs = pub_exts = 0; }
  void publish(uint32_t first, uint32_t n, uint32_t ext_first, uint32_t n_ext);  // records / extensions are final: copy them to the mirrors
  void publish_bytes(int array, size_t at, size_t len);                          // ... a byte range of one array (0 recs, 1 bins, 2 exts)
  void count_begin(int bins_x, int bins_y);
  void count_add(const BBox& b);
  int count_close();  // the largest count of any bin since the last close; leaves the array zeroed
};

// (in the header: once per record on the record path, inlined into Recorder::commit_bins)
inline void Lane::count_add(const BBox& b) {
  if (bbox_empty(b)) return;
  constexpr int kBinShift = 6;
  static_assert((1 << kBinShift) == kBin, "bins are 64 px");
  const int bx0 = b.x0 >> kBinShift, by0 = b.y0 >> kBinShift, bx1 = ((b.x1 - 1) >> kBinShift) + 1, by1 = ((b.y1 - 1) >> kBinShift) + 1;  // [bx0,bx1) x [by0,by1)
  if (bx1 >= dw || by1 >= dh) return;  // (bounds are clipped to the frame: cannot happen)
  int* d = diff.data();
  d[(size_t)by0 * dw + bx0]++; d[(size_t)by0 * dw + bx1]--; d[(size_t)by1 * dw + bx0]--; d[(size_t)by1 * dw + bx1]++;
  if (!touched) { tx0 = bx0; ty0 = by0; tx1 = bx1; ty1 = by1; touched = true; }
  else { tx0 = std::min(tx0, bx0); ty0 = std::min(ty0, by0); tx1 = std::max(tx1, bx1); ty1 = std::max(ty1, by1); }
}

struct Piece {
  int lane = 0;                     // (-1: the lane Context::consolidate_pieces copies a frame of too many pieces into)
  uint32_t first = 0, n = 0;        // records [first, first + n) of the lane
  uint32_t ext_first = 0, n_ext = 0;  // their quad extensions
};

// The frame as it is being recorded (calling thread): kStaging sets of lanes in rotation, the pieces that put the current set's records
// into painter's order, the phases and their blur nodes, and what a frame's launch is sized by (list stride, deepest clip, phase 0's
// fragment counts).  Written by the calling thread's recorder (Context), the join of a sibling group (ParallelWalk::group) and
// Context::consolidate_pieces; read by prepare's stages and the debug digests.  WHEN a set may be used again is submission's business
// (Context::wait_staging): the frame only says which set is current.
class RecordedFrame {
 public:
  static constexpr int kStaging = 4;
  RecordedFrame(bool host_only, int device) : host_only_(host_only), device_(device) {}
  int next_set() const { return (set_ + 1) % kStaging; }  // the set begin() turns to (its last upload must have run by then)
  // The records of this frame go into the next set of lanes: the set's last user was the frame kStaging frames ago.  Lane 0 cleared,
  // one empty phase, lane 0's first piece open.
  Lane& begin(int w, int h);

  // ---- readers
  const std::vector<Piece>& pieces() const { return pieces_; }
  const std::vector<Phase>& phases() const { return phases_; }
  const std::vector<BlurJob>& blurs() const { return blurs_; }
  uint32_t n_records() const { return n_total_; }      // in closed pieces (the whole frame once it has ended)
  uint32_t n_extensions() const { return n_ext_total_; }
  int list_stride() const { return stride_max_; }      // max over the closed phases
  int deepest_clip() const { return deepest_clip_; }
  const int64_t* frag_mode() const { return frag_mode_; }  // phase 0: covered fragments by mode [4], elliptical, other
  int64_t frag_ellip() const { return frag_ellip_; }
  int64_t frag_other() const { return frag_other_; }
  int set() const { return set_; }
  uint64_t frame_no() const { return frame_no_; }
  const Lane& lane(int i) const { return i < 0 ? *merge_lane_[(size_t)set_] : *lanes_[(size_t)set_][(size_t)i]; }  // (-1: consolidate_pieces' lane)
  Lane& lane(int i) { return const_cast<Lane&>(static_cast<const RecordedFrame*>(this)->lane(i)); }
  uint32_t global_index(uint32_t lane0_index) const { return lane0_index + g0_delta_; }
  uint32_t global_count() const;  // records of the frame so far

  // ---- writers: pieces / phases
  uint32_t open_piece();   // lane 0's records from here on form a new piece; returns its first lane index
  void close_piece();
  void add_piece(const Piece& p);  // a pool thread's chunk, in order (the caller closed lane 0's piece before the group)
  void add_sum(const PhaseSum& s, int depth_base);
  void add_stride(int extra) { phase_extra_ += extra; }  // the current phase: bound contributed by pool threads' lanes
  void close_phase(const PhaseSum& rest);  // the phase ends here: summary, bins reached, its share of the list stride
  void split_phase(const PhaseSum& rest, int blur);  // a blurred snapshot is a barrier in painter's order
  void add_blur(const BlurJob& j) { blurs_.push_back(j); }
  void pool_slots(int slots);      // lanes 1 .. slots, ready for a sibling group
  void rewind_lane(int i, size_t recs, size_t exts);  // ... and back to where it stood before a group that failed
  Lane& merge_lane();              // consolidate_pieces: the current set's spare lane, cleared ...
  void replace_pieces(const Piece& all) { pieces_.assign(1, all); }  // ... and the frame as one piece of it
  void release_lanes() { for (auto& set : lanes_) set.clear(); }
  void release_merge_lanes() { for (auto& l : merge_lane_) l.reset(); }

 private:
  Lane& ensure_lane(int i);
  const bool host_only_;
  const int device_;
  int bins_x_ = 0, bins_y_ = 0;
  std::vector<Piece> pieces_;      // the frame in painter's order
  bool piece_open_ = false;        // the last piece is lane 0's and still growing
  uint32_t n_total_ = 0, n_ext_total_ = 0;  // records / extensions in closed pieces
  uint32_t g0_delta_ = 0;          // global index of a record of lane 0's open piece = its lane index + this
  std::vector<Phase> phases_;
  std::vector<BlurJob> blurs_;
  BBox phase_u_{0, 0, 0, 0};       // union of the current phase's record bounds
  int stride_max_ = 1;             // list stride so far: max over the closed phases
  int phase_extra_ = 0;            // the current phase: bound contributed by pool threads' lanes (sum of their own maxima)
  int deepest_clip_ = 0;
  int64_t frag_mode_[4] = {0, 0, 0, 0}, frag_ellip_ = 0, frag_other_ = 0;  // phase 0
  std::vector<std::unique_ptr<Lane>> lanes_[kStaging];
  std::unique_ptr<Lane> merge_lane_[kStaging];
  int set_ = 0;
  uint64_t frame_no_ = 0;
};

// Where everything lies in a frame's device block: records | extensions | bin records | bin boxes | chunk boxes | phase table | blur
// weight tables, byte offsets on 256-byte boundaries.  Laid out once per frame (Context::layout_frame_block) and kept with the frame.
struct FrameLayout {
  size_t recs = 0, exts = 0, binrecs = 0, boxes = 0, chunks = 0, phase_first = 0, tables = 0, total = 0;
  size_t n = 0, n_ext = 0, n_chunks = 1;  // records, extensions, chunk boxes (one per 256 records)
  std::vector<size_t> mx_h, mx_v;         // per blur node: its H / V weight table (0: none -- a filter too wide for the matrix-pipe passes)
  size_t misc() const { return chunks; }  // "from the chunk boxes on": what a staging slot's misc buffer holds (Context::build_misc)
  void lay_out(size_t n_recs, size_t n_exts, size_t n_phases, const std::vector<BlurJob>& blurs);  // fdh_prepare.cpp
  // two frames put everything at the same place (`tables` and `n_chunks` follow from the fields compared)
  bool operator==(const FrameLayout& o) const {
    return total == o.total && recs == o.recs && exts == o.exts && binrecs == o.binrecs && boxes == o.boxes && chunks == o.chunks &&
           phase_first == o.phase_first && n == o.n && n_ext == o.n_ext && mx_h == o.mx_h && mx_v == o.mx_v;
  }
};

// What the launch side needs of one frame: filled by Context::prepare on the calling thread (which also fills the run table
// the upload kernel works through), consumed by Context::issue / launch_frame on the context's submit thread, and kept
// for fdh_replay / fdh_profile.
struct LaunchJob {
  struct View { DrawRec* recs = nullptr; QuadExt* exts = nullptr; BinRec* binrecs = nullptr; int* phase_first = nullptr; uint32_t* binbox = nullptr; uint32_t* chunkbox = nullptr; };
  int W = 0, H = 0;
  int rec_y0 = 0, rec_y1 = 0;  // rows the records were culled to (the frame, or a stripe + blur reach): a replay must stay inside
  bool clear = true;
  bool latency_routes = true;  // the frame was recorded for the one-kernel blur routes (Context::pick_routes)
  uint32_t clear_rgba8 = 0xFFFFFFFFu;
  bool opaque = false;     // the surface holds alpha 255 from the frame's first launch to its last (Context::decide_opaque)
  std::vector<Phase> phases;
  std::vector<BlurJob> blurs;
  std::vector<const uint4*> mx_w_h, mx_w_v;  // per blur job: weight fragments of the matrix-pipe passes (in the frame block), or null
  std::vector<char> blur_fused;              // per blur job: both passes run as ONE out-of-place kernel (full-frame nodes)
  int n_fused = 0;
  int n_recs = 0;
  FrameLayout layout;      // of the device frame block, as this frame was prepared
  View dv;                 // typed views into it
  uint32_t* mask_spill = nullptr;  // clip levels beyond kMaskDepth, [level][strip][lane]; spill_stride dwords per level
  size_t spill_stride = 0;
  uint2* lists = nullptr;  // bin lists / counts (device)
  uint32_t* counts = nullptr;
  int bins_x = 0, bins_y = 0, list_stride = 0, binbox_shift = 0;
  int big_blur = -1;       // index of the frame's largest blur job (its passes are timed on their own)
  // the upload: the runs k_upload_frame gathers (records, bin records, extensions of every piece; phase table; blur tables)
  std::vector<UploadRun> runs;
  UploadTable table;       // (filled from `runs` when the frame is issued)
  void* d_dst = nullptr;
  int staging_slot = -1;
  // damage tracking (fdh_set_damage_tracking): the frame is tracked; it is rendered in full whatever its key (no clear, a fused full-frame
  // blur, more blur nodes than the resolve takes); the frame key (Context::damage_frame_key: everything outside the lists a bin's pixels depend on)
  bool damage = false, damage_force = false;
  uint64_t damage_key = 0;
  int n_exts = 0;
  // picking (include/figdraw_hip_pick.h): the frame was recorded with picking on; its records' tags in painter's order; its deepest clip
  // nesting (what the pick kernels' clip stacks need)
  bool pick = false;
  std::vector<PickTag> pick_tags;
  int pick_depth = 0;
};

}  // namespace fdh
