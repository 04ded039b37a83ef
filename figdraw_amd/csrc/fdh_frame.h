// fdh_frame.h -- the recorded frame and its launch description: a phase and its blur node, the lane one thread records into, the pieces
// that put the lanes' records into painter's order, the layout of the frame's device block, and the LaunchJob the submit side works from.
#pragma once
#include <cstdint>
#include <vector>

#include "fdh_kernels.h"
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

struct Piece {
  int lane = 0;                     // (-1: the lane Context::consolidate_pieces copies a frame of too many pieces into)
  uint32_t first = 0, n = 0;        // records [first, first + n) of the lane
  uint32_t ext_first = 0, n_ext = 0;  // their quad extensions
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
