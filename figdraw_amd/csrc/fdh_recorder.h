// fdh_recorder.h -- the BackendContext state machine (glcontext.nim): transform stack, clip / rect-mask stacks, and the draw calls, each
// turning into records of ONE lane (fdh_record.cpp).  Context derives from it (lane 0: the C entry points and the serial walk); the walk
// pool's threads each own one more (fdh_frontend.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/figdraw_hip.h"
#include "fdh_plain.h"     // Error, Aff, PickTag, PhaseSum
#include "fdh_frame.h"     // Lane, BlurJob
#include "fdh_atlas.h"     // AtlasEntry, Atlas
#include "fdh_retained.h"  // RetainedRoot
#include "fdh_calllog.h"

namespace fdh {

struct RectMaskEntry { int kind; };  // 1 = fast analytic, 2 = real mask (glcontext.nim:36-44)
struct SerialOnly {};  // thrown by a pool thread's recorder at a call only the calling thread can serve (a blur node, the lazily
                       // created 4x4 "rect" atlas image): the calling thread then walks that sibling group itself
// the two bands of an upright draw's saturated core in BinRec's form (fdh_types.h; all zero: none)
struct CoreBands { uint32_t grow = 0; uint16_t hy0 = 0, hy1 = 0, vx0 = 0, vx1 = 0; };

// What a recorder may READ of the frame being recorded.  Owned by Context, which writes it on the calling thread only -- begin_frame and
// the setters (fdh_set_cull, ...) -- never while a sibling group is on the pool.
struct FrameEnv {
  int W = 0, H = 0;
  int cull_y0 = 0, cull_y1 = 0;  // rows a draw must reach to be recorded (begin_frame: the frame, or the stripe + blur reach)
  int cull_mode = 1;             // fdh_set_cull
  bool subpixel_enabled = false, subpixel_variants = false;
  bool pick_frame = false;       // fdh_set_pick, latched at begin_frame: the lanes keep tags
  int binbox_shift = 0;          // bin boxes in 64 << shift px units (frames of more than 128 bins along an axis)
  bool frame_begun = false;
  bool latency_routes = true;    // this frame takes the one-kernel blur routes (Context::pick_routes)
  const Atlas* atlas = nullptr;
};

// what a pool thread's recorder made of one chunk of a sibling group (ParallelWalk::group merges it on the calling thread)
struct ChunkResult { PhaseSum sum; BBox outer_union{0, 0, 0, 0}; int64_t fragments = 0, culled = 0; };

class Recorder {
 public:
  Recorder(const FrameEnv& env, CallLog* log) : env_(env), log_(log) {}
  virtual ~Recorder() = default;
  void save_transform();
  void restore_transform();
  void translate(float x, float y);
  void rotate(float a);
  void scale(float sx, float sy);
  void apply_transform(const float m[16]);
  bool transform_mirrors_y() const;
  void set_aa(float aa);
  float aa() const { return aa_; }
  void draw_rounded_rect_sdf(const float rect[4], const FdhColor colors[4], const float rx[4], const float ry[4], int mode,
                             float factor, float spread, const float shape[2], int fill_mode, FdhColor mid, FdhColor stop,
                             float mid_pos);
  void draw_rounded_rect_fill(const float rect[4], const FdhFill& fill, const float rx[4], const float ry[4], int mode,
                              float factor, float spread, const float shape[2]);
  void draw_image(int64_t key, const float pos[2], const FdhColor colors[4], const float size[2], bool flip_y);
  void draw_image_adj(int64_t key, const float pos[2], FdhColor color, const float size[2]);
  void draw_msdf(int64_t key, const float pos[2], FdhColor color, const float size[2], float px_range, float sd_threshold,
                 float stroke_weight, bool mtsdf, bool flip_y);
  void draw_quadratic_bezier_sdf(const float rect[4], const FdhFill& fill, const float p0[2], const float p1[2], const float p2[2],
                                 float stroke_weight, int cap);
  void draw_filled_quad(const float verts[8], const FdhColor colors[4]);
  void draw_rect(const float rect[4], FdhColor color);
  void draw_backdrop_blur(const float rect[4], const float rx[4], const float ry[4], float blur_radius);
  void begin_mask(const float rect[4], const float rx[4], const float ry[4]);
  void end_mask();
  void pop_mask();
  void begin_rect_mask(const float rect[4], const float rx[4], const float ry[4]);
  void pop_rect_mask();
  void set_subpixel_shift(float s);
  bool subpixel_enabled() const { return env_.subpixel_enabled; }
  bool subpixel_variants() const { return env_.subpixel_variants; }
  bool culling() const { return env_.cull_mode == 2 || (env_.cull_mode == 1 && !(log_ && log_->on())); }
  // would a quad over `rect` (pre-transform units), grown by `pad` pixels on every side, reach a pixel the frame will produce?
  bool rect_visible(const float rect[4], float pad) const;
  void set_tag(PickTag t) { tag_ = t; }  // the tag of the records made next (picking frames: fdh_set_pick_tag, the front-end)

  // ---- a recorder's uses.  reset: a frame begins in `lane` (transform stack, AA factor and sub-pixel shift are kept across frames).
  // adopt: a pool thread's recorder takes a chunk of a sibling group: `base`'s inherited state, nothing open of its own -- reset plus
  // what a chunk inherits, so that there is ONE list of what a recorder forgets between uses.
  void reset(Lane& lane);
  void adopt(const Recorder& base, Lane& lane, int outer_rect_masks, bool outer_open);
  ChunkResult finish_chunk() const { return ChunkResult{sum_, outer_union_, fragments_, culled_draws_}; }
  int rect_masks_around() const { return (int)rect_masks_.size() + outer_rect_masks_; }  // what adopt() is told of its base
  bool clips_open() const { return !open_ops_.empty() || outer_open_; }
  // the calling thread's recorder takes a chunk's result: the clips open around the group reach what it drew.  Returns the clip
  // nesting the chunk's own sits on.
  int absorb(const ChunkResult& c);
  // retained scenes (Context::scene_render): what a root adds, measured around its walk; a cached root's records spliced into the lane
  struct RootMark { int64_t fragments; int depth; };
  struct RootSince { int64_t fragments; PhaseSum sum; };
  RootMark mark() const { return RootMark{fragments_, depth_now_}; }
  RootSince since(const RootMark& m) const;
  void splice(const RetainedRoot& C);

 protected:
  void log_begin_frame(bool clear, const float rgba[4]);  // begin_frame / end_frame as the call log sees them
  void log_end_frame();
  PhaseSum take_sum() { const PhaseSum s = sum_; sum_ = PhaseSum{}; return s; }  // of the records committed since the last call
  void set_phase_floor(size_t lane_index) { phase_floor_ = (int)lane_index; }
  // Calling-thread-only work (Context overrides; a pool thread's recorder hands its sibling group back):
  virtual void make_rect_image() { throw SerialOnly{}; }  // the 4x4 white "rect" image, missing from the atlas
  virtual void blur_node(const DrawRec& quad, const float rect[4], float blur_radius) { throw SerialOnly{}; }  // phases are the calling thread's
  // blur_node's two halves on the lane: the open clips end with the phase / are re-established in the next one, then the mode-17 quad
  // is emitted (returns its lane index)
  std::vector<DrawRec> close_open_clips();
  uint32_t reopen_clips_and_emit(const std::vector<DrawRec>& reopen, const DrawRec& quad, const float rect[4]);
  bool clip_free() const { return open_ops_.empty(); }
  void commit_bins(uint32_t idx);  // the record's bounds are final: list-entry flags, list-stride count, phase summary

  const FrameEnv& env_;
  Lane* lane_ = nullptr;
  float aa_ = 1.2f;
  int mask_depth_ = 0;
  std::vector<RectMaskEntry> rect_masks_;
  int64_t fragments_ = 0, culled_draws_ = 0;

 private:
  DrawRec& next_rec();  // the lane's next record slot, zeroed (counted by emit_* when the draw survives culling)
  bool emit_quad(DrawRec& r, float x0, float y0, float x1, float y1, bool count_fragments);  // false: culled, nothing was recorded
  bool emit_quad_pts(DrawRec& r, const float vx[4], const float vy[4], bool count_fragments);
  struct QuadPx { float px[4], py[4]; BBox b; bool finite; };
  void quad_corners(const float vx[4], const float vy[4], QuadPx& q) const;
  bool emit_corners(DrawRec& r, const QuadPx& q, bool count_fragments);
  void push_rec(BBox b);  // count the slot next_rec() handed out
  void link_share(uint32_t idx);   // LE_SHARE on idx - 1 when record idx is drawn over the same quad with the same shape
  bool bbox_visible(const BBox& b) const;
  void culled();  // the draw call just logged left no record
  struct EntryUV { const AtlasEntry* e; float S, x, y, w, h; };  // an atlas entry, the atlas size, the entry's rect / size
  EntryUV entry_uv(int64_t key) const;
  struct PixelQuad { float x0, y0, x1, y1, w, h; };
  PixelQuad axis_lod(DrawRec& r, float S, float x0, float y0, float x1, float y1) const;
  void rect_entry();  // the 4x4 white image exists from here on (SerialOnly on a pool thread that finds it missing)
  void white_texel_uv(DrawRec& r) const;
  void shrink_to_ink(const AtlasEntry& e, bool use_alpha, int level_t);

  CallLog* const log_;              // null on a pool thread's recorder (while the log runs nothing is handed to the walk pool)
  Aff mat_;
  std::vector<Aff> mats_;
  float subpixel_shift_ = 0.0f;
  bool mask_begun_ = false;
  int outer_rect_masks_ = 0;        // pool threads: rect masks open around the sibling group (begin_rect_mask nests differently inside one)
  std::vector<uint32_t> open_ops_;  // lane indices of the open MASK_PUSH / RMASK_BEGIN records (their bounds grow with their content)
  bool outer_open_ = false;         // pool threads: clips are open around the sibling group; their bounds take ...
  BBox outer_union_{0, 0, 0, 0};    // ... the union of everything emitted here (merged by the calling thread)
  int depth_now_ = 0;               // clip nesting inside the current phase (open pushes are re-emitted at a phase's start)
  PhaseSum sum_;                    // of the records committed since the last take_sum()
  int phase_floor_ = 0;             // lane index of the first record of the current phase in this lane (LE_SHARE never crosses it)
  PickTag tag_{-1, -1};             // the tag of the records this recorder makes next
  CoreBands bands_;                 // emit_corners -> push_rec: the core bands of the record being emitted
};

}  // namespace fdh
