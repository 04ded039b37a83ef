// fdh_context.h -- host side of libfigdraw_hip.so: the BackendContext-shaped state machine that turns
// backend calls into draw records (what glcontext.nim does into vertex streams) and submits them.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/figdraw_hip.h"
#include "../../include/figdraw_hip_pick.h"
#include "../../include/figdraw_hip_readback.h"
#include "../../include/figdraw_hip_stream.h"
#include "fdh_kernels.h"
#include "fdh_plain.h"        // Error, Aff, PickTag, PhaseSum
#include "fdh_memory.h"       // FDH_HIP, DeviceBuf, PinnedBuf, HostVec
#include "fdh_frame.h"        // Phase, BlurJob, Lane, Piece, RecordedFrame (one member of Context), FrameLayout, LaunchJob
#include "fdh_atlas.h"        // AtlasEntry, Atlas: one member of Context
#include "fdh_recorder.h"     // Recorder (Context is lane 0's), FrameEnv, CallLog
#include "fdh_glyphs.h"       // GlyphMaker, beside it: glyphs made on the device
#include "fdh_import.h"       // Importer, beside both: images and video frames from device memory
#include "fdh_damage_host.h"  // DamageTracker, DamageReadback: two members of Context
#include "fdh_retained.h"     // RetainedScene: one member of Context
#include "fdh_video_out.h"    // video_out::read, beside it: the frame out as NV12, P010, BGRA8

namespace fdh {

class Context : public Recorder {
 public:
  Context(int atlas_size, float pixel_scale, int device, uint32_t flags);
  ~Context();

  // BackendContext surface: the draw calls are Recorder's
  void begin_frame(int w, int h, bool clear, const float rgba[4]);
  void end_frame();
  float pixel_scale() const { return pixel_scale_; }
  void set_subpixel_enabled(bool e) { frame_env_.subpixel_enabled = e; }
  void set_subpixel_variants(bool e) { frame_env_.subpixel_variants = e; }
  void set_text_lcd_filtering(bool e) { text_lcd_filtering_ = e; }
  bool text_lcd_filtering() const { return text_lcd_filtering_; }
  void comm_info(int* rank, int* world) const { *rank = comm_ ? comm_rank_ : 0; *world = comm_ ? comm_world_ : 1; }

  // atlas (fdh_atlas.h): the context's part of a call that changes texels is sync() -- a frame in flight may still sample the atlas -- and
  // what FDH_GLYPH_LCD_CONTEXT means here; the rest is atlas_'s, for glyphs made on the device glyphs_' (fdh_glyphs.h) and for images and video
  // frames from device memory importer_'s (fdh_import.h), which place them in atlas_
  void put_image(int64_t key, int w, int h, const uint8_t* rgba, int out_rect[4]) { sync(); atlas_.put_image(stream_, key, w, h, rgba, out_rect); }
  void put_glyph_image(int64_t key, int w, int h, const uint8_t* rgba, uint32_t flags, int out_rect[4]) { sync(); glyphs_.put_glyph_image(stream_, atlas_, key, w, h, rgba, resolve_lcd(flags), out_rect); }
  void put_glyph_outline(int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]) { sync(); glyphs_.put_glyph_outline(stream_, atlas_, key, w, h, segs, n, resolve_lcd(flags), out_rect); }
  void update_image(int64_t key, int w, int h, const uint8_t* rgba) { sync(); atlas_.update_image(key, w, h, rgba); }
  void put_mips(int64_t key, int n, const int* ws, const int* hs, const uint8_t* const* premul_rgba, int out_rect[4]) { sync(); atlas_.put_mips(stream_, key, n, ws, hs, premul_rgba, out_rect); }
  void put_flippy(int64_t key, const uint8_t* data, size_t n, int out_rect[4]) { sync(); atlas_.put_flippy(stream_, key, data, n, out_rect); }
  void remove_image(int64_t key) { atlas_.remove(key); }
  void put_glyph_outline_cubic(int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]) { sync(); glyphs_.put_glyph_outline_cubic(stream_, atlas_, key, w, h, segs, n, resolve_lcd(flags), out_rect); }
  void put_glyph_outlines(const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) { sync(); glyphs_.put_glyph_outlines(stream_, atlas_, glyphs, n, flags, out_rects); }
  void put_glyph_outlines_cubic(const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) { sync(); glyphs_.put_glyph_outlines_cubic(stream_, atlas_, glyphs, n, flags, out_rects); }
  const FdhGlyphBatchStats& glyph_batch_stats() const { return glyphs_.glyph_batch_stats(); }
  void put_glyph_coverage_batch(const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) { sync(); glyphs_.put_glyph_coverage_batch(stream_, atlas_, glyphs, n, resolve_lcd(flags), out_rects); }
  void put_glyph_coverage_batch_cubic(const FdhGlyphOutline* glyphs, int n, uint32_t flags, int (*out_rects)[4]) { sync(); glyphs_.put_glyph_coverage_batch_cubic(stream_, atlas_, glyphs, n, resolve_lcd(flags), out_rects); }
  const FdhGlyphBatchStats& glyph_coverage_batch_stats() const { return glyphs_.glyph_coverage_batch_stats(); }
  void put_image_sdf(int64_t key, int w, int h, const uint8_t* rgba, int channel, int pad, uint32_t flags, int out_rect[4]) { sync(); glyphs_.put_image_sdf(stream_, atlas_, key, w, h, rgba, channel, pad, flags, out_rect); }
  void put_image_sdf_of(int64_t src_key, int64_t key, int channel, int pad, uint32_t flags, int out_rect[4]) { sync(); glyphs_.put_image_sdf_of(stream_, atlas_, src_key, key, channel, pad, flags, out_rect); }
  void put_image_device(int64_t key, const FdhDeviceImage* img, int out_rect[4]) { sync(); importer_.put_device_image(stream_, atlas_, device_, key, img, out_rect); }
  void update_image_device(int64_t key, const FdhDeviceImage* img) { sync(); importer_.update_device_image(stream_, atlas_, device_, key, img); }
  void put_images_device(const int64_t* keys, const FdhDeviceImage* images, int n, int (*out_rects)[4]) { sync(); importer_.put_device_images(stream_, atlas_, device_, keys, images, n, out_rects); }
  void update_images_device(const int64_t* keys, const FdhDeviceImage* images, int n) { sync(); importer_.update_device_images(stream_, atlas_, device_, keys, images, n); }
  const FdhImageBatchStats& image_batch_stats() const { return importer_.image_batch_stats(); }
  void put_video_frame(int64_t key, const FdhVideoFrame* frame, int out_rect[4]) { sync(); importer_.put_video_frame(stream_, atlas_, device_, key, frame, out_rect); }
  void update_video_frame(int64_t key, const FdhVideoFrame* frame) { sync(); importer_.update_video_frame(stream_, atlas_, device_, key, frame); }
  void put_video_frames(const int64_t* keys, const FdhVideoFrame* frames, int n, int (*out_rects)[4]) { sync(); importer_.put_video_frames(stream_, atlas_, device_, keys, frames, n, out_rects); }
  void update_video_frames(const int64_t* keys, const FdhVideoFrame* frames, int n) { sync(); importer_.update_video_frames(stream_, atlas_, device_, keys, frames, n); }
  const FdhVideoBatchStats& video_batch_stats() const { return importer_.video_batch_stats(); }
  void put_video_planes(int64_t key, const FdhVideoPlanes* frame, int out_rect[4]) { sync(); importer_.put_video_planes(stream_, atlas_, device_, key, frame, out_rect); }
  void update_video_planes(int64_t key, const FdhVideoPlanes* frame) { sync(); importer_.update_video_planes(stream_, atlas_, device_, key, frame); }
  void put_video_422(int64_t key, const FdhVideoPlanes* frame, int out_rect[4]) { sync(); importer_.put_video_422(stream_, atlas_, device_, key, frame, out_rect); }
  void update_video_422(int64_t key, const FdhVideoPlanes* frame) { sync(); importer_.update_video_422(stream_, atlas_, device_, key, frame); }
  void put_video_alpha(int64_t key, const FdhVideoAlphaPlanes* frame, int out_rect[4]) { sync(); importer_.put_video_alpha(stream_, atlas_, device_, key, frame, out_rect); }
  void update_video_alpha(int64_t key, const FdhVideoAlphaPlanes* frame) { sync(); importer_.update_video_alpha(stream_, atlas_, device_, key, frame); }
  bool has_image(int64_t key) const { return atlas_.has(key); }
  void reset_atlas(int minimum_size) { sync(); atlas_.reset(minimum_size, stream_); }
  int atlas_size() const { return atlas_.size(); }
  int64_t atlas_packed_area() const { return atlas_.packed_area(); }
  // compaction and keep mode (include_glyphs/figdraw_hip_atlas.h): the atlas's; glyphs_ moves the texels for it (AtlasMover)
  void compact_atlas(int size, FdhAtlasMoveStats* out) { sync(); atlas_.compact(stream_, size, out); }
  void set_atlas_keep(bool on) { atlas_.set_keep(on); }
  bool atlas_keep() const { return atlas_.keep(); }
  void image_rect(int64_t key, int out_rect[4]) const;
  void atlas_usage(FdhAtlasUsage* out) const { atlas_.usage(out); }
  void debug_read_atlas_level(int level, uint8_t* out, int64_t capacity_bytes);  // (fdh_debug.cpp)

  // readback / interop
  void read_pixels(int x, int y, int w, int h, uint8_t* out);
  void read_video_frame(const FdhVideoTarget* target);  // (include_video/figdraw_hip_video_out.h; fdh_video_out.h)
  void read_video_planes(const FdhVideoPlanesTarget* target);  // (include_video/figdraw_hip_video_planar.h; fdh_video_out.h)
  void read_video_422(const FdhVideoPlanesTarget* target);     // (include_video/figdraw_hip_video_422.h; fdh_video_out.h)
  void read_video_alpha(const FdhVideoAlphaPlanesTarget* target);  // (include_video/figdraw_hip_video_alpha.h; fdh_video_out.h)
  void frame_device_ptr(void** p, int* w, int* h, int64_t* pitch_bytes);
  void debug_read_surface(int which, uint8_t* out);
  // call recorder (fdh_record_begin / fdh_record_json): the backend-level calls the scene front-end makes, as JSON
  void record_begin() { call_log_.begin(); }
  const char* record_json() { return call_log_.json(); }
  void sync();
  void set_stream(void* s);

  // scene front-end (fdh_frontend.cpp)
  void set_ui_scale(float s) { ui_scale_ = s; }
  float ui_scale() const { return ui_scale_; }
  void render_frame(const FdhScene* scene, float fw, float fh, bool clear, const float rgba[4]);
  // retained scenes: the tree and its edits are retained_'s (fdh_retained.h); a frame of it is recorded here (fdh_frontend.cpp)
  void scene_retain(const FdhScene* scene, float fw, float fh, bool clear, const float rgba[4]) { retained_.retain(scene, fw, fh, clear, rgba); scene_render(); }
  void scene_update_nodes(int layer, int first, int count, const FdhFig* nodes, const FdhScene* side) { retained_.update_nodes(layer, first, count, nodes, side); }
  void scene_replace_root(int layer, int slot, const FdhFig* subtree, int n, const FdhScene* side, bool insert) { retained_.replace_root(layer, slot, subtree, n, side, insert); }
  void scene_render();
  void scene_stats(int64_t* walked, int64_t* reused) const { retained_.stats(walked, reused); }
  int64_t uploaded_bytes() { drain(); return uploaded_bytes_; }
  // fault hunting (fdh_debug.cpp)
  void debug_verify_upload(uint32_t out[24]);  // fdh_debug_verify_upload
  void debug_bin_digest(uint64_t out[8]);      // fdh_debug_bin_digest
  uint64_t record_digest();  // FNV-1a over the last frame's draw records (diagnostic: works on record-only contexts)

  // multi-GPU: the gather over RCCL (fdh_comm.cpp)
  void comm_init(const uint8_t id[FDH_COMM_ID_BYTES], int rank, int world);
  void comm_share(Context* owner);
  void comm_destroy();
  void gather_stripes(int dst_rank, void* dst_image);
  void gather_frames(int dst_rank, void* const* dst_images);
  int comm_world() const { return comm_ ? comm_world_ : 1; }

  // multi-GPU / measurement
  void set_stripe(int y0, int y1) {
    drain();
    if (damage_.on && y1 > y0) throw Error(FDH_ERR_INVALID, "fdh_set_stripe: damage tracking is on (fdh_set_damage_tracking: not under row stripes)");
    if (readback_.on && y1 > y0) throw Error(FDH_ERR_INVALID, "fdh_set_stripe: damage readback is on (fdh_set_damage_readback: not under row stripes)");
    stripe_y0_ = y0; stripe_y1_ = y1;
  }
  // damage tracking, damage readback and coded damage readback: the context's part of each entry point; the rest is fdh_damage.cpp's
  void set_damage_tracking(bool on);
  void damage_bins(uint8_t* mask, int cap, int* bins_x, int* bins_y, int* n_damaged, bool changed_only);
  void set_damage_readback(bool on);
  void read_damage(const FdhDamageTile** tiles, const uint8_t** pixels, int* n_tiles, int* frame_w, int* frame_h, int* full);
  void read_damage_into(uint8_t* image, int64_t pitch_bytes, int w, int h, int* n_tiles);
  void read_damage_coded(const FdhCodedTile** tiles, const uint8_t** payload, int* n_tiles, int64_t* payload_bytes, int* frame_w, int* frame_h, int* full);
  void set_damage_exact(bool on);
  void damage_exact_stats(int* n_pending, int* n_changed, int* fresh);
  void read_damage_moved(const FdhDamageMove* moves, int n_moves, const FdhCodedTile** tiles, const uint8_t** payload, int* n_tiles, int64_t* payload_bytes,
                         int* frame_w, int* frame_h, int* full, int* n_copied);
  void find_damage_moves(int max_shift, FdhDamageMove* out_moves, int* out_votes, int cap, int* n_out);
  // picking (include/figdraw_hip_pick.h; fdh_pick.cpp)
  void set_pick(bool on) { pick_on_ = on; }
  void set_pick_tag(int32_t z, int32_t id) { set_tag(PickTag{z, id}); }
  void pick_points(const float* xy, int n, int threshold, uint32_t flags, int max_hits, FdhPickHit* out, int* counts);
  void pick_region(int x, int y, int w, int h, int threshold, uint32_t flags, int32_t* out_draw);
  void pick_draw_tags(int32_t* zlevels, int32_t* ids, int cap, int* n);
  // Culling (fdh_set_cull): draws whose pixel bounds miss the frame -- or, under fdh_set_stripe, the stripe's rows widened by the
  // reach of the scene's blur nodes -- are not recorded, and the scene front-end skips the content of a clipping node whose mask
  // lies outside.  0 off, 1 on (default; off while the call recorder runs, so that recorded streams stay the reference's), 2 on
  // even while recording (tests).  The pixels are the same either way.
  void set_cull(int mode) { frame_env_.cull_mode = mode < 0 ? 0 : (mode > 2 ? 2 : mode); }
  int64_t culled_draws() const { return culled_total_; }
  // The scene front-end decomposes large sibling groups on `n` pool threads beside the calling one (0: serial; default:
  // FDH_WALK_THREADS or a few, by the host's core count).  Same records either way (fdh_debug_record_digest).
  void set_walk_threads(int n) { walk_threads_ = n < 0 ? -1 : (n > 64 ? 64 : n); }
  int walk_threads() const;
  int64_t parallel_groups() const { return parallel_groups_; }
  // What a sibling group on the pool needs of the context (ParallelWalk::group, fdh_frontend.cpp).
  // GroupCuts: where the last frames cut their forked sibling groups into chunks, and what each chunk cost (records made + a share per
  // item visited): a group that comes again -- same first item, same length -- is cut where that cost says the work is, not into equal
  // item counts (a viewport's visible rows are a fifth of its cells).  Boundaries change nothing a frame records.
  struct GroupCuts { int first_item = -1, n = 0; std::vector<int> cut; std::vector<float> cost; uint64_t used = 0; };
  std::vector<GroupCuts>& group_cuts() { return group_cuts_; }
  void count_parallel_group() { parallel_groups_++; }
  bool may_fork() const { return env_.frame_begun && !call_log_.on(); }  // (not while the call recorder runs)
  RecordedFrame& frame() { return frame_; }
  void reopen_piece() { set_phase_floor(frame_.open_piece()); }  // lane 0 goes on after a group (LE_SHARE never looks across a piece boundary)
  Recorder& pool_recorder(int slot);  // the pool threads' recorders (slot s records into lane s + 1)
  void use_device_here() const;       // a pool thread before it publishes: a lane's pinned mirror is allocated by the thread that publishes into it
  void set_blur_route(int route) { blur_route_ = route < 0 ? -1 : (route ? 1 : 0); }
  void replay(int times);
  void replay_timed(int times, float* ms_out);
  void replay_async(int times);
  void profile(int times);
  int block_wave_bins() { drain(); return block_wave_bins_; }
  void frame_stats(FdhFrameStats* out) { drain(); *out = stats_; out->ms_host_launch = launch_ms_.load(std::memory_order_relaxed); }
  // Submission is asynchronous: end_frame hands the recorded frame to the context's submit thread (the upload, the kernel
  // launches) and returns.  flush() returns once everything submitted so far has been ENQUEUED on the
  // stream (a consumer that orders its own work after the frame on the same stream calls it first); sync() also waits for the GPU.
  void flush() { drain(); }

 private:
  void release_device_state();  // the destructor's device half (also a constructor that fails half way)
  // Recorder's calling-thread-only work (fdh_context.cpp)
  void make_rect_image() override;
  void blur_node(const DrawRec& quad, const float rect[4], float blur_radius) override;
  // FDH_GLYPH_LCD_CONTEXT: the LCD filter as setTextLcdFilteringEnabled said.  (With FDH_GLYPH_MTSDF the flags pass as they are: a distance
  // field takes neither LCD flag, and the atlas refuses them.)
  uint32_t resolve_lcd(uint32_t flags) const {
    if (!(flags & FDH_GLYPH_LCD_CONTEXT) || (flags & FDH_GLYPH_MTSDF)) return flags;
    return (flags & ~(uint32_t)(FDH_GLYPH_LCD_FILTER | FDH_GLYPH_LCD_CONTEXT)) | (text_lcd_filtering_ ? FDH_GLYPH_LCD_FILTER : 0u);
  }
  // fold_clear's guard: puts a folded draw's bounds back into its lane when prepare is left, by return or by exception
  struct FoldGuard {
    BinRec* br = nullptr;
    BBox box{0, 0, 0, 0};
    FoldGuard() = default;
    FoldGuard(FoldGuard&& o) noexcept : br(o.br), box(o.box) { o.br = nullptr; }
    FoldGuard(const FoldGuard&) = delete;
    FoldGuard& operator=(const FoldGuard&) = delete;
    ~FoldGuard() { if (br) br->box = box; }
  };

  // calling thread: recorded frame -> run table + launch description (fdh_prepare.cpp)
  void prepare(LaunchJob& J);
  // prepare's stages, in the order it takes them.  The order is part of their contract:
  //  - consolidate_pieces (a frame of more pieces than the run table holds) runs BEFORE fold_clear: the copy would carry the emptied box,
  //    and the guard restores the original lane only -- fdh_debug_record_digest would find an empty box for record 0 of such a frame;
  //  - fold_clear runs before damage_frame_key and decide_opaque: both read the folded clear colour;
  //  - patch_runs / gather_runs read a lane's device views after the lane was published (the mirrors are then where they will stay);
  //  - fence_staging comes last: everything this thread and the pool's threads stored into device memory is behind it.
  void describe_frame(LaunchJob& J);
  void size_bin_buffers(LaunchJob& J);       // bin lists, counts, the clip spill plane
  void layout_frame_block(LaunchJob& J);     // J.layout; the block itself; views, table pointers and upload offsets from it
  void choose_fused_blurs(LaunchJob& J);
  void consolidate_pieces();                 // (only a frame of more pieces than the upload's run table holds)
  FoldGuard fold_clear(LaunchJob& J);
  void decide_opaque(LaunchJob& J) const;    // J.opaque, from the FOLDED clear colour
  void damage_frame_key(LaunchJob& J) const;
  bool shadow_usable(const LaunchJob& J);
  bool tables_resident(const LaunchJob& J, bool shadow_ok);
  void build_misc(const LaunchJob& J, bool tables_resident);
  bool patch_runs(LaunchJob& J, bool shadow_ok);          // retained scenes: upload what differs from the shadow; false: not this frame
  void gather_runs(LaunchJob& J, bool tables_resident);   // every piece whole (+ the shadow's refresh)
  void account_frame(LaunchJob& J);
  void fence_staging();
  void issue(LaunchJob& J);    // submit thread: upload + kernel launches
  void launch_frame(const LaunchJob& J, bool profile, uint32_t upload_seq = 0);  // upload_seq: the bin launch reports it to the host
  // launch_frame's stages, in the order it takes them
  struct Schedule { const int* order_now = nullptr; int* order_next = nullptr; int deep_min = 0, deep_k8 = 0, block_max = 0, block_k8 = -1; };  // of the full-frame launch
  void phase_rows(const LaunchJob& J, std::vector<int>& lo, std::vector<int>& hi) const;
  BinParams bin_params(const LaunchJob& J, uint32_t upload_seq) const;
  Schedule schedule(const LaunchJob& J, bool direct, bool partial);
  uint32_t* launch_blur(const LaunchJob& J, int p, uint32_t* cur, int row_lo, int row_hi, bool partial);
  CompositeParams composite_params(const LaunchJob& J, int p, uint32_t* cur, int row_lo, int row_hi, bool direct, const Schedule& S) const;
  template <typename Buf> void reserve_quiet(Buf& buf, size_t n);  // (defined below the class)
  void drain();        // wait until the submit thread is idle; rethrows what its last job threw
  void worker_main();
  hipEvent_t next_event();
  void ensure_surfaces();
  void need_device(const char* what) const;
  // render_frame's and scene_render's frame around walk(links): the frame of fw x fh UI units begun (culled, under a row stripe, by the
  // blur reach of `scene`), the pixel scale on the transform stack, the frame ended -- or, when the walk throws, left unbegun
  template <typename Walk> void walk_frame(float fw, float fh, bool clear, const float rgba[4], const FdhScene& scene, Walk walk);  // (fdh_frontend.cpp)
  void pick_routes();                       // begin_frame: the one-kernel blur routes (a frame alone) or the two-pass ones (frames in flight)

  int device_ = 0;
  uint32_t flags_ = 0;
  int blur_route_ = -1;   // fdh_set_blur_route: -1 per-frame decision, 0 two passes, 1 fused
  std::shared_ptr<void> comm_;  // shared communicator object (fdh_comm.cpp), shared with the contexts that borrowed it: destroyed with its last holder
  int comm_rank_ = 0, comm_world_ = 1;
  hipStream_t own_stream_ = nullptr, stream_ = nullptr;
  volatile unsigned int* hdp_flush_reg_ = nullptr;  // the device's HDP_MEM_COHERENCY_FLUSH_CNTL register, mapped by the runtime (or null)
  hipEvent_t ev_[2] = {};
  std::vector<hipEvent_t> ev_pool_;
  size_t ev_used_ = 0;
  // profile mode (fdh_profile): a launch's own start / end events, summed per kind -- the bin launch (and damage tracking's), phase 0's
  // composite, the later phases', a blur node's H / V pass (the frame's largest node: kinds of their own), a node's fused H + V kernel
  enum SpanKind { kSpanBin, kSpanCompositeMain, kSpanCompositeLater, kSpanBlurH, kSpanBlurV, kSpanBigBlurH, kSpanBigBlurV, kSpanBlurFused, kSpanKinds };
  struct Span { SpanKind kind; hipEvent_t a, b; };
  std::vector<Span> spans_;
  bool profiling_ = false;  // the frame being launched is fdh_profile's
  void span_begin(SpanKind kind); void span_end();

  // frame state
  FrameEnv frame_env_;  // what the recorders read of the frame (Recorder::env_ is this, const): size, cull rows, settings latched at begin_frame
  bool clear_ = true;
  uint32_t clear_rgba8_ = 0xFFFFFFFFu;
  float pixel_scale_ = 1.0f, ui_scale_ = 1.0f;
  float ctx_aa_ = 1.2f;   // (Recorder::aa_ of lane 0 is the live value; kept across frames)
  bool text_lcd_filtering_ = false;
  int stripe_y0_ = 0, stripe_y1_ = 0;
  int pending_reach_ = -1;         // render_frame / scene_render: summed vertical reach of the scene's blur nodes (-1: unknown)
  int64_t culled_total_ = 0;       // of the last recorded frame
  int walk_threads_ = -1;
  int64_t parallel_groups_ = 0;    // sibling groups of the last frame that were decomposed on the pool
  std::vector<GroupCuts> group_cuts_;

  // submit thread (device contexts, unless FDH_CREATE_SYNC_SUBMIT): one job in flight at most.  The flag both sides poll
  // sits on a cache line of its own, and so do the submission side's state and the recording side's: an idle submit thread
  // polling `pending_` next to the vector headers the caller bumps with every draw call tripled the cost of recording.
  std::thread worker_;
  alignas(128) std::atomic<bool> pending_{false};
  alignas(128) std::mutex mu_;
  std::condition_variable cv_job_, cv_done_;
  bool quit_ = false;
  std::exception_ptr worker_error_;
  alignas(128) LaunchJob job_;  // the frame being (or last) issued; what fdh_replay / fdh_profile launch again
  std::atomic<float> launch_ms_{0.0f};
  alignas(128) LaunchJob next_; // the frame being prepared (calling thread)
  const void* tables_dev_ = nullptr;  // the device block whose tail holds the blur weight tables described by ...
  FrameLayout tables_layout_;
  std::vector<float> tables_sig_, tables_sig_next_;  // the filters behind those tables; ... behind the frame being prepared

  // recorded frame (calling thread)
  alignas(128) bool rec_diff_upload_ = false;
  RecordedFrame frame_;            // (fdh_frame.h)
  bool have_frame_ = false;

  // device state (submission side)
  alignas(128) uint32_t* fb_ = nullptr;
  uint32_t *backdrop_ = nullptr, *blur_tmp_ = nullptr;
  uint32_t* alt_ = nullptr;  // second frame surface: a fused full-frame blur renders out of place, phases alternate between fb_ and this
  uint32_t* dbg_snap_ = nullptr;
  RetainedScene retained_;  // (fdh_retained.h)
  bool host_only_ = false;  // FDH_CREATE_RECORD_ONLY
  CallLog call_log_;        // fdh_record_begin / fdh_record_json (fdh_calllog.h)
  int surf_w_ = 0, surf_h_ = 0;
  // records, quad extensions, bin records and phase offsets of a frame live in ONE device block; the typed views point into it
  DeviceBuf<uint8_t> d_frame_;
  DeviceBuf<uint32_t> d_mask_spill_;  // clip-stack levels beyond kMaskDepth (Context::size_bin_buffers sizes it)
  DeviceBuf<uint2> d_lists_;
  DeviceBuf<uint32_t> d_counts_;
  DeviceBuf<int> d_order_[2];  // phase 0's bins, longest list first: read by this frame's launch / written for the next
  DamageTracker damage_;
  DamageReadback readback_;
  ReadFrame read_frame(const char* who);  // a read's first steps: the last frame is complete; what the read needs of it
  // the context's part of fdh_read_video_frame, _planes, _422 and _alpha: the last frame is complete, where it lies and what no plane may touch
  template <class Target>
  void read_video(const char* who, void (*read)(hipStream_t, int, const uint32_t*, int, int, const Target*, const video_out::Own*, int), const Target* target);
  // picking: fdh_set_pick (calling thread), latched per frame at begin_frame (FrameEnv::pick_frame: the lanes keep tags); the pick launches' buffers
  bool pick_on_ = false;
  void pick_check(const char* who, int threshold, uint32_t flags);
  DeviceBuf<uint8_t> d_pick_, d_pick_spill_;
  PinnedBuf<uint8_t> h_pick_;
  int order_read_ = 0, order_nb_ = 0;
  bool order_valid_ = false;
  // the frame's kStaging sets of lanes in rotation (RecordedFrame), each released when the upload that reads it has run (the bin launch behind it says so
  // through *seq_host_, Context::issue; an event where a frame has no bin launch): the host records
  // frames N + 1 .. while frame N's upload has not run yet (one set forced a stream sync per frame)
  struct MxTables { int reach; std::vector<float> dense; std::vector<uint8_t> h, v; bool keeps_opaque = false; };  // k_blur_mx weight fragments of one filter
  std::vector<MxTables> mx_cache_;
  static constexpr int kStaging = RecordedFrame::kStaging;
  std::vector<std::unique_ptr<Recorder>> pool_recs_;  // the pool threads' recorders (slot s records into lane s + 1)
  HostVec<uint8_t> misc_[kStaging];   // per slot (pinned): phase table, blur weight tables
  std::vector<uint8_t> misc_host_;    // ... as build_misc builds them
  const uint8_t* misc_dev_[kStaging] = {};   // the pinned buffers' device views (hipHostGetDevicePointer costs a third of a microsecond)
  const uint8_t* misc_dev_host_[kStaging] = {};
  // retained scenes: host copy of what the device's frame block holds (patch_runs: upload only what differs; gather_runs refreshes it)
  std::vector<uint8_t> shadow_;
  FrameLayout shadow_layout_;         // the offsets that block was laid out with
  const void* shadow_dev_ = nullptr;  // ... and where it lives
  int64_t uploaded_bytes_ = 0;        // by the last submit
  hipEvent_t staging_ev_[kStaging] = {};
  char staging_busy_[kStaging] = {};     // 0: free; 1: until staging_ev_ fires; 2: until *seq_host_ reaches staging_seq_ (Context::issue)
  uint32_t staging_seq_[kStaging] = {};
  // pinned, 16 words, written by the compositor's sorting waves: bins per class with lists of at least deep_min draws, then (words 8..15) of
  // more than block_max draws
  volatile uint32_t* deep_host_ = nullptr;
  int block_wave_bins_ = -1;  // bins of the last full-frame launch whose blocks had one wave each (-1: the launch did not take the form)
  volatile uint32_t* seq_host_ = nullptr;  // pinned: the sequence number of the last frame whose bin launch has started (k_bin_draws)
  uint32_t upload_seq_ = 0;
  void wait_staging(int slot);             // calling thread: until the set's last upload has run

  Atlas atlas_;  // (fdh_atlas.h)
  GlyphMaker glyphs_;  // (fdh_glyphs.h)
  Importer importer_;  // (fdh_import.h)

  FdhFrameStats stats_ = {};
 public:
  // where the calling thread's time went in the last frame, ns (fdh_debug_host_times): 0 begin_frame, 1 of it: waiting for the
  // lane set's previous upload, 2 walk / calls (begin_frame's end .. end_frame), 3 end_frame before prepare, 4 prepare, 5 of it:
  // publishing, 6 waiting for the submit thread, 7 sibling groups on the pool (of 2), 8 of it: the pool's run, 9 of it: merging
  int64_t host_ns_[12] = {};
  struct HostTimer {
    int64_t& acc; std::chrono::steady_clock::time_point t0;
    explicit HostTimer(int64_t& a) : acc(a), t0(std::chrono::steady_clock::now()) {}
    ~HostTimer() { acc += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
  };
 private:
  std::chrono::steady_clock::time_point t_begin_frame_, t_walk_begin_;
  float host_record_ms_ = 0.0f;
};

// a device buffer the frame in submission may still use: wait for it before the block moves
template <typename Buf> void Context::reserve_quiet(Buf& buf, size_t n) {
  if (n <= buf.cap) return;
  drain();
  FDH_HIP(hipStreamSynchronize(stream_));
  buf.reserve(n);
}

void record_host_form(DrawRec& r);  // undo the device form of a committed record's colours (fdh_record.cpp)
void stripe_rows(int height, int world, int rank, int* y0, int* y1);
void comm_unique_id(uint8_t out[FDH_COMM_ID_BYTES]);
void blur_weight_fragments(float blur_radius, bool vertical, float* dense, uint16_t* frag_bits, int* reach, int* k_steps);
void saturated_core_of(const float rect[4], const float rx[4], const float ry[4], int mode, float factor, float spread,
                       const float shape[2], float aa, int out[4]);
int saturated_core_union_of(const float rect[4], const float rx[4], const float ry[4], int mode, float factor, float spread,
                            const float shape[2], float aa, int push, int out[12]);
int binrec_core_rects(const BinRec& br, int out[12]);

}  // namespace fdh
