// fdh_context.cpp -- a context's life and a frame's way through it: creation and teardown, the submit thread, begin_frame /
// end_frame, and the launches of a prepared frame (issue, launch_frame and its stages, replay / profile), readback, and the context's
// part of the damage entry points (the rest of those is fdh_damage.cpp's).  The draw calls between begin_frame and end_frame are fdh_record.cpp's; what end_frame does on the calling thread
// before the hand-over is fdh_prepare.cpp's.
#include "fdh_context.h"
#include "fdh_host.h"
#include "fdh_walkpool.h"

#include <chrono>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace fdh {

void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw Error(FDH_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

void poison_fresh(void* p, size_t bytes) {
#if defined(FDH_POISON)  // fault-hunting builds only (make variant DEFS=-DFDH_POISON=0xA5)
  if (!p || !bytes) return;
  (void)hipMemset(p, FDH_POISON, bytes);
  (void)hipDeviceSynchronize();
#else
  (void)p; (void)bytes;
#endif
}

// ------------------------------------------------------------------ lifetime
Context::Context(int atlas_size, float pixel_scale, int device, uint32_t flags)
    : Recorder(frame_env_, &call_log_), device_(device), flags_(flags), pixel_scale_(pixel_scale),
      frame_((flags & FDH_CREATE_RECORD_ONLY) != 0, device), host_only_((flags & FDH_CREATE_RECORD_ONLY) != 0) {
  frame_env_.atlas = &atlas_;
  atlas_.set_mover(&glyphs_);
  if (host_only_) {  // a call recorder: the front-end and the atlas packer run, nothing is drawn, no device is touched
    atlas_.init(atlas_size, false, nullptr);
    return;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw Error(FDH_ERR_NO_DEVICE, "no HIP device visible (libfigdraw_hip has no CPU fallback)");
  if (device < 0 || device >= n) throw Error(FDH_ERR_NO_DEVICE, "HIP device ordinal out of range");
  FDH_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  FDH_HIP(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    throw Error(FDH_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
  // host writes into device memory through the BAR pass the GPU's host data path, which may hold them: its flush register (mapped
  // for exactly this: HSA_AMD_AGENT_INFO_HDP_FLUSH) is written before the launches that read the staging mirrors (Context::fence_staging)
  hdp_flush_reg_ = prop.hdpMemFlushCntl;
  // counted in BEFORE the first piece of device state: from here on no trim of the staging store can run (vram_context_gone); a
  // constructor that fails below counts itself out again (release_device_state: the destructor of a half-built object never runs)
  vram_context_born(device_);
  try {
    FDH_HIP(hipStreamCreateWithFlags(&own_stream_, hipStreamNonBlocking));
    stream_ = own_stream_;
    for (auto& e : ev_) FDH_HIP(hipEventCreate(&e));
    for (auto& e : staging_ev_) FDH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    atlas_.init(atlas_size, true, stream_);
    static const bool env_sync = [] { const char* e = std::getenv("FDH_SYNC_SUBMIT"); return e && std::atoi(e) != 0; }();
    if (!(flags & FDH_CREATE_SYNC_SUBMIT) && !env_sync) worker_ = std::thread([this] { worker_main(); });
  } catch (...) {
    release_device_state();  // (the stream, the events, the atlas levels allocated so far)
    throw;
  }
}

Context::~Context() {
  if (host_only_) return;
  try { comm_destroy(); } catch (...) {}
  if (worker_.joinable()) {
    { std::lock_guard<std::mutex> lk(mu_); quit_ = true; }
    cv_job_.notify_all();
    worker_.join();
  }
  release_device_state();
}

// everything the context holds on its device, then its count in the staging store (every pointer is null or live: safe half-built)
void Context::release_device_state() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
  for (auto& e : ev_pool_) (void)hipEventDestroy(e);
  atlas_.release();
  glyphs_.release();
  importer_.release();
  if (fb_) (void)hipFree(fb_);
  if (backdrop_) (void)hipFree(backdrop_);
  if (blur_tmp_) (void)hipFree(blur_tmp_);
  if (alt_) (void)hipFree(alt_);
  if (dbg_snap_) (void)hipFree(dbg_snap_);
  d_frame_.release(); d_lists_.release(); d_counts_.release(); d_order_[0].release(); d_order_[1].release();
  damage_.release(); readback_.release();
  d_mask_spill_.release();
  d_pick_.release(); d_pick_spill_.release(); h_pick_.release();
  frame_.release_lanes();  // (pinned arrays: freed while the device is still this thread's)
  for (auto& m : misc_) m.release();
  for (auto& e : staging_ev_) if (e) (void)hipEventDestroy(e);
  if (seq_host_) (void)hipHostFree((void*)seq_host_);
  if (deep_host_) (void)hipHostFree((void*)deep_host_);
  if (own_stream_) (void)hipStreamDestroy(own_stream_);
  frame_.release_merge_lanes();  // (their staging blocks go to the store before the store is looked at)
  vram_context_gone(device_);
}

void Context::set_stream(void* s) {
  need_device("set_stream");
  drain();
  FDH_HIP(hipStreamSynchronize(stream_));
  stream_ = s ? (hipStream_t)s : own_stream_;
}
void Context::need_device(const char* what) const {
  if (host_only_) throw Error(FDH_ERR_NO_DEVICE, std::string(what) + ": this context was created with FDH_CREATE_RECORD_ONLY (it records calls, it draws nothing)");
}
// ------------------------------------------------------------------ the submit thread
// end_frame prepares the frame on the calling thread, hands the LaunchJob over and returns; this thread issues the launches
// (Context::issue: ~20 us of HIP runtime calls per bench frame that used to sit between the caller's tree walks).  One job at
// a time; the caller only waits when it has the NEXT frame prepared before this one's launches are out.
// Both sides spin briefly before they sleep: at 10 000 frames/s a futex round trip per hand-over would be a tenth of a frame.
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
}
void Context::worker_main() {
  (void)hipSetDevice(device_);
  for (;;) {
    bool have = false;
    for (int spin = 0; spin < 4000 && !have; spin++) { have = pending_.load(std::memory_order_acquire); if (!have) cpu_relax(); }
    if (!have) {
      std::unique_lock<std::mutex> lk(mu_);
      cv_job_.wait(lk, [&] { return pending_.load(std::memory_order_acquire) || quit_; });
      if (!pending_.load(std::memory_order_acquire)) return;  // quit_
    }
    try {
      issue(job_);
    } catch (...) {
      worker_error_ = std::current_exception();
    }
    {
      std::lock_guard<std::mutex> lk(mu_);
      pending_.store(false, std::memory_order_release);
    }
    cv_done_.notify_all();
  }
}
void Context::drain() {
  if (!worker_.joinable()) return;
  for (int spin = 0; spin < 4000 && pending_.load(std::memory_order_acquire); spin++) cpu_relax();
  if (pending_.load(std::memory_order_acquire)) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] { return !pending_.load(std::memory_order_acquire); });
  }
  if (worker_error_) {
    std::exception_ptr e = worker_error_;
    worker_error_ = nullptr;
    // what that frame was to upload may not have arrived: nothing is taken for resident in the device block any more
    tables_dev_ = nullptr; shadow_dev_ = nullptr; have_frame_ = false;
    std::rethrow_exception(e);
  }
}

void Context::wait_staging(int slot) {
  if (staging_busy_[slot] == 2) {
    // the word is pinned host memory the device writes: a load of it is an uncached read (~100 ns); spin, then yield, and after
    // a few milliseconds stop trusting it and wait for the stream (the frame is then done for certain)
    const uint32_t want = staging_seq_[slot];
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; (int32_t)(*seq_host_ - want) < 0; spins++) {
      if (spins < 2000) { cpu_relax(); continue; }
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) { FDH_HIP(hipStreamSynchronize(stream_)); break; }
      std::this_thread::yield();
    }
  } else if (staging_busy_[slot] == 1) {
    FDH_HIP(hipEventSynchronize(staging_ev_[slot]));
  }
  staging_busy_[slot] = 0;
}

void Context::sync() {
  if (host_only_) return;
  drain();
  FDH_HIP(hipSetDevice(device_));
  FDH_HIP(hipStreamSynchronize(stream_));
}

// ------------------------------------------------------------------ frame
void Context::ensure_surfaces() {
  if (host_only_ || (surf_w_ == env_.W && surf_h_ == env_.H && fb_)) return;
  drain();  // the frame in submission still renders into the old surfaces
  FDH_HIP(hipStreamSynchronize(stream_));
  if (fb_) FDH_HIP(hipFree(fb_));
  if (backdrop_) FDH_HIP(hipFree(backdrop_));
  if (blur_tmp_) FDH_HIP(hipFree(blur_tmp_));
  if (alt_) { FDH_HIP(hipFree(alt_)); alt_ = nullptr; }
  if (dbg_snap_) { FDH_HIP(hipFree(dbg_snap_)); dbg_snap_ = nullptr; }
  const size_t n = (size_t)env_.W * env_.H;
  FDH_HIP(hipMalloc((void**)&fb_, n * 4));
  FDH_HIP(hipMalloc((void**)&backdrop_, n * 4));
  FDH_HIP(hipMalloc((void**)&blur_tmp_, n * 4));
  poison_fresh(backdrop_, n * 4); poison_fresh(blur_tmp_, n * 4); poison_fresh(fb_, n * 4);
#if defined(FDH_POISON)  // (fault-hunting builds: the surface starts as 0x11 bytes instead of zeros -- a zero pixel in a frame is then nobody's of ours)
  FDH_HIP(hipMemsetAsync(fb_, 0x11, n * 4, stream_));
#else
  FDH_HIP(hipMemsetAsync(fb_, 0, n * 4, stream_));
#endif
  surf_w_ = env_.W;
  surf_h_ = env_.H;
}

void Context::begin_frame(int w, int h, bool clear, const float rgba[4]) {  // glcontext.nim:2080-2092, 1951-1980
  log_begin_frame(clear, rgba);
  if (env_.frame_begun) throw Error(FDH_ERR_INVALID, "ctx.beginFrame has already been called.");
  if (w <= 0 || h <= 0 || w > 16384 || h > 16384) throw Error(FDH_ERR_INVALID, "beginFrame: frame size must be in 1..16384");
  t_begin_frame_ = std::chrono::steady_clock::now();
  for (auto& v : host_ns_) v = 0;
  if (!host_only_) FDH_HIP(hipSetDevice(device_));
  frame_env_.W = w;
  frame_env_.H = h;
  ensure_surfaces();
  clear_ = clear;
  if (clear) {
    auto q = [](float v) { return (uint32_t)std::floor(clampf(v, 0.0f, 1.0f) * 255.0f + 0.5f); };
    clear_rgba8_ = q(rgba[0]) | (q(rgba[1]) << 8) | (q(rgba[2]) << 16) | (q(rgba[3]) << 24);
  }
  // The records of this frame go into the next set of lanes: the set's last user was the frame kStaging frames ago, whose upload
  // kernel has run by now (that frame's issue was waited for by the end_frame after it: the event is recorded).
  if (!host_only_ && staging_busy_[frame_.next_set()]) { HostTimer t(host_ns_[1]); wait_staging(frame_.next_set()); }
  reset(frame_.begin(w, h));
  frame_env_.binbox_shift = ((w + kBin - 1) / kBin > 128 || (h + kBin - 1) / kBin > 128) ? 1 : 0;
  frame_env_.frame_begun = true;
  frame_env_.pick_frame = pick_on_;
  parallel_groups_ = 0;
  rec_diff_upload_ = false;
  pick_routes();
  // rows a draw has to reach: the frame's, or -- under fdh_set_stripe, when the front-end has told how far the scene's blur nodes
  // reach (render_frame: the per-call path cannot know what is still to come) -- the stripe's, widened by that reach
  frame_env_.cull_y0 = 0; frame_env_.cull_y1 = env_.H;
  if (stripe_y1_ > stripe_y0_ && pending_reach_ >= 0) {
    frame_env_.cull_y0 = std::max(0, std::min(env_.H, stripe_y0_) - pending_reach_);
    frame_env_.cull_y1 = std::min(env_.H, std::max(0, stripe_y1_) + pending_reach_);
  }
  pending_reach_ = -1;
  t_walk_begin_ = std::chrono::steady_clock::now();
  host_ns_[0] = std::chrono::duration_cast<std::chrono::nanoseconds>(t_walk_begin_ - t_begin_frame_).count();
}

// end_frame = prepare (this thread) + issue (the context's submit thread).
//   prepare  lays the frame block out and lists the runs the upload kernel gathers; everything per record was produced while the
//            frame was recorded (commit_bins).  It runs on the CALLING thread.
//   issue    launches the upload kernel and the frame's kernels (~20 us of HIP runtime calls) from the submit thread, so the
//            caller is already walking the next frame's tree.  FDH_CREATE_SYNC_SUBMIT contexts run it inline.
void Context::end_frame() {  // glcontext.nim:1982-1989
  log_end_frame();
  if (!env_.frame_begun) throw Error(FDH_ERR_INVALID, "ctx.beginFrame was not called first.");
  if (mask_depth_ != 0) throw Error(FDH_ERR_INVALID, "Not all masks have been popped.");
  if (!rect_masks_.empty()) throw Error(FDH_ERR_INVALID, "Not all rect masks have been popped.");
  frame_env_.frame_begun = false;
  const auto t0 = std::chrono::steady_clock::now();
  host_ns_[2] = std::chrono::duration_cast<std::chrono::nanoseconds>(t0 - t_walk_begin_).count();
  frame_.close_phase(take_sum());
  frame_.close_piece();
  culled_total_ = culled_draws_;
  const auto t1 = std::chrono::steady_clock::now();
  host_ns_[3] = std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
  // (without what begin_frame waited for the GPU -- the lane set's previous upload: back-pressure, not work)
  host_record_ms_ = std::chrono::duration<float, std::milli>(t1 - t_begin_frame_).count() - (float)host_ns_[1] * 1e-6f;
  // a list entry carries the draw index in 25 bits beside its path code and flags (k_bin_draws, LE_INDEX)
  if (frame_.n_records() >= LE_INDEX) throw Error(FDH_ERR_INVALID, "more than 33 554 430 draw records in one frame");
  {  // picking: the frame's tag table, in painter's order, goes with the frame (a record-only context keeps it as its last frame)
    LaunchJob& T = host_only_ ? job_ : next_;
    T.pick = env_.pick_frame;
    T.pick_depth = frame_.deepest_clip();
    T.pick_tags.clear();
    if (env_.pick_frame) {
      T.pick_tags.resize(frame_.n_records());
      size_t o = 0;
      for (const Piece& p : frame_.pieces()) {
        if (p.n) std::memcpy(static_cast<void*>(T.pick_tags.data() + o), frame_.lane(p.lane).tags.p + p.first, p.n * sizeof(PickTag));
        o += p.n;
      }
    }
  }
  if (host_only_) return;
  // prepare() notes what the device block will hold once this frame's upload has run (blur tables, the retained path's shadow):
  // if the frame is dropped before it is handed over -- prepare or the wait for the previous frame's launches throws, or an
  // inline issue fails -- those notes are void (a later frame would skip uploads the device never received)
  try {
    { HostTimer t(host_ns_[4]); prepare(next_); }
    { HostTimer t(host_ns_[6]); drain(); }  // the previous frame's launches (normally long issued: they ran while this frame was being recorded)
    std::swap(job_, next_);
    have_frame_ = true;
    if (!worker_.joinable()) { issue(job_); return; }
  } catch (...) {
    tables_dev_ = nullptr; shadow_dev_ = nullptr; have_frame_ = false;
    throw;
  }
  {
    std::lock_guard<std::mutex> lk(mu_);
    pending_.store(true, std::memory_order_release);
  }
  cv_job_.notify_one();
}

Recorder& Context::pool_recorder(int slot) {
  while ((int)pool_recs_.size() <= slot) pool_recs_.emplace_back(new Recorder(frame_env_, nullptr));
  return *pool_recs_[(size_t)slot];
}
void Context::use_device_here() const {
  thread_local int t_dev = -1;
  if (!host_only_ && t_dev != device_) { (void)hipSetDevice(device_); t_dev = device_; }
}
// The 4x4 white "rect" atlas image drawRect / drawFilledQuad sample (glcontext.nim:966-970, 1411-1415); it takes atlas space on first
// use exactly like the reference's -- on the calling thread.
void Context::make_rect_image() {
  uint8_t white[4 * 4 * 4];
  std::memset(white, 255, sizeof white);
  put_image(kRectImageKey, 4, 4, white, nullptr);
}
// A blurred snapshot is a barrier in painter's order: close the phase, blur, continue in a new phase.
void Context::blur_node(const DrawRec& quad, const float rect[4], float blur_radius) {
  const std::vector<DrawRec> reopen = close_open_clips();
  frame_.split_phase(take_sum(), (int)frame_.blurs().size());
  set_phase_floor(lane_->recs.n);
  // no clip state to carry: the V pass can composite the quad itself -- unless the region is small enough for the one-kernel
  // route, whose snapshot goes to the backdrop surface and is sampled by the phase's compositor launch (k_blur_small)
  const uint32_t idx = reopen_clips_and_emit(reopen, quad, rect);
  const BBox fb = lane_->bins[idx].box;
  BlurJob job;
  job.taps = make_taps(blur_radius);
  const bool fuse = clip_free() && !(env_.latency_routes && blur_one_kernel_ok(fb.x1 - fb.x0, fb.y1 - fb.y0, job.taps.reach));
  job.fuse_draw = -1;
  if (fuse) {
    job.fuse_draw = (int)frame_.global_index(idx);
    lane_->bins[idx].box = BBox{0, 0, 0, 0};  // never binned: k_blur_v blends it
  }
  commit_bins(idx);
  job.radius = blur_radius;
  job.x0 = fb.x0; job.y0 = fb.y0; job.x1 = fb.x1; job.y1 = fb.y1;
  frame_.add_blur(job);
}
int Context::walk_threads() const { return walk_threads_ >= 0 ? walk_threads_ : WalkPool::default_helpers(); }

// The launches of one prepared frame: the upload (a kernel on the render stream gathering the recorded pieces out of pinned host
// memory), then binning, blur passes and compositing.  Submit thread (or the caller's, FDH_CREATE_SYNC_SUBMIT).
// A frame every phase of which holds at most 64 draws, none of them a rotated quad or a curve (their entries need the bin kernel's
// per-strip tests): no bin launch, the compositor's waves make their entries themselves (k_composite_tiles, "direct").  FDH_DIRECT=0: never.
static bool direct_frame(const LaunchJob& J) {
  // (FDH_FORCE_KERNEL_PATHS=3 / 19 / 8, the test hook that puts a frame on the builds with the slot path / the rotated-quad path: those
  // have no direct form)
  static const bool on = [] { const char* e = std::getenv("FDH_DIRECT"); return !e || std::atoi(e) != 0; }();
  const int forced = forced_kernel_paths();
  if (!on || forced == 3 || forced == 8 || forced == 19) return false;
  if (J.phases.empty() || J.damage) return false;  // (a tracked frame: its signatures are folded over the bin lists)
  for (const Phase& ph : J.phases)
    if (ph.count > 64 || ph.has_rot || ph.has_slow) return false;
  return true;
}

void Context::issue(LaunchJob& J) {
  const auto t_l0 = std::chrono::steady_clock::now();
  FDH_HIP(hipSetDevice(device_));
  {
    UploadTable& T = J.table;
    T.n_runs = 0; T.copy_units = 0;
    for (const UploadRun& r : J.runs) {
      if (T.n_runs >= (uint32_t)kMaxUploadRuns) throw Error(FDH_ERR_UNSUPPORTED, "upload: run table overflow");
      T.run[T.n_runs] = r;
      T.unit_first[T.n_runs] = T.copy_units;
      T.copy_units += (r.bytes + 1023u) / 1024u;
      T.n_runs++;
    }
    launch_upload_frame(stream_, J.d_dst, T);
  }
  // WHO RELEASES THE STAGING SET.  The calling thread may write into a set of lanes again once the upload that read it has run.
  // An event recorded behind the upload said so until round 4 -- and cost the GPU 5.7 - 5.9 us of idle time on every frame: the
  // bin launch started that long after the upload had ended, whether the event was a packet of its own (hipEventRecord) or rode on
  // the upload's dispatch (hipExtLaunchKernelGGL's stop event: 4.6 us), and not at all without one
  // (tools/trace_gaps.sh).  Now the BIN launch says it: its first wave stores the frame's sequence number to a word of pinned host
  // memory (k_bin_draws) -- it has started, so the upload in front of it is done -- and begin_frame compares that word.
  // (A frame without a bin launch -- no phase -- keeps the event.)
  uint32_t seq = 0;
  if (J.staging_slot >= 0) {
    const bool binned = !J.phases.empty() && J.bins_x * J.bins_y > 0 && !direct_frame(J);
    if (binned && !seq_host_) {
      FDH_HIP(hipHostMalloc((void**)&seq_host_, 64, hipHostMallocDefault));
      *seq_host_ = 0;
    }
    if (binned) {
      seq = ++upload_seq_;
      if (seq == 0) seq = ++upload_seq_;  // (0 = no store)
      staging_seq_[J.staging_slot] = seq;
      staging_busy_[J.staging_slot] = 2;
    } else {
      FDH_HIP(hipEventRecord(staging_ev_[J.staging_slot], stream_));
      staging_busy_[J.staging_slot] = 1;
    }
  }
  launch_frame(J, false, seq);
  launch_ms_.store(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_l0).count(), std::memory_order_relaxed);
}


// ---- launch_frame's stages
// profile mode: every launch stamps its own pair of events (set_launch_events: the kernel's execution time, no gaps)
void Context::span_begin(SpanKind kind) { if (profiling_) { Span sp{kind, next_event(), next_event()}; set_launch_events(sp.a, sp.b); spans_.push_back(sp); } }
void Context::span_end() { if (profiling_) { if (!launch_events_used()) spans_.pop_back(); set_launch_events(nullptr, nullptr); } }

// rows each phase has to produce: the stripe, widened by the vertical reach of every later blur
void Context::phase_rows(const LaunchJob& J, std::vector<int>& lo, std::vector<int>& hi) const {
  const int np = (int)J.phases.size();
  int s0 = 0, s1 = J.H;
  if (stripe_y1_ > stripe_y0_) { s0 = std::max(0, stripe_y0_); s1 = std::min(J.H, stripe_y1_); }
  lo.assign(np, 0); hi.assign(np, 0);
  int l = s0, h = s1;
  for (int p = np - 1; p >= 0; p--) {
    lo[p] = l; hi[p] = h;
    if (J.phases[p].blur >= 0) {
      const int reach = J.blurs[J.phases[p].blur].taps.reach;
      l = std::max(0, l - reach);
      h = std::min(J.H, h + reach);
    }
  }
  // the records were culled to rows [rec_y0, rec_y1) when they were made (fdh_set_cull): every row a phase produces must lie inside
  if (s1 > s0 && (l < J.rec_y0 || h > J.rec_y1))
    throw Error(FDH_ERR_INVALID, "the resident draw records were culled to another row stripe: render the frame again after fdh_set_stripe (or fdh_set_cull(0))");
}

BinParams Context::bin_params(const LaunchJob& J, uint32_t upload_seq) const {
  const int np = (int)J.phases.size();
  BinParams B;
  B.binrec = J.dv.binrecs; B.binbox = J.dv.binbox; B.chunkbox = J.dv.chunkbox; B.n_draws = J.n_recs; B.binbox_shift = J.binbox_shift; B.lists = J.lists; B.counts = J.counts; B.phase_first = J.dv.phase_first; B.draws = J.dv.recs; B.exts = J.dv.exts;
  B.refine = 0;
  for (const Phase& ph : J.phases) if (ph.has_rot || ph.has_slow) B.refine = 1;
  B.n_phases = np; B.bins_x = J.bins_x; B.bins_y = J.bins_y; B.stride = J.list_stride;
  if (upload_seq) { B.seq_out = const_cast<uint32_t*>(seq_host_); B.seq = upload_seq; }
  static const bool sub_on = [] { const char* e = std::getenv("FDH_BIN_SUBGRIDS"); return !e || std::atoi(e) != 0; }();
  if (sub_on && np >= 1 && np <= BinParams::kBinSubs) {  // later phases: the bins their compositor launch reads (the same Phase::bin_* box)
    int at = 0;
    for (int p = 0; p < np; p++) {
      const Phase& ph = J.phases[p];
      const bool whole = p == 0;
      const int x0 = whole ? 0 : std::max(0, ph.bin_x0), y0 = whole ? 0 : std::max(0, ph.bin_y0);
      const int x1 = whole ? J.bins_x : std::min(J.bins_x, ph.bin_x1), y1 = whole ? J.bins_y : std::min(J.bins_y, ph.bin_y1);
      const int nx = std::max(0, x1 - x0), ny = std::max(0, y1 - y0);
      B.sub_first[p] = at; B.sub_x0[p] = x0; B.sub_y0[p] = y0; B.sub_nx[p] = std::max(1, nx);
      at += nx * ny;
    }
    B.sub_first[np] = at;
    B.sub_n = np;
  }
  return B;
}

// Phase 0's full-grid composite takes its bins longest-list first, in the order its predecessor sorted (an extra wavefront of that
// launch); it sorts this frame's counts for its successor.  Any permutation is a correct schedule.
Context::Schedule Context::schedule(const LaunchJob& J, bool direct, bool partial) {
  const int nb = J.bins_x * J.bins_y;
  Schedule S;
  const int order_key = J.bins_x * 65536 + J.bins_y;  // entries are (row << 16 | column) of THIS grid
  if (order_valid_ && order_nb_ != order_key) order_valid_ = false;  // frame size changed
  const bool sorting = J.clear && !J.phases.empty() && nb <= 8192 && J.phases[0].count > 0 && !direct && !partial;  // (a direct frame has no counts to sort by)
  if (sorting) {
    S.order_now = order_valid_ ? d_order_[order_read_].ptr : nullptr;
    const int wr = order_valid_ ? 1 - order_read_ : order_read_;
    d_order_[wr].reserve(nb);
    S.order_next = d_order_[wr].ptr;
    order_read_ = wr;
    order_nb_ = order_key;
    order_valid_ = true;
  }
  // Quarter strips for the frame's longest lists (k_composite_tiles, round 6): the sorting waves of earlier full-frame launches left, per
  // class of bins, how many hold at least deep_min draws; that many leading positions of the order (x 8 classes) get four waves per
  // strip.  Whatever value is there serves -- a frame or two stale, 0 before the first launch has run: any count is a correct schedule.
  // The threshold goes by who else renders: a deep strip holds four wave slots and its waves mostly wait, which is what a frame that has
  // the GPU to itself wants (the launch is its longest strips' chain) and what frames of OTHER contexts pay for.  Bench tree through
  // fdh_render_frame (profiles/r06_deep_in_flight.txt): one context, 1080p, 49.7 us per frame without deep strips, 46.6 with bins of >= 24
  // draws, 46.4 with >= 40; four contexts in flight 30.3 / 31.1 / 28.9 us -- so 24 for a device's only context, 40 beside others.
  static const int deep_env = [] { const char* e = std::getenv("FDH_DEEP_MIN"); return e ? std::atoi(e) : -1; }();
  S.deep_min = deep_env >= 0 ? deep_env : (vram_contexts_alive(device_) > 1 ? kDeepMinInFlight : kDeepMinDefault);
  // Block waves (blocks::k_composite_tiles): behind the bins with more than block_max draws -- counted by the same waves into
  // the next eight words -- a wave shades the four strips of a 32 x 32 block.  Before a sorting wave has written them the words say "every
  // bin": one wave per strip.  The threshold bounds what a wave does in series; FDH_BLOCK_MAX overrides it, FDH_BLOCK_WAVES=0 turns the form off.
  // The form pays where frames of SEVERAL contexts are in flight (it spends a sixth fewer wave cycles on the bench frame, which the other
  // contexts' launches use) and costs where a frame has the GPU to itself (a block's four strips in series, at the END of the launch: 26.8 us
  // -> 27.3 at a threshold of 1, 38 at 8): it goes by whether another context has launched on the device in the last few milliseconds, not by
  // whether one exists -- a second context that sits idle must not slow the first.  The sorting waves count against the threshold either way.
  static const int block_env = [] {
    const char* off = std::getenv("FDH_BLOCK_WAVES");
    if (off && std::atoi(off) == 0) return 0;
    const char* e = std::getenv("FDH_BLOCK_MAX");
    return e ? std::min(std::max(std::atoi(e), 0), 254) : -1;
  }();
  const bool shared = device_shared_now(device_, this);
  S.block_max = block_env >= 0 ? block_env : kBlockMaxInFlight;
  const bool block_waves = S.block_max > 0 && (block_env >= 0 || shared);
  if (sorting && (S.deep_min > 0 || S.block_max > 0)) {
    if (!deep_host_) {
      FDH_HIP(hipHostMalloc((void**)&deep_host_, 64, hipHostMallocDefault));
      for (int c = 0; c < 8; c++) { deep_host_[c] = 0; deep_host_[8 + c] = 0xffffffffu; }
    }
    if (S.order_now && S.deep_min > 0) {
      uint32_t most = 0;
      for (int c = 0; c < 8; c++) most = std::max(most, (uint32_t)deep_host_[c]);
      S.deep_k8 = 8 * (int)std::min<uint32_t>(most, 1024u);
    }
    if (S.order_now && block_waves) {
      uint32_t most = 0;
      for (int c = 0; c < 8; c++) most = std::max(most, (uint32_t)deep_host_[8 + c]);
      S.block_k8 = 8 * (int)std::min<uint32_t>(most, 1024u);
    }
  }
  return S;
}

// Phase p's blur node, ahead of its composite: both passes as one kernel out of place (a full-frame node: the surface flips), one kernel into
// the backdrop surface (a small region), or the two passes.  Returns the surface the phase composites into.
uint32_t* Context::launch_blur(const LaunchJob& J, int p, uint32_t* cur, int row_lo, int row_hi, bool partial) {
  const Phase& ph = J.phases[p];
  if (ph.blur < 0) return cur;
  const BlurJob& j = J.blurs[ph.blur];
  const bool big = ph.blur == J.big_blur;
  // V output: footprint rows this phase must produce; H output: those rows widened by the tap reach
  const int vy0 = std::max(j.y0, row_lo), vy1 = std::min(j.y1, row_hi);
  if (vy1 <= vy0 || j.x1 <= j.x0) return cur;
  BlurParams bp;
  bp.W = J.W; bp.H = J.H; bp.pitch = J.W;
  bp.taps = j.taps;
  bp.node_pixels = (long long)(j.x1 - j.x0) * (j.y1 - j.y0);
  bp.fuse_draw = -1;
  bp.mx_w = (size_t)ph.blur < J.mx_w_h.size() ? J.mx_w_h[ph.blur] : nullptr;
  // every pass below reads this frame's surface (`cur`) or, the V pass, what the H pass made of it (blur_tmp_): on an opaque frame the
  // matrix-pipe kernels filter three channels (the fragments' sum was checked when they were built: Context::build_misc)
  bp.opaque = J.opaque ? 1 : 0;
  bp.x0 = j.x0; bp.x1 = j.x1; bp.y0 = vy0; bp.y1 = vy1;
  if ((size_t)ph.blur < J.blur_fused.size() && J.blur_fused[ph.blur]) {
    uint32_t* other = cur == fb_ ? alt_ : fb_;
    bp.src = cur; bp.dst = other;
    bp.fuse_draw = j.fuse_draw;
    span_begin(kSpanBlurFused);
    const bool done = launch_blur_fused(stream_, bp, J.mx_w_v[ph.blur], J.dv.recs, J.dv.exts);
    span_end();
    if (!done) throw Error(FDH_ERR_HIP, "fused blur: no kernel for this filter width (blur_fused_supported out of step with the launcher)");
    return other;
  }
  if (j.fuse_draw < 0 && J.latency_routes && blur_one_kernel_ok(j.x1 - j.x0, j.y1 - j.y0, j.taps.reach)) {
    // a small region: one kernel, source window -> LDS -> horizontal -> LDS -> vertical -> the backdrop surface
    bp.src = cur; bp.dst = backdrop_;
    span_begin(big ? kSpanBigBlurV : kSpanBlurV);
    launch_blur_small(stream_, bp);
    span_end();
    return cur;
  }
  bp.src = cur; bp.dst = blur_tmp_;
  bp.y0 = std::max(0, vy0 - j.taps.reach); bp.y1 = std::min(J.H, vy1 + j.taps.reach);
  const bool guard = partial && j.fuse_draw >= 0;  // (a V pass that composites its quad runs whether its node took damage or not)
  if (guard) damage_.guard(stream_, J, ph.blur, false, cur, vy0, vy1);
  span_begin(big ? kSpanBigBlurH : kSpanBlurH);
  launch_blur_h(stream_, bp);
  span_end();
  bp.src = blur_tmp_; bp.dst = j.fuse_draw >= 0 ? cur : backdrop_;
  bp.mx_w = (size_t)ph.blur < J.mx_w_v.size() ? J.mx_w_v[ph.blur] : nullptr;
  bp.fuse_draw = j.fuse_draw;
  bp.y0 = vy0; bp.y1 = vy1;
  span_begin(big ? kSpanBigBlurV : kSpanBlurV);
  launch_blur_v(stream_, bp, J.dv.recs, J.dv.exts);
  span_end();
  if (guard) damage_.guard(stream_, J, ph.blur, true, cur, vy0, vy1);
  return cur;
}

// phase p's compositor launch into `cur`: the whole grid from the clear colour for the launch that starts the frame, with the schedule;
// the phase's bin box over what the surface holds for a later phase
CompositeParams Context::composite_params(const LaunchJob& J, int p, uint32_t* cur, int row_lo, int row_hi, bool direct, const Schedule& S) const {
  const Phase& ph = J.phases[p];
  const int nb = J.bins_x * J.bins_y;
  const bool full = p == 0 && J.clear;
  CompositeParams C;
  C.lists = J.lists + (size_t)p * nb * J.list_stride;
  C.counts = J.counts + (size_t)p * nb;
  C.backdrop = backdrop_;
  C.fb = cur;
  C.atlas = atlas_.view();
  C.W = J.W; C.H = J.H; C.pitch = J.W;
  C.bins_x = J.bins_x; C.stride = J.list_stride;
  C.bin_x0 = full ? 0 : ph.bin_x0; C.bin_y0 = full ? 0 : ph.bin_y0;
  C.bin_nx = full ? J.bins_x : ph.bin_x1 - ph.bin_x0; C.bin_ny = full ? J.bins_y : ph.bin_y1 - ph.bin_y0;
  C.row_lo = row_lo; C.row_hi = row_hi;
  C.load_fb = full ? 0 : 1;
  C.clear_rgba8 = J.clear_rgba8;
  C.opaque = J.opaque ? 1 : 0;
  C.direct = direct ? 1 : 0; C.direct_first = ph.first; C.direct_n = ph.count; C.binrec = J.dv.binrecs;
  C.order = full ? S.order_now : nullptr; C.order_next = full ? S.order_next : nullptr;
  C.deep_k8 = full ? S.deep_k8 : 0; C.deep_min = S.deep_min;
  static const int deep_strip_min = [] { const char* e = std::getenv("FDH_DEEP_STRIP_MIN"); return e ? std::atoi(e) : kDeepStripMinDefault; }();
  C.deep_strip_min = deep_strip_min;
  C.deep_out = (full && S.order_next && (S.deep_min > 0 || S.block_max > 0)) ? const_cast<uint32_t*>(deep_host_) : nullptr;
  C.block_max = S.block_max; C.block_k8 = full ? S.block_k8 : -1;
  C.has_slow = ph.has_slow; C.has_slow_atlas = ph.has_slow_atlas; C.has_rot = ph.has_rot; C.has_atlas = ph.has_atlas; C.has_masks = ph.has_masks;
  C.mask_spill = J.mask_spill; C.spill_stride = J.spill_stride;
  return C;
}

// The launches of a frame, in stream order: binning, damage tracking's, then per phase its blur node and its compositor launch.
void Context::launch_frame(const LaunchJob& J, bool profile, uint32_t upload_seq) {
  profiling_ = profile;
  std::vector<int> lo, hi;
  phase_rows(J, lo, hi);
  const bool direct = direct_frame(J);
  const BinParams B = bin_params(J, upload_seq);
  span_begin(kSpanBin); if (!direct) launch_bin(stream_, B); span_end();
  const bool partial = damage_.launch(stream_, J, B, readback_, [this](bool begin) { if (begin) span_begin(kSpanBin); else span_end(); });
  const Schedule S = schedule(J, direct, partial);
  // The surface that holds the live image.  A fused full-frame blur renders out of place and flips it; a frame that flips an odd
  // number of times ends in alt_, and the two pointers trade places: the frame surface IS the one the frame ended in
  // (fdh_frame_device_ptr is asked again after every frame).  Phase 0 always starts in fb_, i.e. on the surface the previous
  // frame's last pass WROTE: starting in the other one -- the surface that pass had only read -- cost the phase-0 launch 2 us
  // (32.1 against 30.2: its 33 MB of stores then land on lines other XCDs' L2s hold clean copies of).
  uint32_t* cur = fb_;
  for (int p = 0; p < (int)J.phases.size(); p++) {
    cur = launch_blur(J, p, cur, lo[p], hi[p], partial);
    CompositeParams C = composite_params(J, p, cur, lo[p], hi[p], direct, S);
    if (C.load_fb == 0) {  // (the launch that starts the frame: its deep strips, its block waves)
      const CompositeBuild cb = composite_build(C);
      stats_.deep_bins = (float)cb.deep_k8;
      block_wave_bins_ = cb.block && !partial ? std::max(C.bin_nx * C.bin_ny - cb.block_k8, 0) : -1;
    }
    span_begin(p == 0 ? kSpanCompositeMain : kSpanCompositeLater);
    if (partial) damage_.composite(stream_, J, C);
    else launch_composite(stream_, J.dv.recs, J.dv.exts, C);
    span_end();
  }
  if (cur != fb_) std::swap(fb_, alt_);  // the frame ended in the other surface: it is the frame surface now
  damage_.launched_whole(J);
  FDH_HIP(hipGetLastError());
}

void Context::replay(int times) {
  need_device("replay");
  drain();
  if (!have_frame_) throw Error(FDH_ERR_INVALID, "replay: no frame has been submitted");
  FDH_HIP(hipSetDevice(device_));
  if (times <= 0) return;
  FDH_HIP(hipEventRecord(ev_[0], stream_));
  for (int i = 0; i < times; i++) launch_frame(job_, false);
  FDH_HIP(hipEventRecord(ev_[1], stream_));
  FDH_HIP(hipEventSynchronize(ev_[1]));
  float ms = 0.0f;
  FDH_HIP(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
  stats_.ms_total = ms / (float)times;
}

// enqueue only: several contexts (own streams, own surfaces) can then have frames in flight on one GPU at once
void Context::replay_async(int times) {
  need_device("replay_async");
  drain();
  if (!have_frame_) throw Error(FDH_ERR_INVALID, "replay: no frame has been submitted");
  FDH_HIP(hipSetDevice(device_));
  for (int i = 0; i < times; i++) launch_frame(job_, false);
}

// `times` frames back to back with one event between consecutive frames: ms_out[i] = duration of frame i on the stream
void Context::replay_timed(int times, float* ms_out) {
  need_device("replay_timed");
  drain();
  if (!have_frame_) throw Error(FDH_ERR_INVALID, "replay: no frame has been submitted");
  if (times <= 0 || !ms_out) return;
  FDH_HIP(hipSetDevice(device_));
  ev_used_ = 0;
  std::vector<hipEvent_t> marks;
  marks.push_back(next_event());
  FDH_HIP(hipEventRecord(marks.back(), stream_));
  for (int i = 0; i < times; i++) {
    launch_frame(job_, false);
    marks.push_back(next_event());
    FDH_HIP(hipEventRecord(marks.back(), stream_));
  }
  FDH_HIP(hipEventSynchronize(marks.back()));
  for (int i = 0; i < times; i++) FDH_HIP(hipEventElapsedTime(&ms_out[i], marks[i], marks[i + 1]));
}

hipEvent_t Context::next_event() {
  if (ev_used_ == ev_pool_.size()) {
    hipEvent_t e;
    FDH_HIP(hipEventCreate(&e));
    ev_pool_.push_back(e);
  }
  return ev_pool_[ev_used_++];
}

// Per-kernel timing: events bracket every launch, so this is kept apart from replay()'s batch timing.
void Context::profile(int times) {
  need_device("profile");
  drain();
  if (!have_frame_) throw Error(FDH_ERR_INVALID, "profile: no frame has been submitted");
  FDH_HIP(hipSetDevice(device_));
  if (times <= 0) return;
  double acc[kSpanKinds] = {};
  for (int i = 0; i < times; i++) {
    ev_used_ = 0;
    spans_.clear();
    launch_frame(job_, true);
    FDH_HIP(hipStreamSynchronize(stream_));
    for (auto& sp : spans_) {
      float t = 0.0f;
      if (hipEventElapsedTime(&t, sp.a, sp.b) == hipSuccess) acc[sp.kind] += t;  // (a span whose launch had nothing to do never stamped its events)
      else (void)hipGetLastError();
    }
  }
  stats_.ms_bin = (float)(acc[kSpanBin] / times);
  stats_.ms_composite_main = (float)(acc[kSpanCompositeMain] / times);
  stats_.ms_composite = (float)((acc[kSpanCompositeMain] + acc[kSpanCompositeLater]) / times);
  stats_.ms_blur_h = (float)((acc[kSpanBlurH] + acc[kSpanBigBlurH]) / times);
  stats_.ms_blur_v = (float)((acc[kSpanBlurV] + acc[kSpanBigBlurV]) / times);
  stats_.ms_blur_big_h = (float)(acc[kSpanBigBlurH] / times);
  stats_.ms_blur_big_v = (float)(acc[kSpanBigBlurV] / times);
  stats_.ms_blur_fused = (float)(acc[kSpanBlurFused] / times);
}

// ------------------------------------------------------------------ readback (glcontext.nim:2094-2135)
void Context::read_pixels(int x, int y, int w, int h, uint8_t* out) {
  need_device("read_pixels");
  drain();
  if (!fb_) throw Error(FDH_ERR_INVALID, "readPixels before the first frame");
  FDH_HIP(hipSetDevice(device_));
  if (w <= 0 || h <= 0) { x = 0; y = 0; w = env_.W; h = env_.H; }
  if (x < 0 || y < 0 || x + w > env_.W || y + h > env_.H) throw Error(FDH_ERR_INVALID, "readPixels: rectangle outside the frame");
  FDH_HIP(hipStreamSynchronize(stream_));
  FDH_HIP(hipMemcpy2D(out, (size_t)w * 4, fb_ + (size_t)y * env_.W + x, (size_t)env_.W * 4, (size_t)w * 4, h, hipMemcpyDeviceToHost));
}
// fdh_read_video_frame, fdh_read_video_planes, fdh_read_video_422 and fdh_read_video_alpha (include_video/): the context's part -- the last
// frame is complete, and where it lies (a frame with a fused full-frame blur ends in the other surface: fb_ behind drain(), as read_pixels
// takes it); the rest is fdh_video_out.cpp's
template <class Target>
void Context::read_video(const char* who, void (*read)(hipStream_t, int, const uint32_t*, int, int, const Target*, const video_out::Own*, int), const Target* target) {
  const std::string name = who;
  if (host_only_) throw Error(FDH_ERR_INVALID, name + ": this context was created with FDH_CREATE_RECORD_ONLY (it records calls, it draws nothing)");
  drain();
  // (a begin_frame of another size has made new surfaces: the last frame is gone with the old ones)
  if (!have_frame_ || !fb_ || job_.W != surf_w_ || job_.H != surf_h_) throw Error(FDH_ERR_INVALID, name + ": no frame has been submitted");
  if (stripe_y1_ > stripe_y0_) throw Error(FDH_ERR_INVALID, name + ": not under fdh_set_stripe");
  FDH_HIP(hipSetDevice(device_));
  const size_t surface = (size_t)surf_w_ * surf_h_ * 4;
  std::vector<video_out::Own> own = {{fb_, surface, "frame surface"}, {alt_, surface, "frame surface"}, {backdrop_, surface, "backdrop surface"}, {blur_tmp_, surface, "blur surface"}};
  for (int l = 0; l < atlas_.n_levels(); l++) own.push_back({atlas_.level(l), (size_t)(atlas_.size() >> l) * (atlas_.size() >> l) * 4, "atlas"});
  FDH_HIP(hipStreamSynchronize(stream_));
  read(stream_, device_, fb_, surf_w_, surf_h_, target, own.data(), (int)own.size());
}
void Context::read_video_frame(const FdhVideoTarget* target) { read_video("read_video_frame", video_out::read, target); }
void Context::read_video_planes(const FdhVideoPlanesTarget* target) { read_video("read_video_planes", video_out::read_planes, target); }
void Context::read_video_422(const FdhVideoPlanesTarget* target) { read_video("read_video_422", video_out::read_422, target); }
void Context::read_video_alpha(const FdhVideoAlphaPlanesTarget* target) { read_video("read_video_alpha", video_out::read_alpha, target); }
// ------------------------------------------------------------------ damage tracking, damage readback: the context's part (fdh_damage.cpp)
void Context::set_damage_tracking(bool on) {
  if (on && host_only_) throw Error(FDH_ERR_INVALID, "fdh_set_damage_tracking: a record-only context composites nothing");
  drain();
  if (on && stripe_y1_ > stripe_y0_) throw Error(FDH_ERR_INVALID, "fdh_set_damage_tracking: not under fdh_set_stripe");
  damage_.on = on;
}
void Context::damage_bins(uint8_t* mask, int cap, int* bins_x, int* bins_y, int* n_damaged, bool changed_only) {
  need_device("fdh_damage_bins");
  drain();
  if (!have_frame_) throw Error(FDH_ERR_INVALID, "fdh_damage_bins: no frame has been submitted");
  const int gx = job_.bins_x, gy = job_.bins_y, nb = gx * gy;
  if (mask && cap < nb) throw Error(FDH_ERR_INVALID, "fdh_damage_bins: the mask holds fewer bytes than the frame has bins");
  FDH_HIP(hipSetDevice(device_));
  FDH_HIP(hipStreamSynchronize(stream_));
  const std::vector<uint8_t> m = damage_.bins(gx, gy, changed_only);
  int n = 0;
  for (uint8_t v : m) n += v ? 1 : 0;
  if (mask) std::memcpy(mask, m.data(), (size_t)nb);
  if (bins_x) *bins_x = gx;
  if (bins_y) *bins_y = gy;
  if (n_damaged) *n_damaged = n;
}
void Context::set_damage_readback(bool on) {
  if (on && host_only_) throw Error(FDH_ERR_INVALID, "fdh_set_damage_readback: a record-only context composites nothing");
  if (host_only_) return;
  drain();
  if (on && stripe_y1_ > stripe_y0_) throw Error(FDH_ERR_INVALID, "fdh_set_damage_readback: not under fdh_set_stripe");
  FDH_HIP(hipSetDevice(device_));
  readback_.turn(on, stream_);
}
ReadFrame Context::read_frame(const char* who) {
  need_device(who);
  drain();
  if (!readback_.on) throw Error(FDH_ERR_INVALID, std::string(who) + ": damage readback is off (fdh_set_damage_readback)");
  if (!have_frame_ || !fb_) throw Error(FDH_ERR_INVALID, std::string(who) + ": no frame has been submitted");
  FDH_HIP(hipSetDevice(device_));
  FDH_HIP(hipStreamSynchronize(stream_));
  return ReadFrame{stream_, fb_, job_.W, job_.H, job_.bins_x, job_.bins_y};
}
void Context::read_damage(const FdhDamageTile** tiles, const uint8_t** pixels, int* n_tiles, int* frame_w, int* frame_h, int* full) {
  readback_.read_raw(read_frame("fdh_read_damage"), tiles, pixels, n_tiles, frame_w, frame_h, full);
}
void Context::read_damage_into(uint8_t* image, int64_t pitch_bytes, int w, int h, int* n_tiles) {
  readback_.read_into(read_frame("fdh_read_damage_into"), image, pitch_bytes, w, h, n_tiles);
}
void Context::read_damage_coded(const FdhCodedTile** tiles, const uint8_t** payload, int* n_tiles, int64_t* payload_bytes, int* frame_w, int* frame_h, int* full) {
  readback_.read_coded(read_frame("fdh_read_damage_coded"), tiles, payload, n_tiles, payload_bytes, frame_w, frame_h, full);
}
void Context::set_damage_exact(bool on) {
  if (on && host_only_) throw Error(FDH_ERR_INVALID, "fdh_set_damage_exact: a record-only context composites nothing");
  if (host_only_) return;
  drain();
  FDH_HIP(hipSetDevice(device_));
  readback_.turn_exact(on, stream_);
}
void Context::damage_exact_stats(int* n_pending, int* n_changed, int* fresh) {
  drain();
  readback_.exact_stats(n_pending, n_changed, fresh);
}
void Context::read_damage_moved(const FdhDamageMove* moves, int n_moves, const FdhCodedTile** tiles, const uint8_t** payload, int* n_tiles,
                                int64_t* payload_bytes, int* frame_w, int* frame_h, int* full, int* n_copied) {
  readback_.read_moved(read_frame("fdh_read_damage_moved"), moves, n_moves, tiles, payload, n_tiles, payload_bytes, frame_w, frame_h, full, n_copied);
}
void Context::find_damage_moves(int max_shift, FdhDamageMove* out_moves, int* out_votes, int cap, int* n_out) {
  readback_.find_moves(read_frame("fdh_find_damage_moves"), max_shift, out_moves, out_votes, cap, n_out);
}

void Context::frame_device_ptr(void** p, int* w, int* h, int64_t* pitch_bytes) {
  need_device("frame_device_ptr");
  drain();
  if (!fb_) throw Error(FDH_ERR_INVALID, "no frame surface yet");
  *p = fb_; *w = env_.W; *h = env_.H; *pitch_bytes = (int64_t)env_.W * 4;
}

}  // namespace fdh
