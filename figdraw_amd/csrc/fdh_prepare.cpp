// fdh_prepare.cpp -- end_frame's half on the calling thread: the recorded frame -> the frame block's layout, the runs the upload
// kernel gathers, the launch description (LaunchJob).  Also what only this step needs: the f16 blur weight tables.
#include "fdh_context.h"
#include "fdh_damage.h"
#include "fdh_host.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

namespace fdh {

// Weight fragments of a matrix-pipe blur pass (k_blur_mx, k_blur_mx.hip).  Lane (j, g) of fragment m holds, for the window
// texels 16 m + 8 g + t (t = 0..7) of a 32-output block, the tap each meets at output j: k = texel - delta - j, weight
// q[k] (the tap at scale 2^10 as one f16: quantise_taps_f16 below) when 0 <= k <= 2 reach, else 0.  Every product with an 8-bit
// texel is exact in f32.  (Rounds 2 - 4 carried a second half, lo = RNE(w - hi), 22 significant bits: its slot in the layout remains, zero.)
static uint16_t half_bits_rne(float f) {  // |f| < 65504
  uint32_t u;
  std::memcpy(&u, &f, 4);
  const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
  const float a = std::fabs(f);
  if (a == 0.0f) return sign;
  std::memcpy(&u, &a, 4);
  const int e = (int)(u >> 23) - 127;
  if (e < -14) return sign | (uint16_t)std::nearbyint(a * 16777216.0f);  // subnormal half: units of 2^-24 (1024 = the smallest normal)
  const uint32_t mant = u & 0x7fffffu, m = mant >> 13, rem = mant & 0x1fffu;
  uint32_t h = ((uint32_t)(e + 15) << 10) | m;
  if (rem > 0x1000u || (rem == 0x1000u && (m & 1u))) h++;  // round to nearest even; a carry moves into the exponent
  return sign | (uint16_t)h;
}
static float half_value(uint16_t h) {
  const int e = (h >> 10) & 31, m = h & 1023;
  const float v = e == 0 ? std::ldexp((float)m, -24) : std::ldexp((float)(m + 1024), e - 25);
  return (h & 0x8000u) ? -v : v;
}
// Round 5: the taps as ONE f16 each at scale 2^10 (the kernels multiply once per operand and k-step: FDH_MX_LO in fdh_types.h).
// Rounded from the CENTRE tap outwards, the rounding error carried to the next tap out (the filter is symmetric: each side takes half
// of the centre's error): a tap's error is made good by its neighbour, and what is left at the end falls on the outermost taps, whose
// f16 steps are thousands of times finer than the centre's -- the sum of the weights is kept to ~1e-7 (a flat region keeps its value)
// and the error is a fine alternating pattern that smooth content cancels.  (Measured, numpy, two passes with RGBA8 between them, against
// the exact taps: 0.00 - 0.23 % of a UI-like image's texels move, by one LSB; 0.4 - 1.0 % of white noise's.  Rounding every tap on its
// own moves 0.3 - 1.0 % / 2 - 8 %; carrying the error from the outside in and letting the centre tap keep the sum, 0.2 - 0.7 %: the
// centre tap's step is the coarsest of all.)  q[k], k = 0 .. 2 reach, in units of 2^-10.
static void quantise_taps_f16(const BlurTaps& t, float* q) {
  const int r = t.reach;
  const double centre = (double)t.dense[kBlurPad + r] * 1024.0;
  q[r] = half_value(half_bits_rne((float)centre));
  double carry = 0.5 * (centre - (double)q[r]);
  for (int k = r - 1; k >= 0; k--) {
    if (t.dense[kBlurPad + k] == 0.0f) { q[k] = q[2 * r - k] = 0.0f; continue; }  // (a texel the merged FIR does not read stays unread: the error waits for the next tap)
    const double want = std::max((double)t.dense[kBlurPad + k] * 1024.0 + carry, 0.0);
    const float v = half_value(half_bits_rne((float)want));
    carry = want - (double)v;
    q[k] = q[2 * r - k] = v;
  }
}
// Returns how far the fragments' weights, summed per output over the whole window as the kernels sum them, lie from the scale (1024) at
// most: what decides whether an all-255 plane filters to 255 (kMxOpaqueSumBound, fdh_context.h).
static float build_mx_weights(const BlurTaps& t, bool vertical, uint8_t* out) {
  const int nk = mx_nk(t.reach, vertical), delta = mx_delta(t.reach, vertical);
  uint16_t* o = reinterpret_cast<uint16_t*>(out);
  float q[2 * kMaxBlurReach + 1];
  quantise_taps_f16(t, q);
  double sum[32] = {};
  for (int m = 0; m < nk; m++)
    for (int lane = 0; lane < 64; lane++) {
      const int j = lane & 31, g = lane >> 5;
      for (int e = 0; e < 8; e++) {
        // which window texel element e of lane group g stands for (mx_krow, fdh_types.h): the natural order for the horizontal pass;
        // for the vertical one the order in which a 32 x 32 accumulator tile holds its rows, so that the fused kernel's horizontal
        // product feeds the vertical one from registers (k_blur_fx) -- any order serves as long as both operands use the same
        const int k = 16 * m + mx_krow(g, e, vertical) - delta - j;
#if FDH_MX_LO  // (variant builds: the 22-bit weights of rounds 2 - 4, hi = RNE(w), lo = RNE(w - hi); the kernels then multiply twice)
        const float w = (k >= 0 && k <= 2 * t.reach) ? t.dense[kBlurPad + k] * 1024.0f : 0.0f;
        const uint16_t hi = half_bits_rne(w), lo = half_bits_rne(w - half_value(hi));
#else
        const float w = (k >= 0 && k <= 2 * t.reach) ? q[k] : 0.0f;
        const uint16_t hi = half_bits_rne(w), lo = 0;  // (the fragment layout keeps the second half's slot: zeros)
#endif
        o[(((size_t)(2 * m) * 64 + lane) * 8) + e] = hi;
        o[(((size_t)(2 * m + 1) * 64 + lane) * 8) + e] = lo;
        sum[j] += (double)half_value(hi) + (double)half_value(lo);
      }
    }
  double dev = 0.0;
  for (int j = 0; j < 32; j++) dev = std::max(dev, std::fabs(sum[j] - 1024.0));
  return (float)dev;
}

void blur_weight_fragments(float blur_radius, bool vertical, float* dense, uint16_t* frag_bits, int* reach, int* k_steps) {
  const BlurTaps t = make_taps(blur_radius);
  for (int k = 0; k <= 2 * t.reach; k++) dense[k] = t.dense[kBlurPad + k];
  *reach = t.reach;
  *k_steps = mx_nk(t.reach, vertical);
  if (*k_steps > kMxMaxNK) throw Error(FDH_ERR_INVALID, "blur_weight_fragments: filter too wide");
  build_mx_weights(t, vertical, reinterpret_cast<uint8_t*>(frag_bits));
}

// ------------------------------------------------------------------ the frame block's layout
// records | extensions | bin records | bin boxes | chunk boxes | phase table | blur weight tables, each on a 256-byte boundary
void FrameLayout::lay_out(size_t n_recs, size_t n_exts, size_t n_phases, const std::vector<BlurJob>& blurs) {
  n = n_recs; n_ext = n_exts;
  n_chunks = std::max<size_t>((n + 255) / 256, 1);
  recs = 0;
  exts = align256(recs + n * sizeof(DrawRec));
  binrecs = align256(exts + n_ext * sizeof(QuadExt));
  boxes = align256(binrecs + n * sizeof(BinRec));
  chunks = align256(boxes + ((n + 3) & ~(size_t)3) * sizeof(uint32_t));
  phase_first = align256(chunks + n_chunks * sizeof(uint32_t));
  tables = align256(phase_first + (n_phases + 1) * sizeof(int));
  total = tables;
  // weight fragments of the matrix-pipe blur passes, two tables (H, V) per blur job
  mx_h.assign(blurs.size(), 0); mx_v.assign(blurs.size(), 0);
  for (size_t i = 0; i < blurs.size(); i++) {
    const int nkh = mx_nk(blurs[i].taps.reach, false), nkv = mx_nk(blurs[i].taps.reach, true);
    if (nkh > kMxMaxNK || nkv > kMxMaxNK) continue;
    mx_h[i] = total; total = align256(total + mx_table_bytes(nkh));
    mx_v[i] = total; total = align256(total + mx_table_bytes(nkv));
  }
}

// ------------------------------------------------------------------ prepare (calling thread) and its stages
void Context::prepare(LaunchJob& J) {
  const auto t_s0 = std::chrono::steady_clock::now();
  FDH_HIP(hipSetDevice(device_));
  describe_frame(J);
  size_bin_buffers(J);
  layout_frame_block(J);
  choose_fused_blurs(J);
  if (frame_.pieces().size() * 3 + 2 > (size_t)kMaxUploadRuns) consolidate_pieces();  // more pieces than the upload's kernel-argument table holds
  const FoldGuard fold = fold_clear(J);
  decide_opaque(J);
  damage_frame_key(J);
  const bool shadow_ok = shadow_usable(J), resident = tables_resident(J, shadow_ok);
  build_misc(J, resident);
  if (!patch_runs(J, shadow_ok)) gather_runs(J, resident);
  tables_dev_ = d_frame_.ptr; tables_layout_ = J.layout; tables_sig_.swap(tables_sig_next_);  // what the block holds once this upload has run
  account_frame(J);
  fence_staging();
  stats_.ms_host_record = host_record_ms_;
  stats_.ms_host_upload = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_s0).count();
}

// what the launch side reads of the recorded frame, copied: the recording side moves on to the next frame
void Context::describe_frame(LaunchJob& J) {
  J.W = env_.W; J.H = env_.H; J.clear = clear_; J.clear_rgba8 = clear_rgba8_;
  J.rec_y0 = culling() ? env_.cull_y0 : 0; J.rec_y1 = culling() ? env_.cull_y1 : env_.H;
  J.latency_routes = env_.latency_routes;
  J.phases = frame_.phases();  // (copies: the recording side keeps its own for fdh_debug_record_digest)
  J.blurs = frame_.blurs();
  J.n_recs = (int)frame_.n_records();
  J.n_exts = (int)frame_.n_extensions();
  J.bins_x = (env_.W + kBin - 1) / kBin;
  J.bins_y = (env_.H + kBin - 1) / kBin;
  J.binbox_shift = env_.binbox_shift;
  J.staging_slot = frame_.set();
}

void Context::size_bin_buffers(LaunchJob& J) {
  const int nb = J.bins_x * J.bins_y;
  // List stride = the largest number of draws any bin of any phase can receive: counted while the frame was recorded
  // (Lane::count_add / count_close per phase; lanes of pool threads add their own maxima: an upper bound)
  J.list_stride = (frame_.list_stride() + 7) & ~7;
  reserve_quiet(d_lists_, (size_t)J.phases.size() * nb * J.list_stride);
  reserve_quiet(d_counts_, (size_t)J.phases.size() * nb);
  J.lists = d_lists_.ptr; J.counts = d_counts_.ptr;
  // clip nesting beyond the LDS stack (kMaskDepth levels): one global plane per extra level, 256 bytes per strip
  J.mask_spill = nullptr;
  J.spill_stride = (size_t)nb * 16 * 64;
  if (frame_.deepest_clip() > kMaskDepth) {
    const size_t levels = (size_t)(frame_.deepest_clip() - kMaskDepth);
    if (levels * J.spill_stride * sizeof(uint32_t) > ((size_t)2 << 30))
      throw Error(FDH_ERR_UNSUPPORTED, "clip masks nested too deep for this frame size (the spill plane would exceed 2 GiB)");
    reserve_quiet(d_mask_spill_, levels * J.spill_stride);
    J.mask_spill = d_mask_spill_.ptr;
  }
}

// the one place that turns the layout into pointers and offsets the launches use
void Context::layout_frame_block(LaunchJob& J) {
  FrameLayout& F = J.layout;
  F.lay_out(frame_.n_records(), frame_.n_extensions(), J.phases.size(), J.blurs);
  if (F.total >= ((size_t)1 << 32)) throw Error(FDH_ERR_UNSUPPORTED, "frame block beyond 4 GiB");
  reserve_quiet(d_frame_, F.total);
  uint8_t* const d = d_frame_.ptr;
  J.d_dst = d;
  LaunchJob::View& dv = J.dv;
  dv.recs = reinterpret_cast<DrawRec*>(d + F.recs);
  dv.exts = reinterpret_cast<QuadExt*>(d + F.exts);
  dv.binrecs = reinterpret_cast<BinRec*>(d + F.binrecs);
  dv.phase_first = reinterpret_cast<int*>(d + F.phase_first);
  dv.binbox = reinterpret_cast<uint32_t*>(d + F.boxes);
  dv.chunkbox = reinterpret_cast<uint32_t*>(d + F.chunks);
  J.mx_w_h.assign(J.blurs.size(), nullptr);
  J.mx_w_v.assign(J.blurs.size(), nullptr);
  for (size_t i = 0; i < J.blurs.size(); i++)
    if (F.mx_h[i]) { J.mx_w_h[i] = reinterpret_cast<const uint4*>(d + F.mx_h[i]); J.mx_w_v[i] = reinterpret_cast<const uint4*>(d + F.mx_v[i]); }
  J.table = UploadTable{};
  J.table.n_draws = (uint32_t)F.n; J.table.binbox_shift = (uint32_t)J.binbox_shift;
  J.table.bins_off = (uint32_t)F.binrecs; J.table.box_off = (uint32_t)F.boxes;
}

// A blur node that covers the whole frame, composited by its own vertical pass (no clip open), in a frame that starts from
// the clear colour: both passes as ONE kernel, out of place (k_blur_fx) -- launch_frame alternates between fb_ and alt_.
// Which route is a matter of speed only -- the two give the same pixels bit for bit (tests/test_hip_parity.py): Context::pick_routes.
void Context::choose_fused_blurs(LaunchJob& J) {
  const bool fx_on = env_.latency_routes;  // (decided when the frame began: Context::pick_routes)
  J.blur_fused.assign(J.blurs.size(), 0);
  J.n_fused = 0;
  for (size_t i = 0; i < J.blurs.size(); i++) {
    const BlurJob& j = J.blurs[i];
    // (frames under 0.4 Mpx keep the two small-region passes, like every region of that size: launch_blur_h)
    static const bool any_size = [] { const char* e = std::getenv("FDH_FORCE_BLUR_PATH"); return e && std::atoi(e) == 3; }();
    if (fx_on && clear_ && j.fuse_draw >= 0 && J.mx_w_h[i] && j.x0 == 0 && j.y0 == 0 && j.x1 == env_.W && j.y1 == env_.H && blur_fused_supported(j.taps.reach, env_.W, env_.W) &&
        (any_size || (long long)env_.W * env_.H >= 384 * 1024)) {
      J.blur_fused[i] = 1;
      J.n_fused++;
    }
  }
  if (J.n_fused > 0 && !alt_) {
    FDH_HIP(hipMalloc((void**)&alt_, (size_t)env_.W * env_.H * 4));
    poison_fresh(alt_, (size_t)env_.W * env_.H * 4);
    FDH_HIP(hipMemsetAsync(alt_, 0, (size_t)env_.W * env_.H * 4, stream_));
  }
}

// CLEAR FOLDING.  A frame that is cleared and whose first draw is one colour at full coverage over the whole frame -- a window's
// background rectangle, the first node of nearly every UI tree (the bench scene's is translucent white over the clear colour)
// -- starts, in effect, from another clear colour: blend(clear, colour), the very arithmetic the compositor's uniform-blend path
// applies to every strip (blend_pre: F = rint(fma(F, 1 - sa, c * 255 sa)) per channel, IEEE single, no approximations), computed
// once here.  The draw's bin record goes to the device with empty bounds (it is never binned); the lanes keep what was recorded
// (fdh_debug_record_digest): the guard puts the bounds back when prepare is left, by return or by exception.  Bench frame: 32 640
// uniform blends fewer, 8 % of the phase-0 launch's VALU instructions.
Context::FoldGuard Context::fold_clear(LaunchJob& J) {
  FoldGuard g;
  static const bool fold_on = [] { const char* e = std::getenv("FDH_FOLD_CLEAR"); return !e || std::atoi(e) != 0; }();
  if (fold_on && clear_ && !frame_.pieces().empty() && J.phases[0].count > 0) {
    const Piece& p0 = frame_.pieces()[0];
    Lane& L = frame_.lane(p0.lane);
    BinRec& br = L.bins[p0.first];
    const DrawRec& r = L.recs[p0.first];
    const uint32_t om = r.op_mode;
    if (((om >> 12) & 15u) == OP_DRAW && (br.flags & LE_PLAIN) && !(br.flags & BR_CORE_REMOVED) && (br.flags & BR_HAS_CORE) && br.ix0 <= 0 && br.iy0 <= 0 &&
        br.ix1 >= env_.W && br.iy1 >= env_.H && br.box.x0 <= 0 && br.box.y0 <= 0 && br.box.x1 >= env_.W && br.box.y1 >= env_.H) {
      const float inv255 = 1.0f / 255.0f;
      const uint32_t c = r.col[0];
      float cf[3];
      std::memcpy(cf, &r.col[1], sizeof cf);  // (device form: r, g, b / 255 as floats -- Recorder::commit_bins)
      const float sa = (float)(c >> 24) * inv255, A = 255.0f * sa, ia = 1.0f - sa;
      const float src[4] = {cf[0] * A, cf[1] * A, cf[2] * A, A};
      uint32_t out = 0;
      for (int k = 0; k < 4; k++) {
        const float F = (float)((J.clear_rgba8 >> (8 * k)) & 255u);
        const float v = std::nearbyintf(std::fmaf(F, ia, src[k]));  // (round to nearest even, like v_rndne_f32)
        out |= (uint32_t)std::min(std::max((int)v, 0), 255) << (8 * k);
      }
      J.clear_rgba8 = out;
      g.br = &br;
      g.box = br.box;
      br.box = BBox{0, 0, 0, 0};
      if (p0.lane > 0) L.publish_bytes(1, (size_t)p0.first * sizeof(BinRec), sizeof(BinRec));  // (a pool thread published the piece already)
    }
  }
  stats_.clear_folded = g.br ? 1.0f : 0.0f;
  return g;
}

// AN OPAQUE SURFACE.  A frame that is cleared with a colour of alpha 255 -- after clear folding: a translucent clear under an opaque
// background panel counts -- holds alpha 255 on every pixel from its first launch to its last: every draw reaches the surface through
// A' = rint(fma(A, 1 - sa, 255 sa)), which is 255 for A = 255 and every float sa the shading can produce (tests/test_opaque_host.py tries
// every float in [-2^-10, 1 + 2^-10]), and the blur of an all-255 plane is 255 (the weight fragments sum to the scale: build_mx_weights,
// kMxOpaqueSumBound).  The launches of such a frame may take kernels that do not carry the alpha channel: k_composite_tiles<4 | 32>, the
// kOpaque forms of k_blur_mx / k_blur_fx.  Decided per frame and never carried over: a frame that is not cleared starts from a surface
// others may have written (fdh_frame_device_ptr).  FDH_OPAQUE=0 turns it off (same pixels; one of the switches tools/suite_off_defaults.sh runs).
void Context::decide_opaque(LaunchJob& J) const {
  static const bool opaque_on = [] { const char* e = std::getenv("FDH_OPAQUE"); return !e || std::atoi(e) != 0; }();
  J.opaque = opaque_on && clear_ && (J.clear_rgba8 >> 24) == 255u;
}

// Damage tracking: the frame key -- everything a bin's pixels depend on besides its lists and the records they index.  A tracked frame
// whose key differs from the last tracked frame's is rendered in full (DamageTracker::launch), and so is one the tracking launches cannot
// take: no clear (its starting pixels are not this frame's to rebuild), a full-frame blur that renders out of place (k_blur_fx flips the
// frame surface), more blur nodes than k_damage_resolve takes.  (the atlas epoch moves with every put, update, remove and reset: any atlas
// change is a full frame, on purpose.)
void Context::damage_frame_key(LaunchJob& J) const {
  J.damage = damage_.on;
  J.damage_force = !clear_ || J.n_fused > 0 || J.blurs.size() > (size_t)kDamageMaxNodes;
  uint64_t k = 1469598103934665603ull;
  auto mix = [&k](uint64_t v) { for (int b = 0; b < 8; b++) { k ^= (v >> (8 * b)) & 255u; k *= 1099511628211ull; } };
  uint32_t aa_bits = 0, ps_bits = 0;
  std::memcpy(&aa_bits, &ctx_aa_, 4); std::memcpy(&ps_bits, &pixel_scale_, 4);
  mix((uint64_t)(uint32_t)env_.W << 32 | (uint32_t)env_.H); mix((uint64_t)(uint32_t)J.bins_x << 32 | (uint32_t)J.bins_y);
  mix((uint64_t)J.clear_rgba8 << 1 | (clear_ ? 1u : 0u)); mix((uint64_t)aa_bits << 32 | ps_bits);
  mix(atlas_.epoch()); mix((uint64_t)(uint32_t)atlas_.size());
  mix((uint64_t)(env_.latency_routes ? 1u : 0u) << 8 | (uint64_t)(uint32_t)env_.cull_mode);
  J.damage_key = k;
}

// retained scenes: the host shadow (patch_runs) describes the block this frame goes into -- same device block, same layout
bool Context::shadow_usable(const LaunchJob& J) {
  if (!rec_diff_upload_) shadow_dev_ = nullptr;
  return rec_diff_upload_ && shadow_dev_ == d_frame_.ptr && shadow_layout_ == J.layout && shadow_.size() == J.layout.total;
}

// The weight tables depend on the filters alone and sit behind everything else in the block: when the device block already
// holds these very tables at these very offsets (an animation blurs with the same radii frame after frame) they are neither
// staged nor uploaded again -- 40 of the bench frame's 130 KB.
bool Context::tables_resident(const LaunchJob& J, bool shadow_ok) {
  std::vector<float>& sig = tables_sig_next_;
  sig.clear();
  for (size_t i = 0; i < J.blurs.size(); i++)
    if (J.layout.mx_h[i]) { const BlurTaps& t = J.blurs[i].taps; sig.push_back((float)t.reach); sig.insert(sig.end(), t.dense + kBlurPad, t.dense + kBlurPad + 2 * t.reach + 1); }
  return tables_dev_ == d_frame_.ptr && tables_layout_ == J.layout && tables_sig_ == sig && (!rec_diff_upload_ || shadow_ok);
}

// The slot's small print: chunk boxes, phase table, then the blur weight tables (when the device block does not hold them already).
// (built in ordinary memory -- the retained path compares and keeps it -- and copied to the slot's pinned buffer in one go)
void Context::build_misc(const LaunchJob& J, bool tables_resident) {
  const FrameLayout& F = J.layout;
  std::vector<uint8_t>& misc = misc_host_;
  const size_t o_misc = F.misc();
  misc.assign((tables_resident ? F.tables : F.total) - o_misc, 0);
  int* pf = reinterpret_cast<int*>(misc.data() + (F.phase_first - o_misc));
  for (size_t i = 0; i < J.phases.size(); i++) pf[i] = J.phases[i].first;
  pf[J.phases.size()] = (int)F.n;
  {  // chunk boxes: the union box of every 256 consecutive draws = byte-wise min of their bin boxes (x0, y0 min; 127 - x1, 127 - y1 min)
    uint32_t* cb = reinterpret_cast<uint32_t*>(misc.data());
    for (size_t c = 0; c < F.n_chunks; c++) cb[c] = 0x7f7f7f7fu;
    size_t g = 0;
    for (const Piece& p : frame_.pieces()) {
      const uint32_t* bx = frame_.lane(p.lane).boxes.p + p.first;
      for (uint32_t i = 0; i < p.n; i++, g++) {
        const uint32_t m = cb[g >> 8], v = bx[i];
        uint32_t o = 0;
        for (int sh = 0; sh < 32; sh += 8) o |= std::min((m >> sh) & 255u, (v >> sh) & 255u) << sh;
        cb[g >> 8] = o;
      }
    }
  }
  for (size_t i = 0; i < J.blurs.size() && !tables_resident; i++)
    if (F.mx_h[i]) {
      // the fragments depend on the filter alone: an animation blurs with the same radii frame after frame, and building
      // the four tables of the bench frame took 35 of the 54 us this function spent before its first launch
      const BlurTaps& t = J.blurs[i].taps;
      const size_t bh = mx_table_bytes(mx_nk(t.reach, false)), bv = mx_table_bytes(mx_nk(t.reach, true));
      const MxTables* hit = nullptr;
      for (const MxTables& c : mx_cache_)
        if (c.reach == t.reach && std::memcmp(c.dense.data(), t.dense + kBlurPad, sizeof(float) * (2 * t.reach + 1)) == 0) { hit = &c; break; }
      if (!hit) {
        if (mx_cache_.size() >= 8) mx_cache_.erase(mx_cache_.begin());
        MxTables c;
        c.reach = t.reach;
        c.dense.assign(t.dense + kBlurPad, t.dense + kBlurPad + 2 * t.reach + 1);
        c.h.resize(bh); c.v.resize(bv);
        const float dev_h = build_mx_weights(t, false, c.h.data());
        const float dev_v = build_mx_weights(t, true, c.v.data());
        c.keeps_opaque = std::max(dev_h, dev_v) <= kMxOpaqueSumBound;
        mx_cache_.push_back(std::move(c));
        hit = &mx_cache_.back();
      }
      if (!hit->keeps_opaque) throw Error(FDH_ERR_INVALID, "blur weights: the fragments' sum misses the scale (an opaque surface would not stay opaque)");
      std::memcpy(misc.data() + (F.mx_h[i] - o_misc), hit->h.data(), bh);
      std::memcpy(misc.data() + (F.mx_v[i] - o_misc), hit->v.data(), bv);
    }
  const int slot = J.staging_slot;
  HostVec<uint8_t>& up_misc = misc_[slot];
  up_misc.pinned = true;
  up_misc.vram = vram_staging(device_);
  up_misc.dev = device_;
  up_misc.n = 0;
  up_misc.reserve(misc.size());
  if (up_misc.p != misc_dev_host_[slot]) { misc_dev_[slot] = up_misc.device_view(); misc_dev_host_[slot] = up_misc.p; }
}

// Retained scenes: only what differs from the block the device already holds travels -- after an edit (or between two frames
// of an animation) that is a few hundred bytes of records and bin records out of ~110 KB.  The comparison runs against a
// host shadow of the device block in 256-byte chunks.  (A frame recorded from scratch differs from its predecessor nearly
// everywhere: comparing 110 KB to find that out, and keeping the shadow current, cost 12 us per frame -- only frames of a
// retained scene take the diff route.)  False: the frame does not qualify, or too much of it differs -- gather_runs takes it whole.
bool Context::patch_runs(LaunchJob& J, bool shadow_ok) {
  if (!shadow_ok || frame_.pieces().size() > 1 || (!frame_.pieces().empty() && frame_.pieces()[0].lane != 0)) return false;
  const Piece p0 = frame_.pieces().empty() ? Piece{} : frame_.pieces()[0];
  if (p0.ext_first != 0) return false;  // (one piece of lane 0 starting at extension 0: the records' extension indices are the frame's already)
  const FrameLayout& F = J.layout;
  const std::vector<uint8_t>& misc = misc_host_;
  HostVec<uint8_t>& up_misc = misc_[J.staging_slot];
  const size_t o_misc = F.misc(), b_recs = F.n * sizeof(DrawRec), b_ext = F.n_ext * sizeof(QuadExt), b_bb = F.n * sizeof(BinRec);
  Lane& L = frame_.lane(0);
  L.publish(0, 0, 0, 0);  // (the mirrors exist and fit the lane: their addresses are final, the device views may be taken)
  std::vector<UploadRun>& runs = J.runs;
  runs.clear();
  std::vector<const uint8_t*> from;  // the host bytes behind each run (the shadow is brought up to date from them)
  size_t dirty = 0;
  bool fits = true;
  auto diff = [&](const uint8_t* host, const uint8_t* dev_src, size_t off, size_t bytes, uint32_t kind) {
    for (size_t at = 0; at < bytes && fits; at += 256) {
      const size_t len = std::min<size_t>(256, bytes - at);
      if (std::memcmp(shadow_.data() + off + at, host + at, len) == 0) continue;
      dirty += len;
      if (!runs.empty() && runs.back().kind == kind && (size_t)runs.back().dst_off + runs.back().bytes == off + at) runs.back().bytes += (uint32_t)len;
      else if (runs.size() + 4 < (size_t)kMaxUploadRuns) { runs.push_back(UploadRun{dev_src + at, (uint32_t)(off + at), (uint32_t)len, 0u, kind}); from.push_back(host + at); }
      else fits = false;
    }
  };
  diff(reinterpret_cast<const uint8_t*>(L.recs.p + p0.first), L.d_recs + (size_t)p0.first * sizeof(DrawRec), F.recs, b_recs, 0u);
  diff(reinterpret_cast<const uint8_t*>(L.exts.p), L.d_exts, F.exts, b_ext, 0u);
  diff(reinterpret_cast<const uint8_t*>(L.bins.p + p0.first), L.d_bins + (size_t)p0.first * sizeof(BinRec), F.binrecs, b_bb, 1u);
  diff(misc.data(), misc_dev_[J.staging_slot], o_misc, F.tables - o_misc, 0u);
  if (!fits || dirty * 2 >= F.total) return false;
  for (size_t k = 0; k < runs.size(); k++) {
    std::memcpy(shadow_.data() + runs[k].dst_off, from[k], runs[k].bytes);
    // what travels is published now: the dirty chunks alone
    const size_t off = runs[k].dst_off;
    if (off >= o_misc) std::memcpy(up_misc.p + (off - o_misc), misc.data() + (off - o_misc), runs[k].bytes);
    else if (off >= F.binrecs) L.publish_bytes(1, (size_t)p0.first * sizeof(BinRec) + (off - F.binrecs), runs[k].bytes);
    else if (off >= F.exts && b_ext) L.publish_bytes(2, off - F.exts, runs[k].bytes);
    else L.publish_bytes(0, (size_t)p0.first * sizeof(DrawRec) + (off - F.recs), runs[k].bytes);
  }
  uploaded_bytes_ = (int64_t)dirty;
  return true;
}

// The runs k_upload_frame gathers.  Every piece brings three: its records (extension indices re-based on the way), its bin
// records, its extensions; then the phase table (+ tables).  A frame recorded by one thread is one piece.  A lane's device views
// (taken by whoever allocated its mirrors) are read after the piece was published: the mirrors are then where they will stay.
void Context::gather_runs(LaunchJob& J, bool tables_resident) {
  const FrameLayout& F = J.layout;
  const std::vector<uint8_t>& misc = misc_host_;
  J.runs.clear();
  auto add_run = [&J](const uint8_t* src, size_t dst_off, size_t bytes, uint32_t ext_add, uint32_t kind) {
    if (!bytes) return;
    J.runs.push_back(UploadRun{src, (uint32_t)dst_off, (uint32_t)bytes, ext_add, kind});
  };
  uint32_t at_rec = 0, at_ext = 0;
  std::memcpy(misc_[J.staging_slot].p, misc.data(), misc.size());
  for (const Piece& p : frame_.pieces()) {
    // pieces the calling thread recorded are published here (clips open around a sibling group took the group's bounds after
    // their records were made); a pool thread published its pieces when it finished them
    Lane& L = frame_.lane(p.lane);
    if (p.lane <= 0) { HostTimer t(host_ns_[5]); L.publish(p.first, p.n, p.ext_first, p.n_ext); }
    add_run(L.d_recs + (size_t)p.first * sizeof(DrawRec), F.recs + (size_t)at_rec * sizeof(DrawRec), (size_t)p.n * sizeof(DrawRec), at_ext - p.ext_first, 2u);
    add_run(L.d_bins + (size_t)p.first * sizeof(BinRec), F.binrecs + (size_t)at_rec * sizeof(BinRec), (size_t)p.n * sizeof(BinRec), 0u, 1u);
    if (p.n_ext) add_run(L.d_exts + (size_t)p.ext_first * sizeof(QuadExt), F.exts + (size_t)at_ext * sizeof(QuadExt), (size_t)p.n_ext * sizeof(QuadExt), 0u, 0u);
    at_rec += p.n; at_ext += p.n_ext;
  }
  add_run(misc_dev_[J.staging_slot], F.misc(), misc.size(), 0u, 0u);
  int64_t link_bytes = 0;
  for (const UploadRun& r : J.runs) link_bytes += r.bytes;
  uploaded_bytes_ = link_bytes;
  if (!rec_diff_upload_) return;
  // take the shadow this frame's successors are compared with
  if (shadow_.size() != F.total) shadow_.assign(F.total, 0);
  else if (!tables_resident) std::fill(shadow_.begin(), shadow_.end(), 0);
  size_t ar = 0, ae = 0;
  for (const Piece& p : frame_.pieces()) {
    const Lane& L = frame_.lane(p.lane);
    std::memcpy(shadow_.data() + F.recs + ar * sizeof(DrawRec), L.recs.p + p.first, (size_t)p.n * sizeof(DrawRec));
    if (p.ext_first != ae)  // (the device's copy holds frame-relative extension indices)
      for (size_t i = 0; i < p.n; i++) { DrawRec* r = reinterpret_cast<DrawRec*>(shadow_.data() + F.recs) + ar + i; if (r->op_mode & F_GENERAL) r->ext += (uint32_t)ae - p.ext_first; }
    std::memcpy(shadow_.data() + F.binrecs + ar * sizeof(BinRec), L.bins.p + p.first, (size_t)p.n * sizeof(BinRec));
    if (p.n_ext) std::memcpy(shadow_.data() + F.exts + ae * sizeof(QuadExt), L.exts.p + p.ext_first, (size_t)p.n_ext * sizeof(QuadExt));
    ar += p.n; ae += p.n_ext;
  }
  std::memcpy(shadow_.data() + F.misc(), misc.data(), misc.size());
  shadow_layout_ = F;
  shadow_dev_ = d_frame_.ptr;
}

// algorithmic bytes of this frame: final store + per blur (pre-blur store is the store above for
// a full-frame node; H read + H write + V read + V write + composite read) + records once
void Context::account_frame(LaunchJob& J) {
  const size_t n = J.layout.n;
  int64_t bytes = 4LL * env_.W * env_.H + (int64_t)n * (int64_t)sizeof(DrawRec), bytes_blur = 0, bytes_fused = 0, bytes_saved = 0;
  // a cleared opaque surface stays opaque under SRC_ALPHA / ONE_MINUS_SRC_ALPHA blending (a' = sa + da (1 - sa), da = 1): a
  // fused vertical pass then replaces pixels under full coverage without reading them
  const bool surface_opaque = clear_ && (clear_rgba8_ >> 24) == 255u;
  J.big_blur = -1;
  int64_t big_area = 0;
  stats_.bytes_blur_big_h = stats_.bytes_blur_big_v = 0;
  for (size_t bi = 0; bi < J.blurs.size(); bi++) {
    const BlurJob& j = J.blurs[bi];
    const int ylo = std::max(0, j.y0 - j.taps.reach), yhi = std::min(env_.H, j.y1 + j.taps.reach);
    const int64_t a_h = (int64_t)(j.x1 - j.x0) * (yhi - ylo), a_v = (int64_t)(j.x1 - j.x0) * (j.y1 - j.y0);
    int64_t b_h = 4 * a_h + 4 * a_h, b_v = 4 * a_h + 4 * a_v;  // H read + H write; V read + V write
    // the consuming composite: fused into the V pass it reads the live surface there (where it has to blend); otherwise a
    // composite launch reads the blurred snapshot
    if (j.fuse_draw >= 0) { if (!surface_opaque) b_v += 4 * a_v; } else bytes += 4 * a_v;
    bytes_blur += b_h + b_v;
    if (bi < J.blur_fused.size() && J.blur_fused[bi]) {  // one kernel: the region read once (+ the surface under a translucent composite), written once
      const int64_t b_fx = 4 * a_v + 4 * a_v;
      bytes_fused += b_fx;
      bytes_saved += b_h + b_v - b_fx;
    }
    if (a_v > big_area) { big_area = a_v; J.big_blur = (int)bi; stats_.bytes_blur_big_h = b_h; stats_.bytes_blur_big_v = b_v; }
  }
  bytes += bytes_blur;
  stats_.bytes_blur = bytes_blur;
  stats_.bytes_composite_main = 4LL * env_.W * env_.H * (clear_ ? 1 : 2) + (int64_t)J.phases[0].count * (int64_t)sizeof(DrawRec);
  // algorithmic flops of the phase-0 composite launch, SURVEY.md 8(d): per fragment ClipAA 25, DropShadow 35 + exp, InsetShadow
  // 70 + exp, AnnularAA 28 (other modes priced as ClipAA), elliptical corners + 30, blend + re-quantise + 16
  for (int k = 0; k < 4; k++) stats_.fragments_main_by_mode[k] = frame_.frag_mode()[k];
  stats_.fragments_main_elliptical = frame_.frag_ellip();
  stats_.fragments_main_other = frame_.frag_other();
  stats_.flops_composite_main = frame_.frag_mode()[0] * 25 + frame_.frag_mode()[1] * 36 + frame_.frag_mode()[2] * 71 + frame_.frag_mode()[3] * 28 + frame_.frag_other() * 25 + frame_.frag_ellip() * 30 +
                                (frame_.frag_mode()[0] + frame_.frag_mode()[1] + frame_.frag_mode()[2] + frame_.frag_mode()[3] + frame_.frag_other()) * 16;
  stats_.n_draws = (int32_t)n;
  stats_.n_phases = (int32_t)J.phases.size();
  stats_.n_blurs = (int32_t)J.blurs.size();
  stats_.n_bins = J.bins_x * J.bins_y;
  stats_.bytes_algorithmic = bytes;
  stats_.bytes_blur_fused = bytes_fused;
  stats_.bytes_frame_implementation = bytes - bytes_saved;
  stats_.fragments = fragments_;
}

// what the calling thread and the pool's threads wrote into device memory is on its way before the launches are
void Context::fence_staging() {
  if (!vram_staging(device_)) return;
  store_fence();
  // ... and pushed out of the host data path: without this, frames of fresh contexts on several host threads came out wrong -- or
  // faulted -- in ~5 % of tools/thread_churn.py runs (end of round 4).  (A device register every context of the device writes 1 to,
  // from whichever host thread renders it: an atomic store, so that the language knows too.)
  if (hdp_flush_reg_) { __atomic_store_n(hdp_flush_reg_, 1u, __ATOMIC_RELAXED); store_fence(); }
}

// Which blur routes a frame takes is a matter of speed only (same pixels either way): the one-kernel routes -- k_blur_fx for a node
// that covers the frame, k_blur_small for a small one: fewer dependent launches, half the bytes -- or the two passes as two
// kernels.  Rounds 3 and early 4 chose per frame: one-kernel routes for a frame rendered alone, two-pass routes when another
// context of the process had submitted a frame within the last millisecond, where they measured 3 - 4 % faster (135 against 141
// Gpixel/s with four contexts).  With the last bubbles out of the launch chain (no event behind the upload, bin workgroups per
// phase box) that has turned: one-kernel routes 150.0 - 150.6 Gpixel/s against 145.1 - 147.3 with four contexts (tools/ab_routes.sh,
// three alternations on one box), and 84 against 94 us one frame at a time.  So: the one-kernel routes, always
// (fdh_set_blur_route / FDH_BLUR_FUSED = 0: the two-pass routes).
void Context::pick_routes() {
  static const int fx_env = [] { const char* e = std::getenv("FDH_BLUR_FUSED"); return e ? (std::atoi(e) != 0 ? 1 : 0) : -1; }();
  const int route = blur_route_ >= 0 ? blur_route_ : fx_env;
  frame_env_.latency_routes = route != 0;
}

// More pieces than the upload's run table holds (a frame with many parallel sibling groups): they are copied together into one
// spare lane, in order, extension indices re-based -- the frame becomes one piece again.
void Context::consolidate_pieces() {
  Lane& S = frame_.merge_lane();
  S.recs.reserve(frame_.n_records()); S.bins.reserve(frame_.n_records()); S.exts.reserve(frame_.n_extensions());
  for (const Piece& p : frame_.pieces()) {
    const Lane& L = frame_.lane(p.lane);
    const size_t r0 = S.recs.n, e0 = S.exts.n;
    S.recs.append(L.recs.p + p.first, p.n);
    S.bins.append(L.bins.p + p.first, p.n);
    S.exts.append(L.exts.p + p.ext_first, p.n_ext);
    S.boxes.append(L.boxes.p + p.first, p.n);
    if (env_.pick_frame) S.tags.append(L.tags.p + p.first, p.n);
    for (size_t i = r0; i < S.recs.n; i++) if (S.recs[i].op_mode & F_GENERAL) S.recs[i].ext += (uint32_t)e0 - p.ext_first;
  }
  Piece all;
  all.lane = -1; all.first = 0; all.n = frame_.n_records(); all.ext_first = 0; all.n_ext = frame_.n_extensions();
  frame_.replace_pieces(all);
}

}  // namespace fdh
