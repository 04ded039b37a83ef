// fdh_frame.cpp -- the recorded frame: what a lane publishes and counts, and the bookkeeping of pieces and phases (RecordedFrame).
#include <algorithm>
#include <cstring>

#include "fdh_frame.h"

namespace fdh {

// ------------------------------------------------------------------ publishing (Lane)
// The mirrors grow with the lane (never shrink, never hold more than the lane); a mirror that had to move is filled again from the
// lane up to what had been published -- from ordinary memory: pinned memory is not read.
static void mirror_fit(Lane& L) {
  auto fit = [](auto& up, const auto& src, size_t published, const uint8_t*& dev) {
    if (up.cap >= src.cap) return;
    up.n = 0;  // (nothing to carry over: reserve() would READ the old pinned block)
    up.reserve(src.cap);
    if (published) std::memcpy(static_cast<void*>(up.p), static_cast<const void*>(src.p), published * sizeof(*src.p));
    dev = up.device_view();
  };
  fit(L.up_recs, L.recs, L.pub_recs, L.d_recs);
  fit(L.up_bins, L.bins, L.pub_recs, L.d_bins);
  fit(L.up_exts, L.exts, L.pub_exts, L.d_exts);
}
void Lane::publish(uint32_t first, uint32_t n, uint32_t ext_first, uint32_t n_ext) {
  if (!device) return;
  mirror_fit(*this);
  if (n) {
    std::memcpy(static_cast<void*>(up_recs.p + first), static_cast<const void*>(recs.p + first), (size_t)n * sizeof(DrawRec));
    std::memcpy(static_cast<void*>(up_bins.p + first), static_cast<const void*>(bins.p + first), (size_t)n * sizeof(BinRec));
    pub_recs = std::max(pub_recs, (size_t)first + n);
  }
  if (n_ext) {
    std::memcpy(static_cast<void*>(up_exts.p + ext_first), static_cast<const void*>(exts.p + ext_first), (size_t)n_ext * sizeof(QuadExt));
    pub_exts = std::max(pub_exts, (size_t)ext_first + n_ext);
  }
  if (up_recs.vram) store_fence();  // (write-combined stores into device memory: drained before this thread says the piece is there)
}
void Lane::publish_bytes(int array, size_t at, size_t len) {
  if (!device || !len) return;
  mirror_fit(*this);
  uint8_t* dst = array == 0 ? reinterpret_cast<uint8_t*>(up_recs.p) : array == 1 ? reinterpret_cast<uint8_t*>(up_bins.p) : reinterpret_cast<uint8_t*>(up_exts.p);
  const uint8_t* src = array == 0 ? reinterpret_cast<const uint8_t*>(recs.p) : array == 1 ? reinterpret_cast<const uint8_t*>(bins.p) : reinterpret_cast<const uint8_t*>(exts.p);
  std::memcpy(dst + at, src + at, len);
  if (up_recs.vram) store_fence();
}

// ------------------------------------------------------------------ list stride (Lane)
void Lane::count_begin(int bins_x, int bins_y) {
  if (dw != bins_x + 1 || dh != bins_y + 1) {
    dw = bins_x + 1; dh = bins_y + 1;
    diff.assign((size_t)dw * dh, 0);
  } else if (touched) {
    for (int y = ty0; y <= ty1; y++) std::fill(diff.begin() + (size_t)y * dw + tx0, diff.begin() + (size_t)y * dw + tx1 + 1, 0);
  }
  touched = false;
}
// The largest number of records any bin received since the last close, counted exactly from the 2-D difference array
// (O(records + bins reached)): sizing the lists for "every draw of the phase in every bin" cost 163 MB for the 10 001-draw glyph
// frame; the exact bound is 2040 bins x a few dozen entries.
int Lane::count_close() {
  if (!touched) return 0;
  int mx = 0;
  for (int y = ty0; y < ty1; y++) {
    int run = 0;
    int* row = diff.data() + (size_t)y * dw;
    const int* above = y > ty0 ? row - dw : nullptr;
    for (int x = tx0; x < tx1; x++) {
      run += row[x];
      const int cell = run + (above ? above[x] : 0);  // column prefix over the row prefixes
      row[x] = cell;
      mx = std::max(mx, cell);
    }
  }
  for (int y = ty0; y <= ty1; y++) std::fill(diff.begin() + (size_t)y * dw + tx0, diff.begin() + (size_t)y * dw + tx1 + 1, 0);
  touched = false;
  return mx;
}

// ------------------------------------------------------------------ the frame: pieces and phases (calling thread)
Lane& RecordedFrame::ensure_lane(int i) {
  auto& v = lanes_[(size_t)set_];
  while ((int)v.size() <= i) {
    v.emplace_back(new Lane());
    v.back()->set_pinned(!host_only_, device_);
  }
  return *v[(size_t)i];
}
Lane& RecordedFrame::begin(int w, int h) {
  set_ = next_set();
  frame_no_++;
  bins_x_ = (w + kBin - 1) / kBin; bins_y_ = (h + kBin - 1) / kBin;
  Lane& L0 = ensure_lane(0);
  L0.clear();
  L0.count_begin(bins_x_, bins_y_);
  pieces_.clear();
  n_total_ = n_ext_total_ = 0;
  piece_open_ = false;
  phases_.clear();
  phases_.push_back(Phase{});
  blurs_.clear();
  phase_u_ = BBox{0, 0, 0, 0};
  stride_max_ = 1;
  phase_extra_ = 0;
  deepest_clip_ = 0;
  for (auto& f : frag_mode_) f = 0;
  frag_ellip_ = frag_other_ = 0;
  open_piece();
  return L0;
}
void RecordedFrame::pool_slots(int slots) {
  for (int s = 0; s < slots; s++) {
    Lane& Ln = ensure_lane(s + 1);
    if (Ln.stamp != frame_no_) {  // first use in this frame
      Ln.clear();
      Ln.count_begin(bins_x_, bins_y_);
      Ln.stamp = frame_no_;
    }
  }
}
void RecordedFrame::rewind_lane(int i, size_t recs, size_t exts) {
  Lane& Ln = lane(i);
  Ln.recs.n = Ln.bins.n = Ln.boxes.n = recs; Ln.exts.n = exts;
  if (Ln.tags.n > recs) Ln.tags.n = recs;  // (picking frames)
}
Lane& RecordedFrame::merge_lane() {
  std::unique_ptr<Lane>& slot = merge_lane_[(size_t)set_];
  if (!slot) { slot.reset(new Lane()); slot->set_pinned(!host_only_, device_); }
  slot->clear();
  return *slot;
}
uint32_t RecordedFrame::global_count() const { return piece_open_ ? (uint32_t)lane(0).recs.n + g0_delta_ : n_total_; }
uint32_t RecordedFrame::open_piece() {
  const Lane& L = lane(0);
  Piece p;
  p.lane = 0; p.first = (uint32_t)L.recs.n; p.ext_first = (uint32_t)L.exts.n;
  pieces_.push_back(p);
  piece_open_ = true;
  g0_delta_ = n_total_ - p.first;
  return p.first;  // (LE_SHARE looks one record back in the lane: never across a piece boundary)
}
void RecordedFrame::close_piece() {
  if (!piece_open_) return;
  const Lane& L = lane(0);
  Piece& p = pieces_.back();
  p.n = (uint32_t)L.recs.n - p.first;
  p.n_ext = (uint32_t)L.exts.n - p.ext_first;
  n_total_ += p.n;
  n_ext_total_ += p.n_ext;
  piece_open_ = false;
  if (p.n == 0) pieces_.pop_back();
}
void RecordedFrame::add_sum(const PhaseSum& s, int depth_base) {
  phases_.back().merge_flags(s);
  bbox_union(phase_u_, s.u);
  deepest_clip_ = std::max(deepest_clip_, depth_base + s.deepest);
  if (phases_.size() == 1) {  // the phase-0 composite launch's work units
    for (int k = 0; k < 4; k++) frag_mode_[k] += s.frag_mode[k];
    frag_ellip_ += s.frag_ellip;
    frag_other_ += s.frag_other;
  }
}
void RecordedFrame::add_piece(const Piece& p) {
  if (!p.n) return;
  pieces_.push_back(p);
  n_total_ += p.n;
  n_ext_total_ += p.n_ext;
}
// the phase ends here (a blur node, or the frame's end): its summary and its share of the list stride
void RecordedFrame::close_phase(const PhaseSum& rest) {
  add_sum(rest, 0);
  Phase& ph = phases_.back();
  constexpr int kBinShift = 6;
  const BBox u = phase_u_;
  ph.bin_x0 = u.x0 >> kBinShift; ph.bin_y0 = u.y0 >> kBinShift;
  ph.bin_x1 = bbox_empty(u) ? ph.bin_x0 : (u.x1 + kBin - 1) >> kBinShift;
  ph.bin_y1 = bbox_empty(u) ? ph.bin_y0 : (u.y1 + kBin - 1) >> kBinShift;
  phase_u_ = BBox{0, 0, 0, 0};
  stride_max_ = std::max(stride_max_, lane(0).count_close() + phase_extra_);
  phase_extra_ = 0;
  ph.count = (int)(global_count() - (uint32_t)ph.first);
}
void RecordedFrame::split_phase(const PhaseSum& rest, int blur) {
  close_phase(rest);
  Phase next;
  next.first = (int)global_count();
  next.blur = blur;
  phases_.push_back(next);
}

}  // namespace fdh
