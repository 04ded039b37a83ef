// fdh_pick.cpp -- picking: the host side of the pick launches over the frame block the last frame left on the device.
#include "fdh_context.h"
#include "fdh_host.h"
#include "fdh_pick.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace fdh {

// ------------------------------------------------------------------ picking (include/figdraw_hip_pick.h, k_pick.hip)
void Context::pick_check(const char* who, int threshold, uint32_t flags) {
  need_device(who);
  drain();
  if (!have_frame_ || !job_.pick) throw Error(FDH_ERR_INVALID, std::string(who) + ": the last frame was rendered with picking off (fdh_set_pick)");
  if (threshold < 1 || threshold > 255) throw Error(FDH_ERR_INVALID, std::string(who) + ": threshold must be in 1..255");
  if (flags & ~(uint32_t)FDH_PICK_SHADOWS) throw Error(FDH_ERR_INVALID, std::string(who) + ": unknown flags");
  FDH_HIP(hipSetDevice(device_));
}
// what a pick launch reads of the last frame (the frame block it left on the device; the launch follows the frame on the stream)
static PickParams pick_params(const LaunchJob& J, const AtlasView& atlas, int threshold, uint32_t flags) {
  PickParams P{};
  P.draws = J.dv.recs; P.exts = J.dv.exts; P.phase_first = J.dv.phase_first;
  P.n_phases = (int)J.phases.size(); P.n_recs = J.n_recs;
  P.atlas = atlas;
  P.W = J.W; P.H = J.H;
  P.threshold = threshold; P.flags = flags;
  return P;
}
void Context::pick_points(const float* xy, int n, int threshold, uint32_t flags, int max_hits, FdhPickHit* out, int* counts) {
  if (n < 0 || (n > 0 && (!xy || !out || !counts))) throw Error(FDH_ERR_INVALID, "fdh_pick_points: bad point array");
  if (max_hits < 1 || max_hits > FDH_PICK_MAX_HITS) throw Error(FDH_ERR_INVALID, "fdh_pick_points: max_hits must be in 1..16");
  pick_check("fdh_pick_points", threshold, flags);
  const LaunchJob& J = job_;
  const bool striped = stripe_y1_ > stripe_y0_;
  // the points inside the frame, by 16 x 16 tile (a tile's points in runs of at most 256: one workgroup each)
  struct Q { int64_t key; int i, x, y; };
  std::vector<Q> q;
  q.reserve((size_t)n);
  const int tiles_x = (J.W + kPickTile - 1) / kPickTile;
  for (int i = 0; i < n; i++) {
    counts[i] = 0;
    const float fx = xy[2 * i], fy = xy[2 * i + 1];
    if (!(fx >= 0.0f && fy >= 0.0f && fx < (float)J.W && fy < (float)J.H)) continue;  // (a NaN is outside too)
    const int x = std::min((int)std::floor(fx), J.W - 1), y = std::min((int)std::floor(fy), J.H - 1);
    if (striped && (y < stripe_y0_ || y >= stripe_y1_)) throw Error(FDH_ERR_INVALID, "fdh_pick_points: a point's row lies outside this context's stripe");
    q.push_back(Q{(int64_t)(y / kPickTile) * tiles_x + x / kPickTile, i, x, y});
  }
  if (q.empty()) return;
  std::stable_sort(q.begin(), q.end(), [](const Q& a, const Q& b) { return a.key < b.key; });
  const size_t m = q.size();
  std::vector<int> first;
  std::vector<int2> txy;
  for (size_t k = 0; k < m; k++)
    if (k == 0 || q[k].key != q[k - 1].key || (int)k - first.back() >= kPickThreads) {
      first.push_back((int)k);
      txy.push_back(make_int2((int)(q[k].key % tiles_x) * kPickTile, (int)(q[k].key / tiles_x) * kPickTile));
    }
  const int groups = (int)first.size();
  first.push_back((int)m);
  // one device block: points | tile_first | tile_xy | hits | hit counts (inputs staged through pinned memory, outputs read back into it)
  const size_t o_pts = 0, o_first = align256(m * sizeof(int2)), o_xy = align256(o_first + first.size() * sizeof(int)), o_in_end = o_xy + (size_t)groups * sizeof(int2);
  const size_t o_hits = align256(o_in_end), o_cnt = align256(o_hits + m * (size_t)max_hits * sizeof(uint2)), total = o_cnt + m * sizeof(int);
  reserve_quiet(d_pick_, total);
  h_pick_.reserve(total);
  uint8_t* h = h_pick_.ptr;
  for (size_t k = 0; k < m; k++) reinterpret_cast<int2*>(h + o_pts)[k] = make_int2(q[k].x, q[k].y);
  std::memcpy(h + o_first, first.data(), first.size() * sizeof(int));
  std::memcpy(h + o_xy, txy.data(), txy.size() * sizeof(int2));
  const int levels = std::max(J.pick_depth - kPickDepth, 0);
  if (levels) reserve_quiet(d_pick_spill_, (size_t)levels * groups * kPickThreads);
  PickParams P = pick_params(J, atlas_.view(), threshold, flags);
  uint8_t* d = d_pick_.ptr;
  P.pts = reinterpret_cast<const int2*>(d + o_pts); P.tile_first = reinterpret_cast<const int*>(d + o_first); P.tile_xy = reinterpret_cast<const int2*>(d + o_xy);
  P.max_hits = max_hits;
  P.hits = reinterpret_cast<uint2*>(d + o_hits); P.hit_count = reinterpret_cast<int*>(d + o_cnt);
  P.spill = levels ? d_pick_spill_.ptr : nullptr;
  FDH_HIP(hipMemcpyAsync(d, h, o_in_end, hipMemcpyHostToDevice, stream_));
  launch_pick(stream_, P, groups, levels);
  FDH_HIP(hipGetLastError());
  FDH_HIP(hipMemcpyAsync(h + o_hits, d + o_hits, total - o_hits, hipMemcpyDeviceToHost, stream_));
  FDH_HIP(hipStreamSynchronize(stream_));
  // the rings (painter's order) -> front to back, with the frame's tags
  const uint2* hits = reinterpret_cast<const uint2*>(h + o_hits);
  const int* cnt = reinterpret_cast<const int*>(h + o_cnt);
  for (size_t k = 0; k < m; k++) {
    const int c = cnt[k], kept = std::min(c, max_hits), i = q[k].i;
    FdhPickHit* o = out + (size_t)i * max_hits;
    for (int j = 0; j < kept; j++) {
      const uint2 e = hits[k * max_hits + (size_t)((c - 1 - j) % max_hits)];
      const PickTag g = e.x < J.pick_tags.size() ? J.pick_tags[e.x] : PickTag{-1, -1};
      o[j] = FdhPickHit{g.z, g.id, (int32_t)e.x, (uint8_t)(e.y & 255u), (uint8_t)((e.y >> 8) & 255u), 0};
    }
    counts[i] = kept;
  }
}
void Context::pick_region(int x, int y, int w, int h, int threshold, uint32_t flags, int32_t* out_draw) {
  if (w < 0 || h < 0 || ((int64_t)w * h > 0 && !out_draw)) throw Error(FDH_ERR_INVALID, "fdh_pick_region: bad rectangle");
  if ((int64_t)w * h > ((int64_t)1 << 28)) throw Error(FDH_ERR_INVALID, "fdh_pick_region: rectangle too large");
  pick_check("fdh_pick_region", threshold, flags);
  if (w == 0 || h == 0) return;
  const LaunchJob& J = job_;
  if (stripe_y1_ > stripe_y0_) {  // the rows of the rectangle inside the frame must lie in the stripe
    const int r0 = std::max(y, 0), r1 = std::min(y + h, J.H);
    if (r1 > r0 && (r0 < stripe_y0_ || r1 > stripe_y1_)) throw Error(FDH_ERR_INVALID, "fdh_pick_region: rows outside this context's stripe");
  }
  const int tiles_x = (w + kPickTile - 1) / kPickTile, tiles_y = (h + kPickTile - 1) / kPickTile, groups = tiles_x * tiles_y;
  reserve_quiet(d_pick_, (size_t)w * h * sizeof(int32_t));
  const int levels = std::max(J.pick_depth - kPickDepth, 0);
  if (levels) reserve_quiet(d_pick_spill_, (size_t)levels * groups * kPickThreads);
  PickParams P = pick_params(J, atlas_.view(), threshold, flags);
  P.x0 = x; P.y0 = y; P.w = w; P.h = h; P.tiles_x = tiles_x;
  P.region_out = reinterpret_cast<int32_t*>(d_pick_.ptr);
  P.spill = levels ? d_pick_spill_.ptr : nullptr;
  launch_pick(stream_, P, groups, levels);
  FDH_HIP(hipGetLastError());
  FDH_HIP(hipMemcpyAsync(out_draw, d_pick_.ptr, (size_t)w * h * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
  FDH_HIP(hipStreamSynchronize(stream_));
}
void Context::pick_draw_tags(int32_t* zlevels, int32_t* ids, int cap, int* n) {
  if (!n || cap < 0 || (cap > 0 && (!zlevels || !ids))) throw Error(FDH_ERR_INVALID, "fdh_pick_draw_tags: bad arrays");
  drain();
  const LaunchJob& J = job_;
  if (!J.pick) throw Error(FDH_ERR_INVALID, "fdh_pick_draw_tags: the last frame was rendered with picking off (fdh_set_pick)");
  *n = (int)J.pick_tags.size();
  const size_t k = std::min(J.pick_tags.size(), (size_t)cap);
  for (size_t i = 0; i < k; i++) { zlevels[i] = J.pick_tags[i].z; ids[i] = J.pick_tags[i].id; }
}

}  // namespace fdh
