// fdh_damage.cpp -- damage tracking, damage readback, coded and exact damage readback on the host: the two components a device context holds
// (DamageTracker, DamageReadback: fdh_damage_host.h) -- every launch of k_damage.hip, k_damage_codec.hip, k_damage_filter.hip and k_damage_move.hip, the
// pending set, the page-locked buffers a read returns, exact mode's mirror -- and the host-only functions behind fdh_damage_closure, fdh_apply_damage, fdh_decode_damage and
// fdh_coded_damage_bound.  What belongs to the context of an entry point (its refusals, the wait for the last frame) is fdh_context.cpp's.
#include "fdh_context.h"
#include "fdh_damage.h"
#include "fdh_host.h"
#include "fdh_tile_decode.h"  // decode_tiles, tile_in_image

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace fdh {

// ------------------------------------------------------------------ damage tracking (include/figdraw_hip_damage.h)
// the signatures a tracked frame leaves describe it whole only when every one of its blur nodes was folded in (more nodes than
// kDamageMaxNodes: the frame is rendered in full, and so is the next)
static bool damage_sig_whole(const LaunchJob& J) { return J.blurs.size() <= (size_t)kDamageMaxNodes; }

// The bins whose signatures changed since the context's last tracked frame, closed under the blur rule (fdh_damage.h), as a compact list
// the compositor launches walk.  A frame whose key differs from that frame's is rendered in full (its signatures are still taken: the
// next frame compares against them).
bool DamageTracker::launch(hipStream_t s, const LaunchJob& J, const BinParams& B, DamageReadback& rb, const LaunchSpan& span) {
  const int nb = J.bins_x * J.bins_y, np = (int)J.phases.size();
  const bool tracked = J.damage && nb > 0 && np > 0;
  // whatever this launch renders, the signatures and the surface stop matching until a tracked frame has been launched whole: a frame
  // rendered without tracking leaves its pixels, not the signatures' frame, in the surface
  const bool was_valid = valid;
  valid = false;
  if (!tracked) {
    last = false;
    rb.frame_whole();
    return false;
  }
  const bool full = J.damage_force || !damage_sig_whole(J) || !was_valid || key != J.damage_key;
  const bool keeps = !full && [&] { for (const BlurJob& j : J.blurs) if (j.fuse_draw >= 0) return true; return false; }();
  if (sig.cap < (size_t)nb || count.cap == 0 || (keeps && keep.cap < (size_t)J.W * J.H)) {
    FDH_HIP(hipStreamSynchronize(s));  // (a buffer that grows is freed: nothing in flight may still use it)
    sig.reserve(nb); changed.reserve(nb); mask.reserve(nb); list.reserve(nb);
    count.reserve(1); run.reserve(kDamageMaxNodes);
    if (keeps) keep.reserve((size_t)J.W * J.H);
  }
  DamageSignParams S;
  S.lists = J.lists; S.counts = J.counts; S.draws = J.dv.recs; S.exts = J.dv.exts; S.sig = sig.ptr; S.changed = changed.ptr;
  S.n_phases = np; S.bins_x = J.bins_x; S.bins_y = J.bins_y; S.stride = J.list_stride; S.n_draws = J.n_recs; S.n_exts = J.n_exts;
  S.force = full ? 1 : 0;
  S.sub_n = B.sub_n;
  for (int p = 0; p < kDamageMaxPhases; p++) {
    const bool in = p < B.sub_n;
    S.sub_x0[p] = in ? B.sub_x0[p] : 0; S.sub_y0[p] = in ? B.sub_y0[p] : 0; S.sub_nx[p] = in ? B.sub_nx[p] : 0;
    S.sub_ny[p] = in ? (B.sub_first[p + 1] - B.sub_first[p]) / std::max(1, B.sub_nx[p]) : 0;
  }
  DamageResolveParams R;
  R.changed = changed.ptr; R.mask = mask.ptr; R.list = list.ptr; R.count = count.ptr; R.run = run.ptr;
  R.bins_x = J.bins_x; R.bins_y = J.bins_y;
  S.n_nodes = R.n_nodes = std::min((int)J.blurs.size(), kDamageMaxNodes);  // (more: a full frame, every bin changed)
  for (int i = 0; i < S.n_nodes; i++) {
    const BlurJob& j = J.blurs[(size_t)i];
    int phase = -1;
    for (int p = 0; p < np; p++) if (J.phases[p].blur == i) phase = p;
    uint32_t rbits = 0;
    std::memcpy(&rbits, &j.radius, 4);
    uint64_t k = 1469598103934665603ull;
    for (uint32_t v : {(uint32_t)phase, (uint32_t)j.x0, (uint32_t)j.y0, (uint32_t)j.x1, (uint32_t)j.y1, rbits, (uint32_t)j.taps.reach, (uint32_t)(j.fuse_draw >= 0)})
      for (int b = 0; b < 4; b++) { k ^= (v >> (8 * b)) & 255u; k *= 1099511628211ull; }
    S.foot[i] = damage_region(j.x0, j.y0, j.x1, j.y1, 0, J.bins_x, J.bins_y);
    S.node_key[i] = k;
    R.reg[i] = damage_region(j.x0, j.y0, j.x1, j.y1, j.taps.reach, J.bins_x, J.bins_y);
  }
  span(true); launch_damage_sign(s, S); span(false);
  span(true); launch_damage_resolve(s, R); span(false);
  rb.accumulate(s, J, mask.ptr, span);
  bins_x = J.bins_x; bins_y = J.bins_y;
  last = true;
  return !full;
}
void DamageTracker::launched_whole(const LaunchJob& J) {
  if (last && damage_sig_whole(J)) { valid = true; key = J.damage_key; }
}
// a partial frame: a V pass that composites its quad into the surface runs whether the node took damage or not -- when it did not,
// its footprint is kept aside and put back (k_damage_guard: both return at once when the node's run flag is set)
void DamageTracker::guard(hipStream_t s, const LaunchJob& J, int node, bool restore, uint32_t* surf, int y0, int y1) const {
  const BlurJob& j = J.blurs[(size_t)node];
  launch_damage_guard(s, run.ptr, node, restore, surf, keep.ptr, J.W, j.x0, y0, j.x1, y1);
}
void DamageTracker::composite(hipStream_t s, const LaunchJob& J, const CompositeParams& C) const {
  launch_composite_damage(s, J.dv.recs, J.dv.exts, C, list.ptr, count.ptr, J.bins_x * J.bins_y * 16);  // (a wave per strip)
}
std::vector<uint8_t> DamageTracker::bins(int gx, int gy, bool changed_only) const {
  const int nb = gx * gy;
  std::vector<uint8_t> m((size_t)nb, 1);  // a frame rendered without tracking: every bin
  if (last && bins_x == gx && bins_y == gy && nb > 0)
    FDH_HIP(hipMemcpy(m.data(), changed_only ? changed.ptr : mask.ptr, (size_t)nb, hipMemcpyDeviceToHost));
  return m;
}
void DamageTracker::release() {
  sig.release(); changed.release(); mask.release(); run.release(); list.release(); count.release(); keep.release();
}
void damage_closure(const uint8_t* changed, int bins_x, int bins_y, const int* rects, const float* radii, int n_nodes, uint8_t* out) {
  if (bins_x < 0 || bins_y < 0 || n_nodes < 0 || n_nodes > kDamageMaxNodes) throw Error(FDH_ERR_INVALID, "fdh_damage_closure: bad grid or node count");
  const size_t nb = (size_t)bins_x * bins_y;
  if (nb && (!changed || !out)) throw Error(FDH_ERR_INVALID, "fdh_damage_closure: null mask");
  if (n_nodes && (!rects || !radii)) throw Error(FDH_ERR_INVALID, "fdh_damage_closure: null node arrays");
  std::vector<DamageRegion> reg((size_t)n_nodes);
  for (int i = 0; i < n_nodes; i++) {
    const int* r = rects + 4 * i;
    const int reach = radii[i] > 0.0f ? make_taps(radii[i]).reach : 0;
    reg[(size_t)i] = damage_region(r[0], r[1], r[2], r[3], reach, bins_x, bins_y);
  }
  std::vector<uint8_t> m(nb), run((size_t)n_nodes + 1);
  for (size_t b = 0; b < nb; b++) m[b] = changed[b] ? 1 : 0;
  damage_close(m.data(), bins_x, reg.data(), n_nodes, run.data(), DamageHostTeam());
  if (nb) std::memcpy(out, m.data(), nb);
}

// ------------------------------------------------------------------ damage readback (include/figdraw_hip_readback.h, figdraw_hip_stream.h, figdraw_hip_exact.h)
void DamageReadback::release() {
  pixels.release(); tiles.release(); code.release(); dir.release(); cursor.release(); stamp.release();
  mirror.release(); arrivals.release(); moved.release(); votes.release();
  mirror_valid = false;
  if (count) (void)hipHostFree((void*)count);
  count = nullptr;
}
void DamageReadback::turn(bool on_now, hipStream_t s) {
  if (on_now && !on) {
    if (!count) {
      FDH_HIP(hipHostMalloc((void**)&count, 64, hipHostMallocDefault));
      count[0] = count[1] = 0;
    }
    all = true;  // what the application holds is unknown: the first read brings every bin
    mirror_valid = have_stats = false;
  }
  if (!on_now && on) {
    FDH_HIP(hipStreamSynchronize(s));
    release();
  }
  on = on_now;
}
// the mask joins the pending set -- unless everything is pending already, or the stamps are those of another frame size (a read lays
// them out anew)
void DamageReadback::accumulate(hipStream_t s, const LaunchJob& J, const uint8_t* mask, const LaunchSpan& span) {
  if (!on) return;
  const int nb = J.bins_x * J.bins_y;
  if (all || w != J.W || h != J.H || stamp.cap < (size_t)nb) all = true;
  else { span(true); launch_damage_accumulate(s, mask, stamp.ptr, epoch, nb, const_cast<uint32_t*>(count)); span(false); }
}
// exact mode keeps its flag while readback is off; the mirror lives only while both are on
void DamageReadback::turn_exact(bool on_now, hipStream_t s) {
  if (on_now && !exact) mirror_valid = have_stats = false;
  if (!on_now && exact) {
    if (mirror.ptr) FDH_HIP(hipStreamSynchronize(s));
    mirror.release(); arrivals.release(); moved.release(); votes.release();
    mirror_valid = false;
  }
  exact = on_now;
}
void DamageReadback::exact_stats(int* n_pending, int* n_changed, int* fresh) const {
  if (!have_stats) throw Error(FDH_ERR_INVALID, "fdh_damage_exact_stats: no read with exact damage readback on yet (fdh_set_damage_exact)");
  if (n_pending) *n_pending = stat_pending;
  if (n_changed) *n_changed = stat_changed;
  if (fresh) *fresh = stat_fresh;
}
int DamageReadback::pending(const char* who, const ReadFrame& F, bool* every) const {
  const int nb = F.bins_x * F.bins_y;
  *every = all || w != F.W || h != F.H;
  const int n = *every ? nb : (int)count[0];
  if (n < 0 || n > nb) throw Error(FDH_ERR_HIP, std::string(who) + ": the pending count is out of range");
  return n;
}
void DamageReadback::consumed(const ReadFrame& F) {
  const size_t nb = (size_t)F.bins_x * F.bins_y;
  // the next epoch's stamp is on no bin; fresh stamps, or an epoch that wrapped, start over (epochs start at 1)
  if (stamp.cap < nb || epoch + 1 == 0) {
    stamp.reserve(nb);
    FDH_HIP(hipMemset(stamp.ptr, 0, stamp.cap * sizeof(uint32_t)));
    epoch = 0;
  }
  epoch++;
  all = false; w = F.W; h = F.H;
  count[0] = 0;
}
int64_t coded_damage_bound(int w, int h) {
  if (w <= 0 || h <= 0) return 0;
  return (int64_t)((w + FDH_TILE_PX - 1) / FDH_TILE_PX) * ((h + FDH_TILE_PX - 1) / FDH_TILE_PX) * FDH_TILE_BYTES;
}
void DamageReadback::lost() {
  mirror_valid = false;
  all = true;
}
// The first read after the mirror became invalid (the mode or readback turned on, another frame size, a lost read) is a fresh one: the
// pending set passes unfiltered, and the mirror takes the whole surface in one launch (k_damage_filter's fill form: the tile-major copy).
// Every other read costs one launch and one synchronise in front of pack / encode: the host needs the count for the tile count, for
// the check of the buffers and for fdh_read_damage_into's choice.
int DamageReadback::filter(const char* who, const ReadFrame& F, int n, bool* every) {
  if (!exact) return n;
  stat_pending = stat_changed = n; stat_fresh = 0;
  have_stats = true;
  if (n <= 0) return n;
  const int nb = F.bins_x * F.bins_y;
  const bool fresh = !mirror_valid || mirror_w != F.W || mirror_h != F.H;
  try {
    mirror_valid = false;
    mirror.reserve_exact((size_t)nb * (kBin * kBin));  // (the stream is idle: a block that grows may be freed)
    arrivals.reserve(1);
    if (*every) stamp.reserve((size_t)nb);  // (every workgroup writes its stamp: none needs a value first)
    uint32_t* const words = const_cast<uint32_t*>(count);
    DamageFilterParams P;
    P.surf = F.surf; P.mirror = mirror.ptr; P.stamp = stamp.ptr; P.arrivals = arrivals.ptr; P.n_changed = words + 3;
    P.epoch = epoch; P.n_pending = (uint32_t)n; P.W = F.W; P.H = F.H; P.bins_x = F.bins_x; P.bins_y = F.bins_y;
    P.all = (fresh || *every) ? 1 : 0; P.fill = fresh ? 1 : 0;
    if (fresh) {
      launch_damage_filter(F.stream, P);
      FDH_HIP(hipGetLastError());
      mirror_valid = true; mirror_w = F.W; mirror_h = F.H;
      stat_fresh = 1;
      return n;
    }
    count[3] = 0xFFFFFFFFu;
    FDH_HIP(hipMemsetAsync(arrivals.ptr, 0, sizeof(unsigned long long), F.stream));
    launch_damage_filter(F.stream, P);
    FDH_HIP(hipGetLastError());
    FDH_HIP(hipStreamSynchronize(F.stream));
    const uint32_t kept = count[3];
    if (kept > (uint32_t)n) throw Error(FDH_ERR_HIP, std::string(who) + ": the filter left no valid count");
    mirror_valid = true;
    *every = false;  // the set lives in the stamps from here on
    stat_changed = (int)kept;
    if (kept == 0) consumed(F);
    return (int)kept;
  } catch (...) {
    lost();
    throw;
  }
}
// Both buffers of a read hold the whole grid's worst case, exactly (doubled, a 4K frame's 33.4 MB would become 64): a read of n tiles
// never moves them, so the pointers of the other kind of read stay where they are.
int DamageReadback::read(const char* who, const ReadFrame& F, int64_t* payload_bytes) {
  const bool coded = payload_bytes != nullptr;
  bool every = false;
  int n = pending(who, F, &every);
  if (coded && (F.W > INT16_MAX || F.H > INT16_MAX || (size_t)coded_damage_bound(F.W, F.H) > (size_t)UINT32_MAX))
    throw Error(FDH_ERR_INVALID, "fdh_read_damage_coded: a directory entry holds coordinates up to 32767 and offsets of 32 bits");
  if (coded) *payload_bytes = 0;
  n = filter(who, F, n, &every);
  if (n <= 0) return n;
  return fetch(who, F, n, every, payload_bytes);
}
int DamageReadback::fetch(const char* who, const ReadFrame& F, int n, bool every, int64_t* payload_bytes, const DamageMoveList* moves) try {
  const bool coded = payload_bytes != nullptr;
  const int nb = F.bins_x * F.bins_y;
  const size_t bound = (size_t)coded_damage_bound(F.W, F.H);  // (= nb tiles of FDH_TILE_BYTES)
  uint32_t* const words = const_cast<uint32_t*>(count);
  count[1] = count[2] = count[4] = 0xFFFFFFFFu;
  if (moves) {
    code.reserve_exact(bound); dir.reserve_exact((size_t)nb); cursor.reserve(2);
    DamageEncodeMovedParams Q;
    DamageEncodeParams& P = Q.enc;
    P.surf = F.surf; P.stamp = stamp.ptr;
    P.payload = code.dev; P.dir = reinterpret_cast<uint2*>(dir.dev);
    P.n_tiles = words + 1; P.payload_bytes = words + 2;
    P.cursor = reinterpret_cast<unsigned long long*>(cursor.ptr);
    P.epoch = epoch; P.n_pending = (uint32_t)n; P.W = F.W; P.H = F.H; P.bins_x = F.bins_x; P.bins_y = F.bins_y; P.all = every ? 1 : 0;
    Q.moved = moved.ptr; Q.moves = *moves; Q.n_copied = words + 4;
    FDH_HIP(hipMemsetAsync(cursor.ptr, 0, 2 * sizeof(uint32_t), F.stream));
    launch_damage_encode_moved(F.stream, Q);
  } else if (coded) {
    code.reserve_exact(bound); dir.reserve_exact((size_t)nb); cursor.reserve(2);
    DamageEncodeParams P;
    P.surf = F.surf; P.stamp = stamp.ptr;  // (`every`: the stamps are not read, and may not exist yet)
    P.payload = code.dev; P.dir = reinterpret_cast<uint2*>(dir.dev);
    P.n_tiles = words + 1; P.payload_bytes = words + 2;
    P.cursor = reinterpret_cast<unsigned long long*>(cursor.ptr);
    P.epoch = epoch; P.n_pending = (uint32_t)n; P.W = F.W; P.H = F.H; P.bins_x = F.bins_x; P.bins_y = F.bins_y; P.all = every ? 1 : 0;
    FDH_HIP(hipMemsetAsync(cursor.ptr, 0, 2 * sizeof(uint32_t), F.stream));
    launch_damage_encode(F.stream, P);
  } else {
    pixels.reserve_exact(bound); tiles.reserve_exact((size_t)nb);
    DamagePackParams P;
    P.surf = F.surf; P.stamp = stamp.ptr;
    P.pixels = pixels.dev; P.tiles = reinterpret_cast<int4*>(tiles.dev);
    P.n_tiles = words + 1;
    P.epoch = epoch; P.W = F.W; P.H = F.H; P.bins_x = F.bins_x; P.bins_y = F.bins_y; P.all = every ? 1 : 0;
    launch_damage_pack(F.stream, P);
  }
  FDH_HIP(hipGetLastError());
  FDH_HIP(hipStreamSynchronize(F.stream));
  if (count[1] != (uint32_t)n) throw Error(FDH_ERR_HIP, std::string(who) + ": the " + (coded ? "encoder's" : "pack's") + " tile count differs from the pending count");
  if (coded) {
    *payload_bytes = (int64_t)count[2];  // (the directory is not read here: the CPU's loads from page-locked memory are slow)
    if (*payload_bytes > (int64_t)bound || *payload_bytes % 16 != 0) throw Error(FDH_ERR_HIP, std::string(who) + ": the encoder left no valid payload size");
    if (moves && count[4] > (uint32_t)n) throw Error(FDH_ERR_HIP, std::string(who) + ": the encoder left no valid count of COPY tiles");
  }
  consumed(F);
  return n;
} catch (...) {
  if (exact) lost();  // the filter has run: the mirror holds tiles the application never got
  throw;
}
// what every read tells beside its buffers
static void report(const ReadFrame& F, int n, int* n_tiles, int* frame_w, int* frame_h, int* full) {
  const int nb = F.bins_x * F.bins_y;
  if (n_tiles) *n_tiles = n;
  if (frame_w) *frame_w = F.W;
  if (frame_h) *frame_h = F.H;
  if (full) *full = (nb > 0 && n == nb) ? 1 : 0;
}
void DamageReadback::read_raw(const ReadFrame& F, const FdhDamageTile** t, const uint8_t** px, int* n_tiles, int* frame_w, int* frame_h, int* full) {
  const int n = read("fdh_read_damage", F, nullptr);
  if (t) *t = tiles.ptr;
  if (px) *px = pixels.ptr;
  report(F, n, n_tiles, frame_w, frame_h, full);
}
void DamageReadback::read_coded(const ReadFrame& F, const FdhCodedTile** t, const uint8_t** payload, int* n_tiles, int64_t* payload_bytes, int* frame_w,
                                int* frame_h, int* full) {
  int64_t bytes = 0;
  const int n = read("fdh_read_damage_coded", F, &bytes);
  if (t) *t = dir.ptr;
  if (payload) *payload = code.ptr;
  if (payload_bytes) *payload_bytes = bytes;
  report(F, n, n_tiles, frame_w, frame_h, full);
}
// ------------------------------------------------------------------ moved reads (include_readback/figdraw_hip_moves.h)
// what both entry points refuse alike, before anything is touched
static void need_exact(const char* who, const DamageReadback& rb) {
  if (!rb.on || !rb.exact) throw Error(FDH_ERR_INVALID, std::string(who) + ": needs damage readback and exact damage readback on (fdh_set_damage_readback, fdh_set_damage_exact)");
}
// The match must see the mirror before the filter stores the new tiles into it, so it runs over the pending set as it is before the
// filter -- a superset of the tiles the encoder will meet.  Both launches are in stream order; the filter's synchronise serves both.
void DamageReadback::read_moved(const ReadFrame& F, const FdhDamageMove* moves, int n_moves, const FdhCodedTile** t, const uint8_t** payload, int* n_tiles,
                                int64_t* payload_bytes, int* frame_w, int* frame_h, int* full, int* n_copied) {
  const char* const who = "fdh_read_damage_moved";
  need_exact(who, *this);
  if (n_moves < 0 || n_moves > kDamageMovesMax) throw Error(FDH_ERR_INVALID, std::string(who) + ": n_moves outside 0 .. 8");
  if (n_moves > 0 && !moves) throw Error(FDH_ERR_INVALID, std::string(who) + ": null moves");
  DamageMoveList L{};
  L.n = n_moves;
  for (int i = 0; i < n_moves; i++) {
    if (moves[i].dx == 0 && moves[i].dy == 0) throw Error(FDH_ERR_INVALID, std::string(who) + ": move " + std::to_string(i) + " is (0, 0)");
    L.dx[i] = moves[i].dx; L.dy[i] = moves[i].dy;
  }
  if (F.W > INT16_MAX || F.H > INT16_MAX || (size_t)coded_damage_bound(F.W, F.H) > (size_t)UINT32_MAX)
    throw Error(FDH_ERR_INVALID, std::string(who) + ": a directory entry holds coordinates up to 32767 and offsets of 32 bits");
  bool every = false;
  int n = pending(who, F, &every);
  int64_t bytes = 0;
  int copied = 0;
  const bool fresh = !mirror_valid || mirror_w != F.W || mirror_h != F.H;
  if (n_moves == 0 || fresh || n <= 0) {
    n = read(who, F, &bytes);  // the coded read, byte for byte
  } else {
    const int nb = F.bins_x * F.bins_y;
    moved.reserve((size_t)nb);  // (the stream is idle)
    DamageMoveMatchParams M;
    M.surf = F.surf; M.mirror = mirror.ptr; M.stamp = stamp.ptr; M.moved = moved.ptr; M.moves = L;
    M.epoch = epoch; M.W = F.W; M.H = F.H; M.bins_x = F.bins_x; M.bins_y = F.bins_y; M.all = every ? 1 : 0;
    launch_damage_move_match(F.stream, M);
    FDH_HIP(hipGetLastError());  // (nothing has changed yet: a failure here leaves set and mirror as they were)
    n = filter(who, F, n, &every);
    if (n > 0) {
      n = fetch(who, F, n, every, &bytes, &L);
      copied = (int)count[4];
    }
  }
  if (t) *t = dir.ptr;
  if (payload) *payload = code.ptr;
  if (payload_bytes) *payload_bytes = bytes;
  if (n_copied) *n_copied = copied;
  report(F, n, n_tiles, frame_w, frame_h, full);
}
void DamageReadback::find_moves(const ReadFrame& F, int max_shift, FdhDamageMove* out_moves, int* out_votes, int cap, int* n_out) {
  const char* const who = "fdh_find_damage_moves";
  need_exact(who, *this);
  if (max_shift < 1 || max_shift > kDamageShiftMax) throw Error(FDH_ERR_INVALID, std::string(who) + ": max_shift outside 1 .. 256");
  if (cap < 0 || (cap > 0 && (!out_moves || !out_votes))) throw Error(FDH_ERR_INVALID, std::string(who) + ": negative cap, or null arrays");
  if (n_out) *n_out = 0;
  bool every = false;
  const int n = pending(who, F, &every);
  if (n <= 0 || !mirror_valid || mirror_w != F.W || mirror_h != F.H) return;
  constexpr int kWords = 2 * kDamageVoteSpan;
  votes.reserve((size_t)kWords);
  DamageMoveVotesParams P;
  P.surf = F.surf; P.mirror = mirror.ptr; P.stamp = stamp.ptr; P.votes = votes.ptr;
  P.epoch = epoch; P.W = F.W; P.H = F.H; P.bins_x = F.bins_x; P.bins_y = F.bins_y; P.all = every ? 1 : 0; P.max_shift = max_shift;
  FDH_HIP(hipMemsetAsync(votes.ptr, 0, kWords * sizeof(uint32_t), F.stream));
  launch_damage_move_votes(F.stream, P);
  FDH_HIP(hipGetLastError());
  std::vector<uint32_t> v((size_t)kWords);
  FDH_HIP(hipMemcpyAsync(v.data(), votes.ptr, kWords * sizeof(uint32_t), hipMemcpyDeviceToHost, F.stream));
  FDH_HIP(hipStreamSynchronize(F.stream));
  struct Cand { uint32_t votes; int d, horizontal; };
  std::vector<Cand> cands;
  for (int hz = 0; hz < 2; hz++)
    for (int d = -max_shift; d <= max_shift; d++)
      if (const uint32_t k = v[(size_t)(hz * kDamageVoteSpan + d + kDamageShiftMax)]) cands.push_back(Cand{k, d, hz});
  // votes descending, then |d| ascending, then vertical before horizontal, then negative d first
  std::sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) {
    if (a.votes != b.votes) return a.votes > b.votes;
    if (std::abs(a.d) != std::abs(b.d)) return std::abs(a.d) < std::abs(b.d);
    if (a.horizontal != b.horizontal) return a.horizontal < b.horizontal;
    return a.d < b.d;
  });
  const int m = std::min(cap, (int)cands.size());
  for (int i = 0; i < m; i++) {
    out_moves[i].dx = (int16_t)(cands[(size_t)i].horizontal ? cands[(size_t)i].d : 0);
    out_moves[i].dy = (int16_t)(cands[(size_t)i].horizontal ? 0 : cands[(size_t)i].d);
    out_votes[i] = (int)cands[(size_t)i].votes;
  }
  if (n_out) *n_out = m;
}
// Tiles cross the link at no more bytes than they hold, but reach the mirror through a second pass on the CPU (fdh_apply_damage out of
// page-locked memory: ~0.7 - 1 us a tile), which a whole-frame copy into the caller's memory does not pay (~0.3 us a bin).  From
// kReadbackWholeNum / kReadbackWholeDen of the grid on, the whole frame is the cheaper way to the same mirror
// (profiles/damage_readback.txt: the crossover sits at 0.26 - 0.36 of the grid at 4K and 1080p).
constexpr int kReadbackWholeNum = 3, kReadbackWholeDen = 10;
void DamageReadback::read_into(const ReadFrame& F, uint8_t* image, int64_t pitch_bytes, int iw, int ih, int* n_tiles) {
  bool every = false;
  int n = pending("fdh_read_damage_into", F, &every);
  if (!image) throw Error(FDH_ERR_INVALID, "fdh_read_damage_into: null image");
  if (iw != F.W || ih != F.H) throw Error(FDH_ERR_INVALID, "fdh_read_damage_into: the image is not the size of the last frame");
  if (pitch_bytes < (int64_t)4 * iw) throw Error(FDH_ERR_INVALID, "fdh_read_damage_into: the pitch is shorter than a row");
  const int nb = F.bins_x * F.bins_y;
  n = filter("fdh_read_damage_into", F, n, &every);  // (exact mode: the rule below weighs what is left; the mirror is already the frame)
  if (n > 0 && (int64_t)n * kReadbackWholeDen >= (int64_t)nb * kReadbackWholeNum) {
    if (hipError_t e = hipMemcpy2D(image, (size_t)pitch_bytes, F.surf, (size_t)iw * 4, (size_t)iw * 4, (size_t)ih, hipMemcpyDeviceToHost)) {
      if (exact) lost();
      FDH_HIP(e);
    }
    consumed(F);
  } else {
    if (n > 0) fetch("fdh_read_damage", F, n, every, nullptr);
    apply_damage(image, pitch_bytes, iw, ih, tiles.ptr, pixels.ptr, n);
  }
  if (n_tiles) *n_tiles = n;
}

// ------------------------------------------------------------------ host only: the receiver's side of both reads
void apply_damage(uint8_t* image, int64_t pitch_bytes, int w, int h, const FdhDamageTile* tiles, const uint8_t* pixels, int n_tiles) {
  if (n_tiles < 0) throw Error(FDH_ERR_INVALID, "fdh_apply_damage: negative tile count");
  if (w < 0 || h < 0 || pitch_bytes < (int64_t)4 * w) throw Error(FDH_ERR_INVALID, "fdh_apply_damage: the pitch is shorter than a row");
  if (n_tiles == 0) return;
  if (!image || !tiles || !pixels) throw Error(FDH_ERR_INVALID, "fdh_apply_damage: null image, tiles or pixels");
  for (int i = 0; i < n_tiles; i++)  // every tile is checked before any byte is written
    if (!tile_in_image(tiles[i].x, tiles[i].y, tiles[i].w, tiles[i].h, w, h))
      throw Error(FDH_ERR_INVALID, "fdh_apply_damage: tile " + std::to_string(i) + " is not a bin inside the image");
  for (int i = 0; i < n_tiles; i++) {
    const FdhDamageTile& t = tiles[i];
    const uint8_t* src = pixels + (size_t)i * FDH_TILE_BYTES;
    for (int r = 0; r < t.h; r++) std::memcpy(image + (int64_t)(t.y + r) * pitch_bytes + (int64_t)4 * t.x, src + (size_t)r * FDH_TILE_PITCH, (size_t)4 * t.w);
  }
}

void decode_damage(uint8_t* image, int64_t pitch_bytes, int w, int h, const FdhCodedTile* tiles, int n_tiles, const uint8_t* payload, int64_t payload_bytes) {
  std::string why;
  if (!decode_tiles("fdh_decode_damage", 1, image, pitch_bytes, w, h, tiles, n_tiles, payload, payload_bytes, &why)) throw Error(FDH_ERR_INVALID, why);
}
void decode_damage_moved(uint8_t* image, int64_t pitch_bytes, int w, int h, const FdhCodedTile* tiles, int n_tiles, const uint8_t* payload, int64_t payload_bytes) {
  std::string why;
  if (!decode_tiles("fdh_decode_damage_moved", 2, image, pitch_bytes, w, h, tiles, n_tiles, payload, payload_bytes, &why)) throw Error(FDH_ERR_INVALID, why);
}

}  // namespace fdh
