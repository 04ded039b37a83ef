// fdh_video_out.cpp -- the four export calls' host side (fdh_video_out.h): fdh_read_video_frame, fdh_read_video_planes, fdh_read_video_422,
// fdh_read_video_alpha, their fdh_check_video_*_target and fdh_video_out_coefficients.  No state: a target is checked, turned into its
// kernel's parameter block and launched.  The check and the read are written once, over a family: its target and parameter block, its own
// rules (null, format, flags, plane counts, evenness, in its own words) and the description of a format's planes.
#include "fdh_video_out.h"

#include <algorithm>
#include <string>
#include <type_traits>

#include "fdh_kernels.h"
#include "fdh_memory.h"  // FDH_HIP, device_view_of
#include "fdh_plain.h"   // Error
#include "fdh_place_batch.h"  // Refusal
#include "fdh_video_export.h"
#include "fdh_video_planar.h"
#include "fdh_video_422.h"
#include "fdh_video_alpha.h"

namespace fdh {
namespace video_out {
namespace ve = video_export;
namespace vp = video_planar;
namespace v2 = video_422;
namespace va = video_alpha;

namespace {
constexpr int kPlanes = va::kPlanes;  // the most a target has
// plane p of a format, for a rectangle of w x h texels: the unit its pointer and pitch are multiples of, and that unit's name in a refusal;
// a row's bytes and the rows; the bytes of a run, which are one store where the pointer and the pitch are multiples of them
struct Plane { bool present; int64_t element; const char* unit; int64_t row, rows, run; };
constexpr const char* kElement = "the element size", *kPair = "a pair's size", *kSample = "the sample size", *kGroup = "the group size";
// what a checked target comes to: the rectangle, and per plane it has the bytes from its pointer to its last row's end
struct Layout {
  int x, y, w, h;
  bool present[kPlanes];
  __int128 bytes[kPlanes];
  int64_t run[kPlanes];
  bool wide[kPlanes];  // a run of plane p is one store
};
bool overlap(uintptr_t a, __int128 a_bytes, uintptr_t b, __int128 b_bytes) { return (__int128)a < (__int128)b + b_bytes && (__int128)b < (__int128)a + a_bytes; }

// behind a family's null test: the format as the family knows it, and the fields that every target has
template <class Target>
void shared_rules(const Refusal& bad, const Target& t, bool known_format) {
  if (!known_format) throw bad("unknown format");
  if (t.matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (t.range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (t.flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (t.reserved[0] || t.reserved[1]) throw bad("reserved must be 0");
}

// ---- the families.  Each: Target and Params; kRun, the texels of a lane's run (wide_src asks for a whole one); rules(), every rule in
// front of "empty frame"; uneven(), why the rectangle's origin will not do, or null; plane(); overlap(), the words for planes p and q;
// ten_bit(), the row of ve::kCoefficients; fill(), the planes into the parameter block; launch()
struct Numbered {  // the three families whose parameter block holds its planes in arrays
  static std::string overlap(int p, int q) { return "planes " + std::to_string(p) + " and " + std::to_string(q) + " overlap"; }
  template <class Params>
  static void fill(Params& P, void* const* plane, const int64_t* pitch, const bool* wide) {
    for (int p = 0; p < (int)std::extent<decltype(P.plane)>::value; p++)
      if (plane[p]) { P.plane[p] = plane[p]; P.pitch[p] = pitch[p]; P.wide[p] = wide[p]; }
  }
};

struct Frame {  // NV12, P010, BGRA8 (the specification: include_video/figdraw_hip_video_out.h)
  using Target = FdhVideoTarget;
  using Params = ve::Params;
  static constexpr int kRun = ve::kRun;
  static void rules(const Refusal& bad, const Target* t) {
    if (!t || !t->planes[0]) throw bad("null target");
    shared_rules(bad, *t, t->format <= FDH_VIDEO_P010);
    if (t->flags & FDH_VIDEO_STRAIGHT_ALPHA) throw bad("FDH_VIDEO_STRAIGHT_ALPHA is for the way in: the surface's bytes go out as stored");
    if (t->format == FDH_VIDEO_BGRA8) {
      if (t->matrix || t->range) throw bad("matrix and range must be 0 for BGRA8");
      if (t->planes[1] || t->pitch_bytes[1]) throw bad("BGRA8 has one plane");
      if (t->flags & FDH_VIDEO_CHROMA_LINEAR) throw bad("FDH_VIDEO_CHROMA_LINEAR needs a chroma plane");
    } else {
      if (!t->planes[1]) throw bad("null chroma plane");
      if (t->flags & FDH_VIDEO_IGNORE_ALPHA) throw bad("FDH_VIDEO_IGNORE_ALPHA is BGRA8's");
    }
  }
  static const char* uneven(uint32_t format, int x, int y) { return format != FDH_VIDEO_BGRA8 && ((x | y) & 1) ? "the rectangle's x and y must be even for NV12 / P010" : nullptr; }
  static Plane plane(uint32_t format, int p, int64_t w, int64_t h) {
    const int64_t luma = format == FDH_VIDEO_BGRA8 ? 4 : format == FDH_VIDEO_P010 ? 2 : 1;  // a run: four luma samples or texels; two pairs
    if (p == 0) return {true, luma, kElement, w * luma, h, 4 * luma};
    return {format != FDH_VIDEO_BGRA8, 2 * luma, kPair, (w + 1) / 2 * 2 * luma, (h + 1) / 2, 4 * luma};
  }
  static std::string overlap(int, int) { return "the two planes overlap"; }
  static bool ten_bit(uint32_t format) { return format == FDH_VIDEO_P010; }
  static void fill(Params& P, void* const* plane, const int64_t* pitch, const bool* wide) {
    P.luma = plane[0]; P.chroma = plane[1];
    P.pitch_y = pitch[0]; P.pitch_c = pitch[1];
    P.wide_y = wide[0]; P.wide_c = wide[1];
  }
  static void launch(hipStream_t s, const Params& P) { launch_video_export(s, P); }
};

struct Planar : Numbered {  // I420, I010, I444, I410 in three planes (the specification: include_video/figdraw_hip_video_planar.h)
  using Target = FdhVideoPlanesTarget;
  using Params = vp::OutParams;
  static constexpr int kRun = vp::kRun;
  static void rules(const Refusal& bad, const Target* t) {
    if (!t || !t->planes[0] || !t->planes[1] || !t->planes[2]) throw bad("null target or plane");
    shared_rules(bad, *t, t->format >= FDH_VIDEO_I420 && t->format <= FDH_VIDEO_I410);
    if (t->flags & (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("the alpha flags are BGRA8's");
    if (vp::full_chroma(t->format) && (t->flags & FDH_VIDEO_CHROMA_LINEAR)) throw bad("FDH_VIDEO_CHROMA_LINEAR is for I420 / I010: a 4:4:4 frame has a chroma sample per texel");
  }
  static const char* uneven(uint32_t format, int x, int y) { return !vp::full_chroma(format) && ((x | y) & 1) ? "the rectangle's x and y must be even for I420 / I010" : nullptr; }
  static Plane plane(uint32_t format, int p, int64_t w, int64_t h) {
    const bool half = p && !vp::full_chroma(format);
    const int64_t es = vp::ten_bit(format) ? 2 : 1;
    return {true, es, kSample, (half ? (w + 1) / 2 : w) * es, half ? (h + 1) / 2 : h, (half ? vp::kRun / 2 : vp::kRun) * es};
  }
  static bool ten_bit(uint32_t format) { return vp::ten_bit(format); }
  static void launch(hipStream_t s, const Params& P) { launch_video_planar_export(s, P); }
};

struct F422 : Numbered {  // I422, I210 in three planes, YUY2, UYVY in one (the specification: include_video/figdraw_hip_video_422.h)
  using Target = FdhVideoPlanesTarget;
  using Params = v2::OutParams;
  static constexpr int kRun = v2::kRun;
  static void rules(const Refusal& bad, const Target* t) {
    if (!t || !t->planes[0]) throw bad("null target or plane");
    shared_rules(bad, *t, v2::known(t->format));
    if (t->flags & (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("the alpha flags are BGRA8's");
    const bool packed = v2::packed(t->format);
    if (packed && (t->planes[1] || t->planes[2] || t->pitch_bytes[1] || t->pitch_bytes[2])) throw bad("planes[1], planes[2] and their pitches must be 0 for YUY2 / UYVY: one plane");
    if (!packed && (!t->planes[1] || !t->planes[2])) throw bad("null target or plane");
  }
  static const char* uneven(uint32_t, int x, int) { return x & 1 ? "the rectangle's x must be even for 4:2:2" : nullptr; }
  static Plane plane(uint32_t format, int p, int64_t w, int64_t h) {
    const bool packed = v2::packed(format);
    const int64_t es = v2::element_bytes(format), cw = (w + 1) / 2;
    return {p < v2::n_planes(format), es, packed ? kGroup : kSample, packed ? 4 * cw : (p ? cw : w) * es, h, v2::run_bytes(format, p)};
  }
  static bool ten_bit(uint32_t format) { return v2::ten_bit(format); }
  static void fill(Params& P, void* const* plane, const int64_t* pitch, const bool* wide) {
    Numbered::fill(P, plane, pitch, wide);
    P.order = P.format == v2::kUYVY;
  }
  static void launch(hipStream_t s, const Params& P) { launch_video_422_export(s, P); }
};

struct Alpha : Numbered {  // A420, A444, A410 in four planes, UYVA in two (the specification: include_video/figdraw_hip_video_alpha.h)
  using Target = FdhVideoAlphaPlanesTarget;
  using Params = va::OutParams;
  static constexpr int kRun = va::kRun;
  static void rules(const Refusal& bad, const Target* t) {
    if (!t || !t->planes[0] || !t->planes[va::kAlpha]) throw bad("null target or plane");
    shared_rules(bad, *t, va::known(t->format));
    if (t->flags & FDH_VIDEO_IGNORE_ALPHA) throw bad("FDH_VIDEO_IGNORE_ALPHA is the sibling call: these formats carry an alpha plane");
    if (va::full_chroma(t->format) && (t->flags & FDH_VIDEO_CHROMA_LINEAR)) throw bad("FDH_VIDEO_CHROMA_LINEAR is for A420 / UYVA: a 4:4:4 frame has a chroma sample per texel");
    const bool packed = va::packed(t->format);
    if (packed && (t->planes[1] || t->planes[2] || t->pitch_bytes[1] || t->pitch_bytes[2])) throw bad("planes[1], planes[2] and their pitches must be 0 for UYVA: a UYVY plane and an alpha plane");
    if (!packed && (!t->planes[1] || !t->planes[2])) throw bad("null target or plane");
  }
  static const char* uneven(uint32_t format, int x, int y) {
    if (format == va::kA420 && ((x | y) & 1)) return "the rectangle's x and y must be even for A420";
    return va::packed(format) && (x & 1) ? "the rectangle's x must be even for UYVA" : nullptr;
  }
  static Plane plane(uint32_t format, int p, int64_t w, int64_t h) {
    const int64_t es = va::element_bytes(format, p);
    return {va::has_plane(format, p), es, es == 4 ? kGroup : kSample, va::row_bytes(format, p, w), va::rows(format, p, h), va::run_bytes(format, p)};
  }
  static bool ten_bit(uint32_t format) { return va::ten_bit(format); }
  static void launch(hipStream_t s, const Params& P) { launch_video_alpha_export(s, P); }
};

// ---- every rule that needs no device, in the order the specifications give them
template <class F>
Layout check(const Refusal& bad, const typename F::Target* t, int frame_w, int frame_h) {
  F::rules(bad, t);
  if (frame_w <= 0 || frame_h <= 0) throw bad("empty frame");
  Layout L{};
  L.x = t->rect[0]; L.y = t->rect[1]; L.w = t->rect[2]; L.h = t->rect[3];
  if (L.w <= 0 || L.h <= 0) { L.x = 0; L.y = 0; L.w = frame_w; L.h = frame_h; }
  if (L.x < 0 || L.y < 0 || (int64_t)L.x + L.w > frame_w || (int64_t)L.y + L.h > frame_h) throw bad("rectangle outside the frame");
  if (const char* why = F::uneven(t->format, L.x, L.y)) throw bad(why);
  constexpr int n = (int)std::extent<decltype(t->planes)>::value;
  for (int p = 0; p < n; p++) {
    const Plane d = F::plane(t->format, p, L.w, L.h);
    if (!d.present) continue;
    if ((uintptr_t)t->planes[p] % (uintptr_t)d.element || t->pitch_bytes[p] % d.element)
      throw bad("planes[" + std::to_string(p) + "] and pitch_bytes[" + std::to_string(p) + "] must be multiples of " + d.unit);
    if (t->pitch_bytes[p] < d.row) throw bad("pitch_bytes[" + std::to_string(p) + "] is below a row's bytes");
    L.present[p] = true;
    L.bytes[p] = (__int128)(d.rows - 1) * t->pitch_bytes[p] + (__int128)d.row;
    L.run[p] = d.run;
    L.wide[p] = (uintptr_t)t->planes[p] % (uintptr_t)d.run == 0 && t->pitch_bytes[p] % d.run == 0 && d.row >= d.run;
  }
  for (int p = 0; p < n; p++)
    for (int q = p + 1; q < n; q++)
      if (L.present[p] && L.present[q] && overlap((uintptr_t)t->planes[p], L.bytes[p], (uintptr_t)t->planes[q], L.bytes[q])) throw bad(F::overlap(p, q));
  return L;
}

// ---- behind the context's part: check(), the planes' addresses on `device` and their distance from `own` and from each other, one launch
// of the family's kernel on `s` reading the W x H surface, and the wait for it
template <class F>
void read_as(const char* who, hipStream_t s, int device, const uint32_t* surface, int W, int H, const typename F::Target* target, const Own* own, int n_own) {
  const Refusal bad{who};
  const Layout L = check<F>(bad, target, W, H);
  const typename F::Target t = *target;
  constexpr int n = (int)std::extent<decltype(t.planes)>::value;
  void* planes[kPlanes] = {nullptr, nullptr, nullptr, nullptr};
  for (int p = 0; p < n; p++) {
    if (!L.present[p]) continue;
    planes[p] = device_view_of(device, t.planes[p]);
    if (!planes[p]) throw bad("a plane is neither device memory of the context's device nor page-locked host memory");
    for (int k = 0; k < n_own; k++)
      if (own[k].base && overlap((uintptr_t)planes[p], L.bytes[p], (uintptr_t)own[k].base, (__int128)own[k].bytes))
        throw bad(std::string("a plane overlaps the context's own ") + own[k].what);
  }
  for (int p = 0; p < n; p++)
    for (int q = p + 1; q < n; q++)
      if (planes[p] && planes[q] && overlap((uintptr_t)planes[p], L.bytes[p], (uintptr_t)planes[q], L.bytes[q])) throw bad(F::overlap(p, q));
  typename F::Params P{};
  P.src = surface + (size_t)L.y * W + L.x;
  P.src_pitch = W;
  P.w = L.w; P.h = L.h;
  P.format = t.format; P.flags = t.flags;
  P.wide_src = (uintptr_t)P.src % 16 == 0 && W % 4 == 0 && L.w >= F::kRun;
  // (a page-locked plane's device view need not be aligned as the caller's pointer is: the question is asked of the address the kernel gets)
  bool wide[kPlanes] = {false, false, false, false};
  for (int p = 0; p < n; p++) wide[p] = planes[p] && L.wide[p] && (uintptr_t)planes[p] % (uintptr_t)L.run[p] == 0;
  F::fill(P, planes, t.pitch_bytes, wide);
  if (t.format != FDH_VIDEO_BGRA8) {
    const int32_t* c = ve::kCoefficients[F::ten_bit(t.format)][t.matrix][t.range];  // (the NV12 row for 8 bit, the P010 row for 10)
    P.yoff = c[0]; P.coff = c[1];
    for (int k = 0; k < 3; k++) { P.ky[k] = c[2 + k]; P.ku[k] = c[5 + k]; P.kv[k] = c[8 + k]; }
  }
  F::launch(s, P);
  FDH_HIP(hipStreamSynchronize(s));
  FDH_HIP(hipGetLastError());
}
}  // namespace

void check_target(const char* who, const FdhVideoTarget* t, int frame_w, int frame_h) { (void)check<Frame>(Refusal{who}, t, frame_w, frame_h); }
void check_planes_target(const char* who, const FdhVideoPlanesTarget* t, int frame_w, int frame_h) { (void)check<Planar>(Refusal{who}, t, frame_w, frame_h); }
void check_422_target(const char* who, const FdhVideoPlanesTarget* t, int frame_w, int frame_h) { (void)check<F422>(Refusal{who}, t, frame_w, frame_h); }
void check_alpha_target(const char* who, const FdhVideoAlphaPlanesTarget* t, int frame_w, int frame_h) { (void)check<Alpha>(Refusal{who}, t, frame_w, frame_h); }

void read(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoTarget* t, const Own* own, int n_own) {
  read_as<Frame>("read_video_frame", s, device, surface, W, H, t, own, n_own);
}
void read_planes(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoPlanesTarget* t, const Own* own, int n_own) {
  read_as<Planar>("read_video_planes", s, device, surface, W, H, t, own, n_own);
}
void read_422(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoPlanesTarget* t, const Own* own, int n_own) {
  read_as<F422>("read_video_422", s, device, surface, W, H, t, own, n_own);
}
void read_alpha(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoAlphaPlanesTarget* t, const Own* own, int n_own) {
  read_as<Alpha>("read_video_alpha", s, device, surface, W, H, t, own, n_own);
}

void coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[11]) {
  const Refusal bad{"video_out_coefficients"};
  if (format != FDH_VIDEO_NV12 && format != FDH_VIDEO_P010) throw bad("the format has no conversion: FDH_VIDEO_NV12 or FDH_VIDEO_P010");
  if (matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (!out) throw bad("null pointer");
  std::copy(ve::kCoefficients[format == FDH_VIDEO_P010][matrix][range], ve::kCoefficients[format == FDH_VIDEO_P010][matrix][range] + 11, out);
}

}  // namespace video_out
}  // namespace fdh
