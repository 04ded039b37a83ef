// fdh_video_out.cpp -- fdh_read_video_frame, fdh_check_video_target and fdh_video_out_coefficients (fdh_video_out.h; the specification:
// include_video/figdraw_hip_video_out.h).  No state: a target is checked, turned into k_video_export's parameter block and launched.
// Behind them the same for three planes: fdh_read_video_planes and fdh_check_video_planes_target (include_video/figdraw_hip_video_planar.h;
// k_video_planar_export), and for 4:2:2: fdh_read_video_422 and fdh_check_video_422_target (include_video/figdraw_hip_video_422.h;
// k_video_422_export), and with an alpha plane: fdh_read_video_alpha and fdh_check_video_alpha_target
// (include_video/figdraw_hip_video_alpha.h; k_video_alpha_export).
#include "fdh_video_out.h"

#include <algorithm>
#include <string>

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
// what a checked target comes to: the rectangle, and the bytes from each plane's pointer to its last element's end
struct Layout {
  int x, y, w, h;
  int64_t cw, ch;
  __int128 bytes[2];
  bool wide_y, wide_c;  // a run of four luma samples / of two chroma pairs is one store (ve::Params)
};
bool overlap(uintptr_t a, __int128 a_bytes, uintptr_t b, __int128 b_bytes) { return (__int128)a < (__int128)b + b_bytes && (__int128)b < (__int128)a + a_bytes; }

Layout check(const Refusal& bad, const FdhVideoTarget* t, int frame_w, int frame_h) {
  if (!t || !t->planes[0]) throw bad("null target");
  if (t->format > FDH_VIDEO_P010) throw bad("unknown format");
  if (t->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (t->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (t->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (t->reserved[0] || t->reserved[1]) throw bad("reserved must be 0");
  if (t->flags & FDH_VIDEO_STRAIGHT_ALPHA) throw bad("FDH_VIDEO_STRAIGHT_ALPHA is for the way in: the surface's bytes go out as stored");
  const bool bgra = t->format == FDH_VIDEO_BGRA8;
  if (bgra) {
    if (t->matrix || t->range) throw bad("matrix and range must be 0 for BGRA8");
    if (t->planes[1] || t->pitch_bytes[1]) throw bad("BGRA8 has one plane");
    if (t->flags & FDH_VIDEO_CHROMA_LINEAR) throw bad("FDH_VIDEO_CHROMA_LINEAR needs a chroma plane");
  } else {
    if (!t->planes[1]) throw bad("null chroma plane");
    if (t->flags & FDH_VIDEO_IGNORE_ALPHA) throw bad("FDH_VIDEO_IGNORE_ALPHA is BGRA8's");
  }
  if (frame_w <= 0 || frame_h <= 0) throw bad("empty frame");
  Layout L{};
  L.x = t->rect[0]; L.y = t->rect[1]; L.w = t->rect[2]; L.h = t->rect[3];
  if (L.w <= 0 || L.h <= 0) { L.x = 0; L.y = 0; L.w = frame_w; L.h = frame_h; }
  if (L.x < 0 || L.y < 0 || (int64_t)L.x + L.w > frame_w || (int64_t)L.y + L.h > frame_h) throw bad("rectangle outside the frame");
  if (!bgra && ((L.x | L.y) & 1)) throw bad("the rectangle's x and y must be even for NV12 / P010");
  const int64_t luma = bgra ? 4 : t->format == FDH_VIDEO_P010 ? 2 : 1, pair = 2 * luma;  // the planes' element sizes
  if ((uintptr_t)t->planes[0] % (uintptr_t)luma || t->pitch_bytes[0] % luma) throw bad("planes[0] and pitch_bytes[0] must be multiples of the element size");
  if (t->pitch_bytes[0] < (int64_t)L.w * luma) throw bad("pitch_bytes[0] is below a row's bytes");
  L.cw = ((int64_t)L.w + 1) / 2; L.ch = ((int64_t)L.h + 1) / 2;
  L.bytes[0] = (__int128)(L.h - 1) * t->pitch_bytes[0] + (__int128)L.w * luma;
  if (!bgra) {
    if ((uintptr_t)t->planes[1] % (uintptr_t)pair || t->pitch_bytes[1] % pair) throw bad("planes[1] and pitch_bytes[1] must be multiples of a pair's size");
    if (t->pitch_bytes[1] < L.cw * pair) throw bad("pitch_bytes[1] is below a row's bytes");
    L.bytes[1] = (__int128)(L.ch - 1) * t->pitch_bytes[1] + (__int128)L.cw * pair;
    if (overlap((uintptr_t)t->planes[0], L.bytes[0], (uintptr_t)t->planes[1], L.bytes[1])) throw bad("the two planes overlap");
  }
  const uintptr_t run = (uintptr_t)(4 * luma);  // four luma samples or texels; two pairs
  L.wide_y = (uintptr_t)t->planes[0] % run == 0 && t->pitch_bytes[0] % (int64_t)run == 0 && L.w >= 4;
  L.wide_c = !bgra && (uintptr_t)t->planes[1] % run == 0 && t->pitch_bytes[1] % (int64_t)run == 0 && L.cw >= 2;
  return L;
}
}  // namespace

void check_target(const char* who, const FdhVideoTarget* t, int frame_w, int frame_h) { (void)check(Refusal{who}, t, frame_w, frame_h); }

void coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[11]) {
  const Refusal bad{"video_out_coefficients"};
  if (format != FDH_VIDEO_NV12 && format != FDH_VIDEO_P010) throw bad("the format has no conversion: FDH_VIDEO_NV12 or FDH_VIDEO_P010");
  if (matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (!out) throw bad("null pointer");
  std::copy(ve::kCoefficients[format == FDH_VIDEO_P010][matrix][range], ve::kCoefficients[format == FDH_VIDEO_P010][matrix][range] + 11, out);
}

void read(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoTarget* target, const Own* own, int n_own) {
  const Refusal bad{"read_video_frame"};
  const Layout L = check(bad, target, W, H);
  const FdhVideoTarget t = *target;
  const int n_planes = t.format == FDH_VIDEO_BGRA8 ? 1 : 2;
  void* planes[2] = {nullptr, nullptr};
  for (int p = 0; p < n_planes; p++) {
    planes[p] = device_view_of(device, t.planes[p]);
    if (!planes[p]) throw bad("a plane is neither device memory of the context's device nor page-locked host memory");
    for (int k = 0; k < n_own; k++)
      if (own[k].base && overlap((uintptr_t)planes[p], L.bytes[p], (uintptr_t)own[k].base, (__int128)own[k].bytes))
        throw bad(std::string("a plane overlaps the context's own ") + own[k].what);
  }
  if (n_planes == 2 && overlap((uintptr_t)planes[0], L.bytes[0], (uintptr_t)planes[1], L.bytes[1])) throw bad("the two planes overlap");
  ve::Params P{};
  P.src = surface + (size_t)L.y * W + L.x;
  P.src_pitch = W;
  P.w = L.w; P.h = L.h;
  P.luma = planes[0]; P.chroma = planes[1];
  P.pitch_y = t.pitch_bytes[0]; P.pitch_c = t.pitch_bytes[1];
  P.format = t.format; P.flags = t.flags;
  P.wide_src = (uintptr_t)P.src % 16 == 0 && W % 4 == 0 && L.w >= 4;
  // (a page-locked plane's device view need not be aligned as the caller's pointer is: the question is asked of the address the kernel gets)
  const uintptr_t run = t.format == FDH_VIDEO_BGRA8 ? 16 : t.format == FDH_VIDEO_P010 ? 8 : 4;
  P.wide_y = L.wide_y && (uintptr_t)planes[0] % run == 0;
  P.wide_c = L.wide_c && (uintptr_t)planes[1] % run == 0;
  if (t.format != FDH_VIDEO_BGRA8) {
    const int32_t* c = ve::kCoefficients[t.format == FDH_VIDEO_P010][t.matrix][t.range];
    P.yoff = c[0]; P.coff = c[1];
    for (int k = 0; k < 3; k++) { P.ky[k] = c[2 + k]; P.ku[k] = c[5 + k]; P.kv[k] = c[8 + k]; }
  }
  launch_video_export(s, P);
  FDH_HIP(hipStreamSynchronize(s));
  FDH_HIP(hipGetLastError());
}

// ---- three planes: I420, I010, I444, I410 (the specification: include_video/figdraw_hip_video_planar.h)
namespace {
// what a checked planar target comes to: the rectangle, each plane's extent in samples, and the bytes from its pointer to its last sample's end
struct PlanarLayout {
  int x, y, w, h;
  int64_t pw[3], ph[3];
  __int128 bytes[3];
  bool wide[3];  // a run of plane p is one store (vp::OutParams)
};
int64_t run_bytes(uint32_t format, int p) { return (p && !vp::full_chroma(format) ? vp::kRun / 2 : vp::kRun) * (vp::ten_bit(format) ? 2 : 1); }

PlanarLayout check_planes(const Refusal& bad, const FdhVideoPlanesTarget* t, int frame_w, int frame_h) {
  if (!t || !t->planes[0] || !t->planes[1] || !t->planes[2]) throw bad("null target or plane");
  if (t->format < FDH_VIDEO_I420 || t->format > FDH_VIDEO_I410) throw bad("unknown format");
  if (t->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (t->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (t->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (t->reserved[0] || t->reserved[1]) throw bad("reserved must be 0");
  if (t->flags & (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("the alpha flags are BGRA8's");
  const bool full = vp::full_chroma(t->format);
  if (full && (t->flags & FDH_VIDEO_CHROMA_LINEAR)) throw bad("FDH_VIDEO_CHROMA_LINEAR is for I420 / I010: a 4:4:4 frame has a chroma sample per texel");
  if (frame_w <= 0 || frame_h <= 0) throw bad("empty frame");
  PlanarLayout L{};
  L.x = t->rect[0]; L.y = t->rect[1]; L.w = t->rect[2]; L.h = t->rect[3];
  if (L.w <= 0 || L.h <= 0) { L.x = 0; L.y = 0; L.w = frame_w; L.h = frame_h; }
  if (L.x < 0 || L.y < 0 || (int64_t)L.x + L.w > frame_w || (int64_t)L.y + L.h > frame_h) throw bad("rectangle outside the frame");
  if (!full && ((L.x | L.y) & 1)) throw bad("the rectangle's x and y must be even for I420 / I010");
  const int64_t es = vp::ten_bit(t->format) ? 2 : 1;  // the sample size
  for (int p = 0; p < 3; p++) {
    L.pw[p] = p && !full ? ((int64_t)L.w + 1) / 2 : L.w; L.ph[p] = p && !full ? ((int64_t)L.h + 1) / 2 : L.h;
    if ((uintptr_t)t->planes[p] % (uintptr_t)es || t->pitch_bytes[p] % es) throw bad("planes[" + std::to_string(p) + "] and pitch_bytes[" + std::to_string(p) + "] must be multiples of the sample size");
    if (t->pitch_bytes[p] < L.pw[p] * es) throw bad("pitch_bytes[" + std::to_string(p) + "] is below a row's bytes");
    L.bytes[p] = (__int128)(L.ph[p] - 1) * t->pitch_bytes[p] + (__int128)L.pw[p] * es;
    const int64_t run = run_bytes(t->format, p);
    L.wide[p] = (uintptr_t)t->planes[p] % (uintptr_t)run == 0 && t->pitch_bytes[p] % run == 0 && L.pw[p] * es >= run;
  }
  for (int p = 0; p < 3; p++)
    for (int q = p + 1; q < 3; q++)
      if (overlap((uintptr_t)t->planes[p], L.bytes[p], (uintptr_t)t->planes[q], L.bytes[q])) throw bad("planes " + std::to_string(p) + " and " + std::to_string(q) + " overlap");
  return L;
}
}  // namespace

void check_planes_target(const char* who, const FdhVideoPlanesTarget* t, int frame_w, int frame_h) { (void)check_planes(Refusal{who}, t, frame_w, frame_h); }

void read_planes(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoPlanesTarget* target, const Own* own, int n_own) {
  const Refusal bad{"read_video_planes"};
  const PlanarLayout L = check_planes(bad, target, W, H);
  const FdhVideoPlanesTarget t = *target;
  void* planes[3] = {nullptr, nullptr, nullptr};
  for (int p = 0; p < 3; p++) {
    planes[p] = device_view_of(device, t.planes[p]);
    if (!planes[p]) throw bad("a plane is neither device memory of the context's device nor page-locked host memory");
    for (int k = 0; k < n_own; k++)
      if (own[k].base && overlap((uintptr_t)planes[p], L.bytes[p], (uintptr_t)own[k].base, (__int128)own[k].bytes))
        throw bad(std::string("a plane overlaps the context's own ") + own[k].what);
  }
  for (int p = 0; p < 3; p++)
    for (int q = p + 1; q < 3; q++)
      if (overlap((uintptr_t)planes[p], L.bytes[p], (uintptr_t)planes[q], L.bytes[q])) throw bad("planes " + std::to_string(p) + " and " + std::to_string(q) + " overlap");
  vp::OutParams P{};
  P.src = surface + (size_t)L.y * W + L.x;
  P.src_pitch = W;
  P.w = L.w; P.h = L.h;
  P.format = t.format; P.flags = t.flags;
  P.wide_src = (uintptr_t)P.src % 16 == 0 && W % 4 == 0 && L.w >= vp::kRun;
  for (int p = 0; p < 3; p++) {
    P.plane[p] = planes[p]; P.pitch[p] = t.pitch_bytes[p];
    // (a page-locked plane's device view need not be aligned as the caller's pointer is: the question is asked of the address the kernel gets)
    P.wide[p] = L.wide[p] && (uintptr_t)planes[p] % (uintptr_t)run_bytes(t.format, p) == 0;
  }
  const int32_t* c = ve::kCoefficients[vp::ten_bit(t.format)][t.matrix][t.range];  // (the NV12 row for 8 bit, the P010 row for 10)
  P.yoff = c[0]; P.coff = c[1];
  for (int k = 0; k < 3; k++) { P.ky[k] = c[2 + k]; P.ku[k] = c[5 + k]; P.kv[k] = c[8 + k]; }
  launch_video_planar_export(s, P);
  FDH_HIP(hipStreamSynchronize(s));
  FDH_HIP(hipGetLastError());
}

// ---- 4:2:2: I422, I210 in three planes, YUY2, UYVY in one (the specification: include_video/figdraw_hip_video_422.h)
namespace {
// what a checked 4:2:2 target comes to: the rectangle, its planes, and per plane a row's bytes and the bytes from its pointer to its last row's end
struct Layout422 {
  int x, y, w, h, n;
  int64_t row[3];
  __int128 bytes[3];
  bool wide[3];  // a run of plane p is one store (v2::OutParams)
};

Layout422 check_422(const Refusal& bad, const FdhVideoPlanesTarget* t, int frame_w, int frame_h) {
  if (!t || !t->planes[0]) throw bad("null target or plane");
  if (!v2::known(t->format)) throw bad("unknown format");
  if (t->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (t->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (t->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (t->reserved[0] || t->reserved[1]) throw bad("reserved must be 0");
  if (t->flags & (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("the alpha flags are BGRA8's");
  const bool packed = v2::packed(t->format);
  if (packed && (t->planes[1] || t->planes[2] || t->pitch_bytes[1] || t->pitch_bytes[2])) throw bad("planes[1], planes[2] and their pitches must be 0 for YUY2 / UYVY: one plane");
  if (!packed && (!t->planes[1] || !t->planes[2])) throw bad("null target or plane");
  if (frame_w <= 0 || frame_h <= 0) throw bad("empty frame");
  Layout422 L{};
  L.x = t->rect[0]; L.y = t->rect[1]; L.w = t->rect[2]; L.h = t->rect[3];
  if (L.w <= 0 || L.h <= 0) { L.x = 0; L.y = 0; L.w = frame_w; L.h = frame_h; }
  if (L.x < 0 || L.y < 0 || (int64_t)L.x + L.w > frame_w || (int64_t)L.y + L.h > frame_h) throw bad("rectangle outside the frame");
  if (L.x & 1) throw bad("the rectangle's x must be even for 4:2:2");
  L.n = v2::n_planes(t->format);
  const int64_t es = v2::element_bytes(t->format), cw = ((int64_t)L.w + 1) / 2;
  for (int p = 0; p < L.n; p++) {
    L.row[p] = packed ? 4 * cw : (p ? cw : (int64_t)L.w) * es;
    if ((uintptr_t)t->planes[p] % (uintptr_t)es || t->pitch_bytes[p] % es)
      throw bad("planes[" + std::to_string(p) + "] and pitch_bytes[" + std::to_string(p) + "] must be multiples of the " + (packed ? "group size" : "sample size"));
    if (t->pitch_bytes[p] < L.row[p]) throw bad("pitch_bytes[" + std::to_string(p) + "] is below a row's bytes");
    L.bytes[p] = (__int128)(L.h - 1) * t->pitch_bytes[p] + (__int128)L.row[p];
    const int64_t run = v2::run_bytes(t->format, p);
    L.wide[p] = (uintptr_t)t->planes[p] % (uintptr_t)run == 0 && t->pitch_bytes[p] % run == 0 && L.row[p] >= run;
  }
  for (int p = 0; p < L.n; p++)
    for (int q = p + 1; q < L.n; q++)
      if (overlap((uintptr_t)t->planes[p], L.bytes[p], (uintptr_t)t->planes[q], L.bytes[q])) throw bad("planes " + std::to_string(p) + " and " + std::to_string(q) + " overlap");
  return L;
}
}  // namespace

void check_422_target(const char* who, const FdhVideoPlanesTarget* t, int frame_w, int frame_h) { (void)check_422(Refusal{who}, t, frame_w, frame_h); }

void read_422(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoPlanesTarget* target, const Own* own, int n_own) {
  const Refusal bad{"read_video_422"};
  const Layout422 L = check_422(bad, target, W, H);
  const FdhVideoPlanesTarget t = *target;
  void* planes[3] = {nullptr, nullptr, nullptr};
  for (int p = 0; p < L.n; p++) {
    planes[p] = device_view_of(device, t.planes[p]);
    if (!planes[p]) throw bad("a plane is neither device memory of the context's device nor page-locked host memory");
    for (int k = 0; k < n_own; k++)
      if (own[k].base && overlap((uintptr_t)planes[p], L.bytes[p], (uintptr_t)own[k].base, (__int128)own[k].bytes))
        throw bad(std::string("a plane overlaps the context's own ") + own[k].what);
  }
  for (int p = 0; p < L.n; p++)
    for (int q = p + 1; q < L.n; q++)
      if (overlap((uintptr_t)planes[p], L.bytes[p], (uintptr_t)planes[q], L.bytes[q])) throw bad("planes " + std::to_string(p) + " and " + std::to_string(q) + " overlap");
  v2::OutParams P{};
  P.src = surface + (size_t)L.y * W + L.x;
  P.src_pitch = W;
  P.w = L.w; P.h = L.h;
  P.format = t.format; P.flags = t.flags; P.order = t.format == v2::kUYVY;
  P.wide_src = (uintptr_t)P.src % 16 == 0 && W % 4 == 0 && L.w >= v2::kRun;
  for (int p = 0; p < L.n; p++) {
    P.plane[p] = planes[p]; P.pitch[p] = t.pitch_bytes[p];
    // (a page-locked plane's device view need not be aligned as the caller's pointer is: the question is asked of the address the kernel gets)
    P.wide[p] = L.wide[p] && (uintptr_t)planes[p] % (uintptr_t)v2::run_bytes(t.format, p) == 0;
  }
  const int32_t* c = ve::kCoefficients[v2::ten_bit(t.format)][t.matrix][t.range];  // (the NV12 row for 8 bit, the P010 row for 10)
  P.yoff = c[0]; P.coff = c[1];
  for (int k = 0; k < 3; k++) { P.ky[k] = c[2 + k]; P.ku[k] = c[5 + k]; P.kv[k] = c[8 + k]; }
  launch_video_422_export(s, P);
  FDH_HIP(hipStreamSynchronize(s));
  FDH_HIP(hipGetLastError());
}

// ---- with an alpha plane: A420, A444, A410 in four planes, UYVA in two (the specification: include_video/figdraw_hip_video_alpha.h)
namespace {
// what a checked target with an alpha plane comes to: the rectangle, and per plane it has the bytes from its pointer to its last row's end
struct LayoutAlpha {
  int x, y, w, h;
  __int128 bytes[va::kPlanes];
  bool wide[va::kPlanes];  // a run of plane p is one store (va::OutParams)
};

LayoutAlpha check_alpha(const Refusal& bad, const FdhVideoAlphaPlanesTarget* t, int frame_w, int frame_h) {
  if (!t || !t->planes[0] || !t->planes[va::kAlpha]) throw bad("null target or plane");
  if (!va::known(t->format)) throw bad("unknown format");
  if (t->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (t->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (t->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (t->reserved[0] || t->reserved[1]) throw bad("reserved must be 0");
  if (t->flags & FDH_VIDEO_IGNORE_ALPHA) throw bad("FDH_VIDEO_IGNORE_ALPHA is the sibling call: these formats carry an alpha plane");
  if (va::full_chroma(t->format) && (t->flags & FDH_VIDEO_CHROMA_LINEAR)) throw bad("FDH_VIDEO_CHROMA_LINEAR is for A420 / UYVA: a 4:4:4 frame has a chroma sample per texel");
  const bool packed = va::packed(t->format);
  if (packed && (t->planes[1] || t->planes[2] || t->pitch_bytes[1] || t->pitch_bytes[2])) throw bad("planes[1], planes[2] and their pitches must be 0 for UYVA: a UYVY plane and an alpha plane");
  if (!packed && (!t->planes[1] || !t->planes[2])) throw bad("null target or plane");
  if (frame_w <= 0 || frame_h <= 0) throw bad("empty frame");
  LayoutAlpha L{};
  L.x = t->rect[0]; L.y = t->rect[1]; L.w = t->rect[2]; L.h = t->rect[3];
  if (L.w <= 0 || L.h <= 0) { L.x = 0; L.y = 0; L.w = frame_w; L.h = frame_h; }
  if (L.x < 0 || L.y < 0 || (int64_t)L.x + L.w > frame_w || (int64_t)L.y + L.h > frame_h) throw bad("rectangle outside the frame");
  if (t->format == va::kA420 && ((L.x | L.y) & 1)) throw bad("the rectangle's x and y must be even for A420");
  if (packed && (L.x & 1)) throw bad("the rectangle's x must be even for UYVA");
  for (int p = 0; p < va::kPlanes; p++) {
    if (!va::has_plane(t->format, p)) continue;
    const int64_t es = va::element_bytes(t->format, p), row = va::row_bytes(t->format, p, L.w), run = va::run_bytes(t->format, p);
    if ((uintptr_t)t->planes[p] % (uintptr_t)es || t->pitch_bytes[p] % es)
      throw bad("planes[" + std::to_string(p) + "] and pitch_bytes[" + std::to_string(p) + "] must be multiples of the " + (es == 4 ? "group size" : "sample size"));
    if (t->pitch_bytes[p] < row) throw bad("pitch_bytes[" + std::to_string(p) + "] is below a row's bytes");
    L.bytes[p] = (__int128)(va::rows(t->format, p, L.h) - 1) * t->pitch_bytes[p] + (__int128)row;
    L.wide[p] = (uintptr_t)t->planes[p] % (uintptr_t)run == 0 && t->pitch_bytes[p] % run == 0 && row >= run;
  }
  for (int p = 0; p < va::kPlanes; p++)
    for (int q = p + 1; q < va::kPlanes; q++)
      if (va::has_plane(t->format, p) && va::has_plane(t->format, q) && overlap((uintptr_t)t->planes[p], L.bytes[p], (uintptr_t)t->planes[q], L.bytes[q]))
        throw bad("planes " + std::to_string(p) + " and " + std::to_string(q) + " overlap");
  return L;
}
}  // namespace

void check_alpha_target(const char* who, const FdhVideoAlphaPlanesTarget* t, int frame_w, int frame_h) { (void)check_alpha(Refusal{who}, t, frame_w, frame_h); }

void read_alpha(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoAlphaPlanesTarget* target, const Own* own, int n_own) {
  const Refusal bad{"read_video_alpha"};
  const LayoutAlpha L = check_alpha(bad, target, W, H);
  const FdhVideoAlphaPlanesTarget t = *target;
  void* planes[va::kPlanes] = {nullptr, nullptr, nullptr, nullptr};
  for (int p = 0; p < va::kPlanes; p++) {
    if (!va::has_plane(t.format, p)) continue;
    planes[p] = device_view_of(device, t.planes[p]);
    if (!planes[p]) throw bad("a plane is neither device memory of the context's device nor page-locked host memory");
    for (int k = 0; k < n_own; k++)
      if (own[k].base && overlap((uintptr_t)planes[p], L.bytes[p], (uintptr_t)own[k].base, (__int128)own[k].bytes))
        throw bad(std::string("a plane overlaps the context's own ") + own[k].what);
  }
  for (int p = 0; p < va::kPlanes; p++)
    for (int q = p + 1; q < va::kPlanes; q++)
      if (planes[p] && planes[q] && overlap((uintptr_t)planes[p], L.bytes[p], (uintptr_t)planes[q], L.bytes[q])) throw bad("planes " + std::to_string(p) + " and " + std::to_string(q) + " overlap");
  va::OutParams P{};
  P.src = surface + (size_t)L.y * W + L.x;
  P.src_pitch = W;
  P.w = L.w; P.h = L.h;
  P.format = t.format; P.flags = t.flags;
  P.wide_src = (uintptr_t)P.src % 16 == 0 && W % 4 == 0 && L.w >= va::kRun;
  for (int p = 0; p < va::kPlanes; p++) {
    if (!planes[p]) continue;
    P.plane[p] = planes[p]; P.pitch[p] = t.pitch_bytes[p];
    // (a page-locked plane's device view need not be aligned as the caller's pointer is: the question is asked of the address the kernel gets)
    P.wide[p] = L.wide[p] && (uintptr_t)planes[p] % (uintptr_t)va::run_bytes(t.format, p) == 0;
  }
  const int32_t* c = ve::kCoefficients[va::ten_bit(t.format)][t.matrix][t.range];  // (the NV12 row for 8 bit, the P010 row for 10)
  P.yoff = c[0]; P.coff = c[1];
  for (int k = 0; k < 3; k++) { P.ky[k] = c[2 + k]; P.ku[k] = c[5 + k]; P.kv[k] = c[8 + k]; }
  launch_video_alpha_export(s, P);
  FDH_HIP(hipStreamSynchronize(s));
  FDH_HIP(hipGetLastError());
}

}  // namespace video_out
}  // namespace fdh
