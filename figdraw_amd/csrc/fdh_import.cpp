// fdh_import.cpp -- class Importer (fdh_import.h): images and decoded video frames from device memory on their way into the atlas, every step
// a kernel on the context's stream.  One body per kind of work: the ten single calls (import_one), the four batch calls (put_batch,
// update_batch); what a family of calls differs in -- its struct's rules, its planes on the device, its first kernel -- is a Source.
#include "fdh_import.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_set>

#include "fdh_kernels.h"
#include "fdh_place_batch.h"  // Refusal, place_batch
#include "fdh_image_batch.h"  // and through it fdh_image_import.h
#include "fdh_video_batch.h"  // and through it fdh_video_import.h
#include "fdh_video_planar.h"
#include "fdh_video_422.h"
#include "fdh_video_alpha.h"

namespace fdh {
namespace ii = image_import;
namespace ib = image_batch;
namespace vi = video_import;
namespace vb = video_batch;
namespace vp = video_planar;
namespace v2 = video_422;
namespace va = video_alpha;

static_assert(ii::kLevels == kMaxMips, "image_import::Params holds every level of an atlas");
void Importer::release() { level5_.release(); minified_.release(); tab_.release(); ink_host_.release(); }

// ---- what every family shares
namespace {
constexpr const char* kSourceElsewhere = "the source is neither device memory of the context's device nor page-locked host memory";
constexpr const char* kPlaneElsewhere = "a plane is neither device memory of the context's device nor page-locked host memory";
constexpr const char* kPlaneInAtlas = "a plane lies inside the context's own atlas";
constexpr const char* kSourceInAtlas = "the source lies in the context's own atlas";

bool overlaps_atlas(const Atlas& atlas, uintptr_t lo, uintptr_t bytes) {
  for (int l = 0; l < atlas.n_levels(); l++) {
    const uintptr_t a = (uintptr_t)atlas.level(l), side = (uintptr_t)(atlas.size() >> l);
    if (lo < a + side * side * 4 && a < lo + bytes) return true;
  }
  return false;
}
// On a context with a device: a plane of `bytes` bytes as the device addresses it -- device memory of `device`, or page-locked host memory.
// Anything else (pageable memory, another device's, an address nobody has mapped) is refused as `elsewhere`, the runtime's sticky error
// cleared behind it (device_view_of, fdh_memory.h); one that meets a level of the atlas as `in_atlas` (null: not asked).
const void* plane_on_device(const Refusal& bad, int device, const Atlas& atlas, const void* plane, int64_t bytes, const char* elsewhere, const char* in_atlas) {
  const void* view = device_view_of(device, plane);
  if (!view) throw bad(elsewhere);
  if (in_atlas && overlaps_atlas(atlas, (uintptr_t)view, (uintptr_t)bytes)) throw bad(in_atlas);
  return view;
}
// what every update asks of its key, ahead of the pointers' check and the buffers (begin_update says the same again)
void known_entry(const Refusal& bad, const Atlas& atlas, int64_t key, int w, int h) {
  const AtlasEntry* old = atlas.find(key);
  if (!old) throw bad("unknown key");
  if (old->w != w || old->h != h) throw bad("size mismatch");
}
// the conversion of a parameter block or a batch record: a row of the table (the NV12 rows for 8 bit, the P010 rows for 10)
template <typename P>
void set_coefficients(P& p, bool ten_bit, uint32_t matrix, uint32_t range) {
  const int32_t* c = vi::kCoefficients[ten_bit][matrix][range];
  p.yoff = c[0]; p.coff = c[1]; p.cy = c[2]; p.crv = c[3]; p.cgu = c[4]; p.cgv = c[5]; p.cbu = c[6];
}
// the destination half of a single import's parameter block: the entry's place, the levels it stores, the atlas, the scratch
template <typename P>
void fill_destination(P& p, const Atlas& atlas, const AtlasEntry& e, uint32_t* scratch, int32_t* ink_block) {
  p.x = e.x; p.y = e.y;
  atlas.each_level(e.x, e.y, e.w, e.h, [&](int, int, int, int, int) { p.n_store++; });
  p.ink = e.w <= ii::kInkMax && e.h <= ii::kInkMax;
  for (int l = 0; l < ii::kTileLevels; l++) { p.lw[l] = (e.w + (1 << l) - 1) >> l; p.lh[l] = (e.h + (1 << l) - 1) >> l; }
  for (int l = 0; l < atlas.n_levels(); l++) p.level[l] = atlas.level(l);
  p.size = atlas.size();
  p.scratch = scratch;
  p.ink_block = ink_block;
}
// an entry's sixteen ink boxes from the folded blocks (fold_ink)
void set_ink(AtlasEntry& e, const int32_t got[ii::kInkWords]) {
  for (int k = 0; k < kInkLevels; k++) {  // (a box no texel grew: empty, at the origin)
    const int32_t *a = got + 4 * k, *c = got + 32 + 4 * k;
    e.ink_a[k] = a[2] ? InkBox{(int16_t)a[0], (int16_t)a[1], (int16_t)a[2], (int16_t)a[3]} : InkBox{0, 0, 0, 0};
    e.ink_rgb[k] = c[2] ? InkBox{(int16_t)c[0], (int16_t)c[1], (int16_t)c[2], (int16_t)c[3]} : InkBox{0, 0, 0, 0};
  }
  e.has_ink = true;
}
}  // namespace

// ---- the single calls.  A Source is constructed from the caller's struct -- what the call asks of it, with no context and no device, and its
// copy (`frame`) --, maps its planes (on a context with a device: as the device addresses them, refused where they are not its to read) and
// launches the family's first kernel, which makes levels 0 .. 5 of the entry; -> the levels the entry stores.
template <typename Source, typename Struct>
void Importer::import_one(const char* who, bool update, hipStream_t s, Atlas& atlas, int device, int64_t key, const Struct* given, int out_rect[4]) {
  const Refusal bad{who};
  Source src(bad, given);
  const int w = src.frame.width, h = src.frame.height;
  if (update) known_entry(bad, atlas, key, w, h);
  if (atlas.has_device()) {
    src.map(bad, device, atlas);
    reserve_import(w, h);
  }
  if (!update) atlas.make_room(s, w, h);
  AtlasEntry& e = update ? atlas.begin_update(who, key, w, h) : atlas.place(s, key, w, h, out_rect);
  if (update) e.has_ink = false;  // (the old texels' boxes; finish_import measures the new ones)
  if (atlas.has_device()) finish_import(s, atlas, e, src.launch(s, atlas, e, level5_.ptr, ink_host_.dev));
}
// the scratch of an import, ahead of the placement as every put reserves: the level-5 image and what k_minify2 makes of it
void Importer::reserve_import(int w, int h) {
  if (w > 16384 || h > 16384) return;  // (no atlas takes it: the placement says so)
  const size_t w5 = (size_t)(w + 31) / 32, h5 = (size_t)(h + 31) / 32;
  level5_.reserve(w5 * h5);
  minified_.reserve(((w5 + 1) / 2) * ((h5 + 1) / 2));
  ink_host_.reserve_exact(ii::kInkTiles * ii::kInkWords);
}
// Two launches for a source up to 2048 x 2048: the family's first kernel makes levels 0 .. 5, k_image_import_tail the rest from the
// level-5 image.  A larger level-5 image first takes k_minify2 / k_atlas_blit steps, as GlyphMaker::glyph_to_atlas does, until the tail's
// workgroup can hold it.  Waits for the stream once; the tiles' ink blocks are in page-locked memory by then (the kernel stores them there).
void Importer::finish_import(hipStream_t s, const Atlas& atlas, AtlasEntry& e, int n_store) {
  uint32_t *cur = level5_.ptr, *nxt = minified_.ptr;
  int l = ii::kTileLevels - 1, cw = (e.w + (1 << l) - 1) >> l, ch = (e.h + (1 << l) - 1) >> l;
  const int tiles = cw * ch;
  for (; (cw > ii::kTailMax || ch > ii::kTailMax) && l + 1 < n_store; std::swap(cur, nxt)) {
    launch_minify2(s, cur, nxt, cw, ch);
    l++; cw = (cw + 1) / 2; ch = (ch + 1) / 2;
    launch_atlas_blit(s, atlas.level(l), atlas.size() >> l, e.x >> l, e.y >> l, nxt, cw, ch);
  }
  if (l + 1 < n_store) {
    ii::TailParams T{};
    T.src = cur; T.sw = cw; T.sh = ch; T.l0 = l; T.n_store = n_store;
    T.x = e.x; T.y = e.y; T.size = atlas.size();
    for (int k = 0; k < atlas.n_levels(); k++) T.level[k] = atlas.level(k);
    launch_image_import_tail(s, T);
  }
  FDH_HIP(hipStreamSynchronize(s));
  FDH_HIP(hipGetLastError());
  e.has_ink = e.w <= ii::kInkMax && e.h <= ii::kInkMax;
  if (!e.has_ink) return;
  int32_t got[ii::kInkWords];
  ii::fold_ink(ink_host_.ptr, tiles, got);
  set_ink(e, got);
}

// ---- images from device memory (the specification: include_glyphs/figdraw_hip_device_image.h).  What the struct is asked; -> whether the
// source's rows are 16-byte aligned (a lane's run of four texels is then one load per plane)
static bool validate_device_image(const Refusal& bad, const FdhDeviceImage* img) {
  if (!img || !img->data) throw bad("null image");
  if (img->width <= 0 || img->height <= 0) throw bad("empty image");
  if (img->format > FDH_IMAGE_PLANAR_F16) throw bad("unknown format");
  if (img->flags & ~(uint32_t)FDH_IMAGE_STRAIGHT_ALPHA) throw bad("unknown flag");
  if (img->reserved) throw bad("reserved must be 0");
  const bool planar = img->format != FDH_IMAGE_RGBA8;
  if (planar ? !(img->channels == 1 || img->channels == 3 || img->channels == 4) : img->channels != 4)
    throw bad("channels must be 4 for RGBA8 and 1, 3 or 4 for a planar format");
  const int64_t element = img->format == FDH_IMAGE_PLANAR_F16 ? 2 : 4;  // (an RGBA8 texel is one aligned word)
  const bool planes = planar && img->channels > 1;
  if ((uintptr_t)img->data % (uintptr_t)element || img->pitch_bytes % element) throw bad("data and pitch_bytes must be multiples of the element size");
  if (img->pitch_bytes < (int64_t)img->width * element) throw bad("pitch_bytes is below a row's bytes");
  if (planes && (__int128)img->plane_bytes < (__int128)img->pitch_bytes * img->height) throw bad("plane_bytes is below pitch_bytes * height");
  if (planes && img->plane_bytes % element) throw bad("plane_bytes must be a multiple of the element size");
  return (uintptr_t)img->data % 16 == 0 && img->pitch_bytes % 16 == 0 && (!planes || img->plane_bytes % 16 == 0);
}
// the source half of ii::Params or of a batch's record; `data` as the device addresses it
template <typename P>
static void set_image(P& p, const FdhDeviceImage& g, const void* data, bool wide) {
  p.data = data; p.pitch_bytes = g.pitch_bytes; p.plane_bytes = g.plane_bytes;
  p.w = g.width; p.h = g.height;
  p.format = g.format; p.channels = g.channels; p.flags = g.flags;
  p.wide = wide && g.width >= 4 ? 1 : 0;
}
namespace {
struct ImageSource {
  FdhDeviceImage frame{};
  const void* data = nullptr;
  bool wide = false;
  ImageSource(const Refusal& bad, const FdhDeviceImage* img) { wide = validate_device_image(bad, img); frame = *img; }
  // (a single call does not ask whether the source lies in the atlas; the batch does)
  void map(const Refusal& bad, int device, const Atlas& atlas) { data = plane_on_device(bad, device, atlas, frame.data, 0, kSourceElsewhere, nullptr); }
  int launch(hipStream_t s, const Atlas& atlas, const AtlasEntry& e, uint32_t* scratch, int32_t* ink_block) const {
    ii::Params P{};
    set_image(P, frame, data, wide);
    fill_destination(P, atlas, e, scratch, ink_block);
    launch_image_import(s, P);
    return P.n_store;
  }
};
}  // namespace
void Importer::put_device_image(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhDeviceImage* img, int out_rect[4]) {
  import_one<ImageSource>("put_image_device", false, s, atlas, device, key, img, out_rect);
}
void Importer::update_device_image(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhDeviceImage* img) {
  import_one<ImageSource>("update_image_device", true, s, atlas, device, key, img, nullptr);
}

// ---- decoded video frames (the specification: include_glyphs/figdraw_hip_video_frame.h): NV12, P010, BGRA8.  What the struct is asked
static void validate_video_frame(const Refusal& bad, const FdhVideoFrame* f, bool* wide_y, bool* wide_c) {
  if (!f || !f->planes[0]) throw bad("null frame");
  if (f->width <= 0 || f->height <= 0) throw bad("empty frame");
  if (f->format > FDH_VIDEO_P010) throw bad("unknown format");
  if (f->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (f->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (f->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (f->reserved[0] || f->reserved[1]) throw bad("reserved must be 0");
  const bool bgra = f->format == FDH_VIDEO_BGRA8;
  const uint32_t alpha = f->flags & (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA);
  if (bgra) {
    if (f->matrix || f->range) throw bad("matrix and range must be 0 for BGRA8");
    if (f->planes[1] || f->pitch_bytes[1]) throw bad("BGRA8 has one plane");
    if (f->flags & FDH_VIDEO_CHROMA_LINEAR) throw bad("FDH_VIDEO_CHROMA_LINEAR needs a chroma plane");
    if (alpha == (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("FDH_VIDEO_STRAIGHT_ALPHA and FDH_VIDEO_IGNORE_ALPHA exclude each other");
  } else {
    if (!f->planes[1]) throw bad("null chroma plane");
    if (alpha) throw bad("the alpha flags are BGRA8's");
  }
  const int64_t luma = bgra ? 4 : f->format == FDH_VIDEO_P010 ? 2 : 1, pair = 2 * luma;  // the planes' element sizes
  if ((uintptr_t)f->planes[0] % (uintptr_t)luma || f->pitch_bytes[0] % luma) throw bad("planes[0] and pitch_bytes[0] must be multiples of the element size");
  if (f->pitch_bytes[0] < (int64_t)f->width * luma) throw bad("pitch_bytes[0] is below a row's bytes");
  const int64_t cw = ((int64_t)f->width + 1) / 2;
  if (!bgra) {
    if ((uintptr_t)f->planes[1] % (uintptr_t)pair || f->pitch_bytes[1] % pair) throw bad("planes[1] and pitch_bytes[1] must be multiples of a pair's size");
    if (f->pitch_bytes[1] < cw * pair) throw bad("pitch_bytes[1] is below a row's bytes");
  }
  const uintptr_t run = (uintptr_t)(4 * luma);  // four luma samples or texels; two pairs
  *wide_y = (uintptr_t)f->planes[0] % run == 0 && f->pitch_bytes[0] % (int64_t)run == 0 && f->width >= 4;
  *wide_c = !bgra && (uintptr_t)f->planes[1] % run == 0 && f->pitch_bytes[1] % (int64_t)run == 0 && cw >= 2;
}
// on a context with a device: both planes as the device addresses them, neither of them inside the atlas (`wide` is not asked again of the
// mapped address; the three- and four-plane families do ask)
static void video_frame_planes(const Refusal& bad, int device, const Atlas& atlas, const FdhVideoFrame& f, const void* out[2]) {
  const int64_t cw = ((int64_t)f.width + 1) / 2, ch = ((int64_t)f.height + 1) / 2;
  const int64_t es = f.format == FDH_VIDEO_BGRA8 ? 4 : f.format == FDH_VIDEO_P010 ? 2 : 1;
  const int64_t bytes[2] = {(f.height - 1) * f.pitch_bytes[0] + f.width * es, (ch - 1) * f.pitch_bytes[1] + cw * 2 * es};
  out[0] = out[1] = nullptr;
  for (int p = 0; p < (f.format == FDH_VIDEO_BGRA8 ? 1 : 2); p++) out[p] = plane_on_device(bad, device, atlas, f.planes[p], bytes[p], kSourceElsewhere, kPlaneInAtlas);
}
// the source half of vi::Params or of a batch's record, but for the planes
template <typename P>
static void set_video_frame(P& p, const FdhVideoFrame& f, bool wide_y, bool wide_c) {
  p.pitch_y = f.pitch_bytes[0]; p.pitch_c = f.pitch_bytes[1];
  p.w = f.width; p.h = f.height; p.cw = (f.width + 1) / 2; p.ch = (f.height + 1) / 2;
  p.format = f.format; p.flags = f.flags;
  p.wide_y = wide_y; p.wide_c = wide_c;
  if (f.format != FDH_VIDEO_BGRA8) set_coefficients(p, f.format == FDH_VIDEO_P010, f.matrix, f.range);
}
namespace {
struct VideoSource {
  FdhVideoFrame frame{};
  const void* planes[2] = {};
  bool wide_y = false, wide_c = false;  // a run of four luma samples / of two chroma pairs is one load (vi::Params)
  VideoSource(const Refusal& bad, const FdhVideoFrame* f) { validate_video_frame(bad, f, &wide_y, &wide_c); frame = *f; }
  void map(const Refusal& bad, int device, const Atlas& atlas) { video_frame_planes(bad, device, atlas, frame, planes); }
  int launch(hipStream_t s, const Atlas& atlas, const AtlasEntry& e, uint32_t* scratch, int32_t* ink_block) const {
    vi::Params P{};
    P.luma = planes[0]; P.chroma = planes[1];
    set_video_frame(P, frame, wide_y, wide_c);
    fill_destination(P, atlas, e, scratch, ink_block);
    launch_video_import(s, P);
    return P.n_store;
  }
};
}  // namespace
void Importer::put_video_frame(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoFrame* frame, int out_rect[4]) {
  import_one<VideoSource>("put_video_frame", false, s, atlas, device, key, frame, out_rect);
}
void Importer::update_video_frame(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoFrame* frame) {
  import_one<VideoSource>("update_video_frame", true, s, atlas, device, key, frame, nullptr);
}
// fdh_video_coefficients: a row of the table (fdh_video_import.h)
void video_coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[7]) {
  const Refusal bad{"video_coefficients"};
  if (format != FDH_VIDEO_NV12 && format != FDH_VIDEO_P010) throw bad("the format has no conversion: FDH_VIDEO_NV12 or FDH_VIDEO_P010");
  if (matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (!out) throw bad("null pointer");
  std::copy(vi::kCoefficients[format == FDH_VIDEO_P010][matrix][range], vi::kCoefficients[format == FDH_VIDEO_P010][matrix][range] + 7, out);
}

// ---- three-plane video frames (the specification: include_video/figdraw_hip_video_planar.h): I420, I010, I444, I410.  What the struct is
// asked; wide[p]: a run of plane p is one load (vp::InParams)
static void validate_video_planes(const Refusal& bad, const FdhVideoPlanes* f, bool wide[3]) {
  if (!f || !f->planes[0] || !f->planes[1] || !f->planes[2]) throw bad("null frame or plane");
  if (f->width <= 0 || f->height <= 0) throw bad("empty frame");
  if (f->format < FDH_VIDEO_I420 || f->format > FDH_VIDEO_I410) throw bad("unknown format");
  if (f->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (f->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (f->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (f->reserved[0] || f->reserved[1]) throw bad("reserved must be 0");
  if (f->flags & (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("the alpha flags are BGRA8's");
  const bool full = vp::full_chroma(f->format);
  if (full && (f->flags & FDH_VIDEO_CHROMA_LINEAR)) throw bad("FDH_VIDEO_CHROMA_LINEAR is for I420 / I010: a 4:4:4 frame has a chroma sample per texel");
  const int64_t es = vp::ten_bit(f->format) ? 2 : 1;  // the sample size
  const int64_t cw = full ? (int64_t)f->width : ((int64_t)f->width + 1) / 2;
  for (int p = 0; p < 3; p++) {
    const int64_t row = p ? cw : (int64_t)f->width, run = (p && !full ? vp::kRun / 2 : vp::kRun) * es;
    if ((uintptr_t)f->planes[p] % (uintptr_t)es || f->pitch_bytes[p] % es) throw bad("planes[" + std::to_string(p) + "] and pitch_bytes[" + std::to_string(p) + "] must be multiples of the sample size");
    if (f->pitch_bytes[p] < row * es) throw bad("pitch_bytes[" + std::to_string(p) + "] is below a row's bytes");
    wide[p] = (uintptr_t)f->planes[p] % (uintptr_t)run == 0 && f->pitch_bytes[p] % run == 0 && row * es >= run;
  }
}
namespace {
struct PlanarSource {
  FdhVideoPlanes frame{};
  const void* planes[3] = {};
  bool wide[3] = {};
  PlanarSource(const Refusal& bad, const FdhVideoPlanes* f) { validate_video_planes(bad, f, wide); frame = *f; }
  void map(const Refusal& bad, int device, const Atlas& atlas) {
    const FdhVideoPlanes& f = frame;
    const bool full = vp::full_chroma(f.format);
    const int64_t es = vp::ten_bit(f.format) ? 2 : 1;
    const int64_t cw = full ? (int64_t)f.width : ((int64_t)f.width + 1) / 2, ch = full ? (int64_t)f.height : ((int64_t)f.height + 1) / 2;
    for (int p = 0; p < 3; p++) {
      const int64_t bytes = ((p ? ch : (int64_t)f.height) - 1) * f.pitch_bytes[p] + (p ? cw : (int64_t)f.width) * es;
      planes[p] = plane_on_device(bad, device, atlas, f.planes[p], bytes, kSourceElsewhere, kPlaneInAtlas);
      // (a page-locked plane's device view need not be aligned as the caller's pointer is: the question is asked of the address the kernel gets)
      wide[p] = wide[p] && (uintptr_t)planes[p] % (uintptr_t)((p && !full ? vp::kRun / 2 : vp::kRun) * es) == 0;
    }
  }
  int launch(hipStream_t s, const Atlas& atlas, const AtlasEntry& e, uint32_t* scratch, int32_t* ink_block) const {
    const FdhVideoPlanes& f = frame;
    const bool full = vp::full_chroma(f.format);
    vp::InParams P{};
    for (int p = 0; p < 3; p++) { P.plane[p] = planes[p]; P.pitch[p] = f.pitch_bytes[p]; P.wide[p] = wide[p]; }
    P.w = f.width; P.h = f.height; P.cw = full ? f.width : (f.width + 1) / 2; P.ch = full ? f.height : (f.height + 1) / 2;
    P.format = f.format; P.flags = f.flags;
    set_coefficients(P, vp::ten_bit(f.format), f.matrix, f.range);
    fill_destination(P, atlas, e, scratch, ink_block);
    launch_video_planar_import(s, P);
    return P.n_store;
  }
};
}  // namespace
void Importer::put_video_planes(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame, int out_rect[4]) {
  import_one<PlanarSource>("put_video_planes", false, s, atlas, device, key, frame, out_rect);
}
void Importer::update_video_planes(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame) {
  import_one<PlanarSource>("update_video_planes", true, s, atlas, device, key, frame, nullptr);
}

// ---- 4:2:2 video frames (the specification: include_video/figdraw_hip_video_422.h): I422, I210 in three planes, YUY2, UYVY in planes[0]
// alone.  What the struct (the three-plane calls') is asked
static void validate_video_422(const Refusal& bad, const FdhVideoPlanes* f, bool wide[3]) {
  if (!f || !f->planes[0]) throw bad("null frame or plane");
  if (f->width <= 0 || f->height <= 0) throw bad("empty frame");
  if (!v2::known(f->format)) throw bad("unknown format");
  if (f->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (f->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (f->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (f->reserved[0] || f->reserved[1]) throw bad("reserved must be 0");
  if (f->flags & (FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("the alpha flags are BGRA8's");
  const bool packed = v2::packed(f->format);
  if (packed && (f->planes[1] || f->planes[2] || f->pitch_bytes[1] || f->pitch_bytes[2])) throw bad("planes[1], planes[2] and their pitches must be 0 for YUY2 / UYVY: one plane");
  if (!packed && (!f->planes[1] || !f->planes[2])) throw bad("null frame or plane");
  const int64_t es = v2::element_bytes(f->format), cw = ((int64_t)f->width + 1) / 2;
  for (int p = 0; p < v2::n_planes(f->format); p++) {
    const int64_t row = packed ? 4 * cw : (p ? cw : (int64_t)f->width) * es, run = v2::run_bytes(f->format, p);
    if ((uintptr_t)f->planes[p] % (uintptr_t)es || f->pitch_bytes[p] % es)
      throw bad("planes[" + std::to_string(p) + "] and pitch_bytes[" + std::to_string(p) + "] must be multiples of the " + (packed ? "group size" : "sample size"));
    if (f->pitch_bytes[p] < row) throw bad("pitch_bytes[" + std::to_string(p) + "] is below a row's bytes");
    wide[p] = (uintptr_t)f->planes[p] % (uintptr_t)run == 0 && f->pitch_bytes[p] % run == 0 && row >= run;
  }
}
namespace {
struct Source422 {
  FdhVideoPlanes frame{};
  const void* planes[3] = {};
  bool wide[3] = {};
  Source422(const Refusal& bad, const FdhVideoPlanes* f) { validate_video_422(bad, f, wide); frame = *f; }
  void map(const Refusal& bad, int device, const Atlas& atlas) {
    const FdhVideoPlanes& f = frame;
    const bool packed = v2::packed(f.format);
    const int64_t es = v2::element_bytes(f.format), cw = ((int64_t)f.width + 1) / 2;
    for (int p = 0; p < v2::n_planes(f.format); p++) {
      const int64_t bytes = ((int64_t)f.height - 1) * f.pitch_bytes[p] + (packed ? 4 * cw : (p ? cw : (int64_t)f.width) * es);
      planes[p] = plane_on_device(bad, device, atlas, f.planes[p], bytes, kSourceElsewhere, kPlaneInAtlas);
      wide[p] = wide[p] && (uintptr_t)planes[p] % (uintptr_t)v2::run_bytes(f.format, p) == 0;  // (of the address the kernel gets: PlanarSource::map)
    }
  }
  int launch(hipStream_t s, const Atlas& atlas, const AtlasEntry& e, uint32_t* scratch, int32_t* ink_block) const {
    const FdhVideoPlanes& f = frame;
    v2::InParams P{};
    for (int p = 0; p < v2::n_planes(f.format); p++) { P.plane[p] = planes[p]; P.pitch[p] = f.pitch_bytes[p]; P.wide[p] = wide[p]; }
    P.w = f.width; P.h = f.height; P.cw = (f.width + 1) / 2;
    P.format = f.format; P.flags = f.flags; P.order = f.format == v2::kUYVY;
    set_coefficients(P, v2::ten_bit(f.format), f.matrix, f.range);
    fill_destination(P, atlas, e, scratch, ink_block);
    launch_video_422_import(s, P);
    return P.n_store;
  }
};
}  // namespace
void Importer::put_video_422(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame, int out_rect[4]) {
  import_one<Source422>("put_video_422", false, s, atlas, device, key, frame, out_rect);
}
void Importer::update_video_422(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame) {
  import_one<Source422>("update_video_422", true, s, atlas, device, key, frame, nullptr);
}

// ---- video frames with an alpha plane (the specification: include_video/figdraw_hip_video_alpha.h): A420, A444, A410 in four planes, UYVA
// in planes[0] and [3].  What the struct is asked
static void validate_video_alpha(const Refusal& bad, const FdhVideoAlphaPlanes* f, bool wide[va::kPlanes]) {
  if (!f || !f->planes[0] || !f->planes[va::kAlpha]) throw bad("null frame or plane");
  if (f->width <= 0 || f->height <= 0) throw bad("empty frame");
  if (!va::known(f->format)) throw bad("unknown format");
  if (f->matrix > FDH_VIDEO_BT2020) throw bad("unknown matrix");
  if (f->range > FDH_VIDEO_FULL) throw bad("unknown range");
  if (f->flags & ~(uint32_t)(FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA | FDH_VIDEO_IGNORE_ALPHA)) throw bad("unknown flag");
  if (f->reserved[0] || f->reserved[1]) throw bad("reserved must be 0");
  if (f->flags & FDH_VIDEO_IGNORE_ALPHA) throw bad("FDH_VIDEO_IGNORE_ALPHA is the sibling call: these formats carry an alpha plane");
  if (va::full_chroma(f->format) && (f->flags & FDH_VIDEO_CHROMA_LINEAR)) throw bad("FDH_VIDEO_CHROMA_LINEAR is for A420 / UYVA: a 4:4:4 frame has a chroma sample per texel");
  const bool packed = va::packed(f->format);
  if (packed && (f->planes[1] || f->planes[2] || f->pitch_bytes[1] || f->pitch_bytes[2])) throw bad("planes[1], planes[2] and their pitches must be 0 for UYVA: a UYVY plane and an alpha plane");
  if (!packed && (!f->planes[1] || !f->planes[2])) throw bad("null frame or plane");
  for (int p = 0; p < va::kPlanes; p++) {
    wide[p] = false;
    if (!va::has_plane(f->format, p)) continue;
    const int64_t es = va::element_bytes(f->format, p), row = va::row_bytes(f->format, p, f->width), run = va::run_bytes(f->format, p);
    if ((uintptr_t)f->planes[p] % (uintptr_t)es || f->pitch_bytes[p] % es)
      throw bad("planes[" + std::to_string(p) + "] and pitch_bytes[" + std::to_string(p) + "] must be multiples of the " + (es == 4 ? "group size" : "sample size"));
    if (f->pitch_bytes[p] < row) throw bad("pitch_bytes[" + std::to_string(p) + "] is below a row's bytes");
    wide[p] = (uintptr_t)f->planes[p] % (uintptr_t)run == 0 && f->pitch_bytes[p] % run == 0 && row >= run;
  }
}
namespace {
struct AlphaSource {
  FdhVideoAlphaPlanes frame{};
  const void* planes[va::kPlanes] = {};
  bool wide[va::kPlanes] = {};
  AlphaSource(const Refusal& bad, const FdhVideoAlphaPlanes* f) { validate_video_alpha(bad, f, wide); frame = *f; }
  void map(const Refusal& bad, int device, const Atlas& atlas) {
    const FdhVideoAlphaPlanes& f = frame;
    for (int p = 0; p < va::kPlanes; p++) {
      if (!va::has_plane(f.format, p)) continue;
      const int64_t bytes = (va::rows(f.format, p, f.height) - 1) * f.pitch_bytes[p] + va::row_bytes(f.format, p, f.width);
      planes[p] = plane_on_device(bad, device, atlas, f.planes[p], bytes, kPlaneElsewhere, kPlaneInAtlas);
      wide[p] = wide[p] && (uintptr_t)planes[p] % (uintptr_t)va::run_bytes(f.format, p) == 0;  // (of the address the kernel gets: PlanarSource::map)
    }
  }
  int launch(hipStream_t s, const Atlas& atlas, const AtlasEntry& e, uint32_t* scratch, int32_t* ink_block) const {
    const FdhVideoAlphaPlanes& f = frame;
    va::InParams P{};
    for (int p = 0; p < va::kPlanes; p++)
      if (va::has_plane(f.format, p)) { P.plane[p] = planes[p]; P.pitch[p] = f.pitch_bytes[p]; P.wide[p] = wide[p]; }
    P.w = f.width; P.h = f.height;
    P.cw = va::full_chroma(f.format) ? f.width : (f.width + 1) / 2; P.ch = (int)va::rows(f.format, 1, f.height);
    P.format = f.format; P.flags = f.flags;
    set_coefficients(P, va::ten_bit(f.format), f.matrix, f.range);
    fill_destination(P, atlas, e, scratch, ink_block);
    launch_video_alpha_import(s, P);
    return P.n_store;
  }
};
}  // namespace
void Importer::put_video_alpha(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoAlphaPlanes* frame, int out_rect[4]) {
  import_one<AlphaSource>("put_video_alpha", false, s, atlas, device, key, frame, out_rect);
}
void Importer::update_video_alpha(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoAlphaPlanes* frame) {
  import_one<AlphaSource>("update_video_alpha", true, s, atlas, device, key, frame, nullptr);
}

// ---- the batches (the specifications: include_glyphs/figdraw_hip_device_images.h, include_glyphs/figdraw_hip_video_frames.h).  What n single
// calls do, in the glyph batches' three passes: every item is validated (the two validate_ functions: nothing behind them refuses an item);
// every item is placed (an update: begun), in order; then the items that are still in the atlas get their texels from a number of launches
// that does not depend on n (the two make functions), over the tables of fdh_image_batch.h and fdh_video_batch.h.  A batch is its records
// and their entries, and what the two kinds of table differ in.
struct Importer::ImageBatch {
  std::vector<ii::BatchImage> tab;    // pass 1: the source as the device addresses it, extents, format, channels, flags, wide; pass 2: the place
  std::vector<AtlasEntry*> entries;   // pass 2: the entries (a placement never moves the ones behind the last growth)
  std::vector<const void*> sources;   // the callers' pointers: what a copy to the host starts from
  static constexpr int32_t FdhImageBatchStats::*kCount = &FdhImageBatchStats::images;
  static size_t tiles_of(int w, int h) { return ib::table_tiles(w, h); }
  static bool has_ink(int w, int h) { return ib::has_ink(w, h); }
  size_t table_words() const { return ib::table_words(tab, kMaxMips); }
};
struct Importer::VideoBatch {
  std::vector<vi::BatchFrame> tab;   // pass 1: planes as the device addresses them, pitches, extents, format, flags, wide, the conversion; pass 2: the place
  std::vector<AtlasEntry*> entries;  // pass 2: the entries
  static constexpr int32_t FdhVideoBatchStats::*kCount = &FdhVideoBatchStats::frames;
  static size_t tiles_of(int w, int h) { return vb::tiles_of(w, h); }
  static bool has_ink(int w, int h) { return vb::has_ink(w, h); }
  size_t table_words() const { return vb::table_words(tab, kMaxMips); }
};
// the buffers of a whole batch, before any placement as every put reserves: the tables whatever atlas the batch ends in, a texel of
// scratch per tile, an ink block per tile of an item that gets ink boxes
template <typename Batch>
void Importer::reserve_batch(const Batch& B) {
  size_t tiles = 0, ink_tiles = 0;
  for (const auto& t : B.tab) {
    const size_t n = Batch::tiles_of(t.w, t.h);
    tiles += n;
    if (Batch::has_ink(t.w, t.h)) ink_tiles += n;
  }
  tab_.reserve(B.table_words());
  level5_.reserve(std::max<size_t>(tiles, 1));
  ink_host_.reserve_exact(std::max<size_t>(ink_tiles, ii::kInkTiles) * ii::kInkWords);
}
template <typename Batch, typename Stats>
void Importer::put_batch(hipStream_t s, Atlas& atlas, const int64_t* keys, int n, int (*out_rects)[4], Batch& B, Stats& stats) {
  stats = Stats{};
  stats.*Batch::kCount = n;
  if (n == 0) return;
  if (atlas.has_device()) reserve_batch(B);
  // ---- pass 2: the places (keep mode: room for all items of the batch at once, before any of them has a place)
  if (atlas.keep()) {
    std::vector<int> wh((size_t)n * 2);
    for (int i = 0; i < n; i++) { wh[(size_t)i * 2] = B.tab[(size_t)i].w; wh[(size_t)i * 2 + 1] = B.tab[(size_t)i].h; }
    atlas.make_room(s, reinterpret_cast<const int (*)[2]>(wh.data()), n);
  }
  int first = 0, placed = 0;
  std::exception_ptr failed = place_batch(s, atlas, n, out_rects, Stored::chain,
                                          [&](int i, int64_t* key, int* w, int* h) { *key = keys[i]; *w = B.tab[(size_t)i].w; *h = B.tab[(size_t)i].h; },
                                          [&](int i, AtlasEntry& e) { B.tab[(size_t)i].x = e.x; B.tab[(size_t)i].y = e.y; B.entries[(size_t)i] = &e; }, &first, &placed);
  stats.written = placed - first;
  stats.dropped_by_growth = first;
  // ---- pass 3: the texels of items first .. placed - 1
  if (placed > first) make(s, atlas, B, first, placed - first);
  if (failed) std::rethrow_exception(failed);
}
template <typename Batch, typename Stats>
void Importer::update_batch(const char* who, hipStream_t s, Atlas& atlas, const int64_t* keys, int n, Batch& B, Stats& stats) {
  stats = Stats{};
  stats.*Batch::kCount = n;
  if (n == 0) return;
  if (atlas.has_device()) reserve_batch(B);
  for (int i = 0; i < n; i++) {
    AtlasEntry& e = atlas.begin_update(who, keys[i], B.tab[(size_t)i].w, B.tab[(size_t)i].h);
    e.has_ink = false;  // (the old texels' boxes; pass 3 measures the new ones)
    B.tab[(size_t)i].x = e.x; B.tab[(size_t)i].y = e.y;
    B.entries[(size_t)i] = &e;
  }
  stats.written = n;
  make(s, atlas, B, 0, n);
}

// ---- batches of device images: one launch per format present and one for the tails
// the source's bytes from `data` to its last element's end
static int64_t source_bytes(const FdhDeviceImage& g) {
  const int64_t element = g.format == FDH_IMAGE_PLANAR_F16 ? 2 : 4;
  const int64_t planes = g.format != FDH_IMAGE_RGBA8 && g.channels > 1 ? g.channels : 1;
  return (planes - 1) * g.plane_bytes + (int64_t)(g.height - 1) * g.pitch_bytes + (int64_t)g.width * element;
}
static void validate_device_images(const char* who, const Atlas& atlas, int device, const int64_t* keys, const FdhDeviceImage* images, int n, bool update, std::vector<ii::BatchImage>* tab) {
  const Refusal bad{who};
  if (n < 0 || (n > 0 && (!keys || !images))) throw bad("bad image array");
  if (n > ib::kMaxImages) throw bad("at most 65535 images");
  tab->assign((size_t)n, ii::BatchImage{});
  std::unordered_set<int64_t> seen;
  int64_t tiles = 0;
  for (int i = 0; i < n; i++) {
    const FdhDeviceImage& g = images[i];
    const bool wide = validate_device_image(bad, &g);
    if (g.width > ii::kBatchMaxExtent || g.height > ii::kBatchMaxExtent) throw bad("an image of a batch is at most 2048 x 2048");
    if (!seen.insert(keys[i]).second) throw bad("a key occurs twice");
    if (update) known_entry(bad, atlas, keys[i], g.width, g.height);
    tiles += (int64_t)ib::covered_tiles(g.width, g.height);
    set_image((*tab)[(size_t)i], g, g.data, wide);
  }
  if (tiles > ib::kMaxTiles) throw bad("at most 2^18 tiles in a batch");
  if (!atlas.has_device()) return;
  for (int i = 0; i < n; i++) (*tab)[(size_t)i].data = plane_on_device(bad, device, atlas, images[i].data, source_bytes(images[i]), kSourceElsewhere, kSourceInAtlas);
}
void Importer::put_device_images(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhDeviceImage* images, int n, int (*out_rects)[4]) {
  ImageBatch B;
  validate_device_images("put_images_device", atlas, device, keys, images, n, false, &B.tab);
  B.entries.assign((size_t)n, nullptr);
  for (int i = 0; i < n; i++) B.sources.push_back(images[i].data);
  put_batch(s, atlas, keys, n, out_rects, B, image_stats_);
}
void Importer::update_device_images(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhDeviceImage* images, int n) {
  ImageBatch B;
  validate_device_images("update_images_device", atlas, device, keys, images, n, true, &B.tab);
  B.entries.assign((size_t)n, nullptr);
  for (int i = 0; i < n; i++) B.sources.push_back(images[i].data);
  update_batch("update_images_device", s, atlas, keys, n, B, image_stats_);
}
// A planar value as the texel's byte, the kernels' import_byte (k_image_import.hip) for the few elements the host converts itself: the one
// row or column of an image 1 texel wide or high, of which nothing is stored and which therefore has no tile in any launch.
static uint32_t host_import_byte(float v) {
  if (v != v) return 0u;
  const float c = std::fmin(std::fmax(v, 0.0f), 1.0f);
  return (uint32_t)std::nearbyint(c * 255.0f);
}
// the texels of such an image from `raw`: its planes one after the other, each n = w * h elements
static void host_import_line(const ii::BatchImage& t, const uint8_t* raw, std::vector<uint32_t>* out) {
  const size_t n = (size_t)t.w * t.h;
  out->resize(n);
  const bool straight = (t.flags & ii::kStraightAlpha) != 0;
  for (size_t i = 0; i < n; i++) {
    uint32_t r, g, b, a;
    if (t.format == ii::kRgba8) {
      uint32_t px;
      std::memcpy(&px, raw + 4 * i, 4);
      r = px & 255u; g = (px >> 8) & 255u; b = (px >> 16) & 255u; a = px >> 24;
    } else {
      auto value = [&](uint32_t plane) {
        if (t.format == ii::kPlanarF32) { float f; std::memcpy(&f, raw + 4 * ((size_t)plane * n + i), 4); return f; }
        uint16_t bits;
        std::memcpy(&bits, raw + 2 * ((size_t)plane * n + i), 2);
        return (float)__builtin_bit_cast(_Float16, bits);
      };
      r = g = b = host_import_byte(value(0)); a = 255u;
      if (t.channels >= 3u) { g = host_import_byte(value(1)); b = host_import_byte(value(2)); }
      if (t.channels == 4u) a = host_import_byte(value(3));
    }
    if (straight) { r = r * a / 255u; g = g * a / 255u; b = b * a / 255u; }
    (*out)[i] = r | (g << 8) | (b << 16) | (a << 24);
  }
}
// Pass 3 of both batches for images first .. first + m - 1, which have their entries: one copy of the tables, at most four launches, one
// wait; then the ink blocks folded per image.  A record-only context counts the tiles and is done.
void Importer::make(hipStream_t s, const Atlas& atlas, ImageBatch& B, int first, int m) {
  if (!atlas.has_device()) {
    for (int k = 0; k < m; k++) image_stats_.tiles += (int32_t)ib::table_tiles(B.tab[(size_t)(first + k)].w, B.tab[(size_t)(first + k)].h);
    return;
  }
  ib::Tables T;
  ib::tables(B.tab, first, m, atlas.n_levels(), &T);
  int launches = 0;
  if (T.n_tiles) {
    FDH_HIP(hipMemcpyAsync(tab_.ptr, T.words.data(), T.words.size() * 4, hipMemcpyHostToDevice, s));
    const ii::BatchImage* d_images = reinterpret_cast<const ii::BatchImage*>(tab_.ptr);
    const uint32_t* d_owner = tab_.ptr + T.owner_at;
    ii::BatchAtlas A{};
    for (int l = 0; l < atlas.n_levels(); l++) A.level[l] = atlas.level(l);
    A.size = atlas.size();
    for (int f = 0; f < ib::kFormats; f++) {
      if (!T.tile_count[f]) continue;
      launch_image_import_batch(s, (uint32_t)f, d_images, tab_.ptr + T.tiles_at + T.tile_first[f], (int)T.tile_count[f], A, level5_.ptr, ink_host_.dev, d_owner);
      launches++;
    }
    if (T.n_tails) {
      launch_image_import_tail_batch(s, d_images, tab_.ptr + T.tails_at, (int)T.n_tails, A, level5_.ptr, d_owner);
      launches++;
    }
    image_stats_.bytes_copied = (int64_t)(T.words.size() * 4);
  }
  // (an image 1 texel wide or high: its one row or column to the host, plane after plane)
  std::vector<std::vector<uint8_t>> lines((size_t)m);
  for (int k = 0; k < m; k++) {
    const ii::BatchImage& t = B.tab[(size_t)(first + k)];
    if (ib::table_tiles(t.w, t.h) || !ib::has_ink(t.w, t.h)) continue;
    const size_t element = t.format == ii::kPlanarF16 ? 2 : 4, planes = t.format != ii::kRgba8 && t.channels > 1u ? t.channels : 1u;
    const size_t row = (size_t)t.w * element, plane = row * t.h;
    lines[(size_t)k].resize(planes * plane);
    for (size_t c = 0; c < planes; c++)
      FDH_HIP(hipMemcpy2DAsync(lines[(size_t)k].data() + c * plane, row, static_cast<const char*>(B.sources[(size_t)(first + k)]) + (int64_t)c * t.plane_bytes, (size_t)t.pitch_bytes, row, (size_t)t.h,
                               hipMemcpyDefault, s));
  }
  FDH_HIP(hipStreamSynchronize(s));  // (`T` and `lines` stay alive until here)
  FDH_HIP(hipGetLastError());
  image_stats_.tiles = (int32_t)T.n_tiles;
  image_stats_.launches = launches;
  std::vector<uint32_t> texels;
  for (int k = 0; k < m; k++) {
    const ii::BatchImage& t = reinterpret_cast<const ii::BatchImage*>(T.words.data())[k];  // (its offsets are in the tables' copy)
    AtlasEntry& e = *B.entries[(size_t)(first + k)];
    int32_t got[ii::kInkWords];
    if (t.ink) {
      ii::fold_ink(ink_host_.ptr + (size_t)t.ink_off * ii::kInkWords, t.lw[ii::kTileLevels - 1] * t.lh[ii::kTileLevels - 1], got);
    } else if (!lines[(size_t)k].empty()) {
      host_import_line(t, lines[(size_t)k].data(), &texels);
      for (int i = 0; i < ii::kInkWords; i++) got[i] = (i & 2) ? 0 : ii::kInkEmpty;
      for (int i = 0; i < t.w * t.h; i++) {
        const uint32_t px = texels[(size_t)i];
        const int x = t.w == 1 ? 0 : i, y = t.w == 1 ? i : 0;
        const int value[2] = {(int)(px >> 24), (int)std::max(px & 255u, std::max((px >> 8) & 255u, (px >> 16) & 255u))};
        for (int kind = 0; kind < 2; kind++)
          for (int j = 0; j < kInkLevels && value[kind] > 16 * j; j++) {
            int32_t* box = got + 32 * kind + 4 * j;
            box[0] = std::min(box[0], x); box[1] = std::min(box[1], y); box[2] = std::max(box[2], x + 1); box[3] = std::max(box[3], y + 1);
          }
      }
    } else {
      e.has_ink = false;
      continue;
    }
    set_ink(e, got);
  }
}

// ---- batches of decoded video frames: one launch per group present (vi::batch_group) and one for the tails
static void validate_video_frames(const char* who, const Atlas& atlas, int device, const int64_t* keys, const FdhVideoFrame* frames, int n, bool update, std::vector<vi::BatchFrame>* tab) {
  const Refusal bad{who};
  if (n < 0 || (n > 0 && (!keys || !frames))) throw bad("bad frame array");
  if (n > vb::kMaxFrames) throw bad("at most 65535 frames");
  tab->assign((size_t)n, vi::BatchFrame{});
  std::unordered_set<int64_t> seen;
  int64_t tiles = 0;
  for (int i = 0; i < n; i++) {
    const FdhVideoFrame& f = frames[i];
    bool wide_y, wide_c;
    validate_video_frame(bad, &f, &wide_y, &wide_c);
    if (f.width > ii::kBatchMaxExtent || f.height > ii::kBatchMaxExtent) throw bad("a frame of a batch is at most 2048 x 2048");
    if (!seen.insert(keys[i]).second) throw bad("a key occurs twice");
    if (update) known_entry(bad, atlas, keys[i], f.width, f.height);
    tiles += (int64_t)vb::tiles_of(f.width, f.height);
    set_video_frame((*tab)[(size_t)i], f, wide_y, wide_c);
  }
  if (tiles > vb::kMaxTiles) throw bad("at most 2^18 tiles in a batch");
  if (!atlas.has_device()) return;
  for (int i = 0; i < n; i++) {
    const void* planes[2];
    video_frame_planes(bad, device, atlas, frames[i], planes);
    (*tab)[(size_t)i].luma = planes[0]; (*tab)[(size_t)i].chroma = planes[1];
  }
}
void Importer::put_video_frames(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhVideoFrame* frames, int n, int (*out_rects)[4]) {
  VideoBatch B;
  validate_video_frames("put_video_frames", atlas, device, keys, frames, n, false, &B.tab);
  B.entries.assign((size_t)n, nullptr);
  put_batch(s, atlas, keys, n, out_rects, B, video_stats_);
}
void Importer::update_video_frames(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhVideoFrame* frames, int n) {
  VideoBatch B;
  validate_video_frames("update_video_frames", atlas, device, keys, frames, n, true, &B.tab);
  B.entries.assign((size_t)n, nullptr);
  update_batch("update_video_frames", s, atlas, keys, n, B, video_stats_);
}
// Pass 3 of both batches for frames first .. first + m - 1, which have their entries: one copy of the tables, at most six launches, one
// wait; then the ink blocks folded per frame.  A record-only context counts the tiles and is done.
void Importer::make(hipStream_t s, const Atlas& atlas, VideoBatch& B, int first, int m) {
  if (!atlas.has_device()) {
    for (int k = 0; k < m; k++) video_stats_.tiles += (int32_t)vb::tiles_of(B.tab[(size_t)(first + k)].w, B.tab[(size_t)(first + k)].h);
    return;
  }
  vb::Tables T;
  vb::tables(B.tab, first, m, atlas.n_levels(), &T);
  FDH_HIP(hipMemcpyAsync(tab_.ptr, T.words.data(), T.words.size() * 4, hipMemcpyHostToDevice, s));
  const vi::BatchFrame* d_frames = reinterpret_cast<const vi::BatchFrame*>(tab_.ptr);
  const uint32_t* d_owner = tab_.ptr + T.owner_at;
  ii::BatchAtlas A{};
  for (int l = 0; l < atlas.n_levels(); l++) A.level[l] = atlas.level(l);
  A.size = atlas.size();
  int launches = 0;
  for (int g = 0; g < vb::kGroups; g++) {
    if (!T.tile_count[g]) continue;
    launch_video_import_batch(s, g, d_frames, tab_.ptr + T.tiles_at + T.tile_first[g], (int)T.tile_count[g], A, level5_.ptr, ink_host_.dev, d_owner);
    launches++;
  }
  if (T.n_tails) {
    launch_image_import_tail_batch(s, reinterpret_cast<const ii::BatchImage*>(tab_.ptr + T.tail_records_at), tab_.ptr + T.tails_at, (int)T.n_tails, A, level5_.ptr, d_owner);
    launches++;
  }
  FDH_HIP(hipStreamSynchronize(s));  // (`T` stays alive until here)
  FDH_HIP(hipGetLastError());
  video_stats_.bytes_copied = (int64_t)(T.words.size() * 4);
  video_stats_.tiles = (int32_t)T.n_tiles;
  video_stats_.launches = launches;
  for (int k = 0; k < m; k++) {
    const vi::BatchFrame& t = B.tab[(size_t)(first + k)];  // (tables() filled in its offsets)
    AtlasEntry& e = *B.entries[(size_t)(first + k)];
    e.has_ink = t.ink != 0;
    if (!t.ink) continue;
    int32_t got[ii::kInkWords];
    ii::fold_ink(ink_host_.ptr + (size_t)t.ink_off * ii::kInkWords, t.lw[ii::kTileLevels - 1] * t.lh[ii::kTileLevels - 1], got);
    set_ink(e, got);
  }
}

}  // namespace fdh
