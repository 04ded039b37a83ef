// fdh_capi.cpp -- extern "C" surface of libfigdraw_hip.so (include/figdraw_hip.h).  Every entry point
// converts C++ exceptions into a negative FdhStatus + a thread-local message: nothing throws across the ABI.
#include <string>

#include "fdh_context.h"
#include "fdh_damage.h"
#include "../../include/figdraw_hip_damage.h"
#include "../../include/figdraw_hip_pick.h"
#include "../../include/figdraw_hip_readback.h"
#include "../../include/figdraw_hip_stream.h"
#include "../../include/figdraw_hip_exact.h"
#include "../../include_schedule/figdraw_hip_schedule.h"
#include "../../include_readback/figdraw_hip_moves.h"
#include "../../include_glyphs/figdraw_hip_glyphs.h"
#include "../../include_glyphs/figdraw_hip_coverage.h"
#include "../../include_glyphs/figdraw_hip_cubic.h"
#include "../../include_glyphs/figdraw_hip_image_sdf.h"
#include "../../include_glyphs/figdraw_hip_device_image.h"
#include "../../include_glyphs/figdraw_hip_device_images.h"
#include "../../include_glyphs/figdraw_hip_video_frame.h"
#include "../../include_glyphs/figdraw_hip_atlas.h"
#include "../../include_video/figdraw_hip_video_out.h"
#include "../../include_video/figdraw_hip_video_planar.h"
#include "../../include_video/figdraw_hip_video_422.h"
#include "../../include_video/figdraw_hip_video_alpha.h"

using fdh::Context;

namespace {
thread_local std::string g_last_error;

template <typename F>
int guard(F&& f) {
  try {
    f();
    return FDH_OK;
  } catch (const fdh::Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return FDH_ERR_INVALID;
  } catch (...) {
    g_last_error = "unknown error";
    return FDH_ERR_INVALID;
  }
}
inline Context* C(FdhContext* c) {
  if (!c) throw fdh::Error(FDH_ERR_INVALID, "null FdhContext");
  return reinterpret_cast<Context*>(c);
}
}  // namespace

extern "C" {

const char* fdh_last_error(void) { return g_last_error.c_str(); }
#if FDH_STATS
extern "C++" { namespace fdh { void debug_counters(unsigned long long out[128], bool reset); void debug_wave_times(unsigned long long* out); } }
__attribute__((visibility("default"))) int fdh_debug_wave_times(unsigned long long* out) { fdh::debug_wave_times(out); return 0; }
__attribute__((visibility("default"))) int fdh_debug_counters(unsigned long long out[128], int reset) { fdh::debug_counters(out, reset != 0); return 0; }
#endif
int fdh_saturated_core(const float rect[4], const float rx[4], const float ry[4], int mode, float factor, float spread,
                       const float shape[2], float aa, int out_px[4]) {
  return guard([&] { fdh::saturated_core_of(rect, rx, ry, mode, factor, spread, shape, aa, out_px); });
}
/* Diagnostic, host-only, for the test-suite (not part of the installed header): fdh_saturated_core for the whole core as the bin launch
 * sees it -- a union of up to three rectangles, DrawRec's own, the full-width band and the full-height band between the corner cells --,
 * 3 x {x0, y0, x1, y1} in out_px as decoded from the draw's BinRec, empty ones as zeros; *n_out = how many are not empty.  push != 0: the
 * record is a clip push (fdh_begin_mask) of that rounded rectangle instead of a draw.  FDH_CORE_UNION=0 leaves the first rectangle alone. */
__attribute__((visibility("default"))) int fdh_saturated_core_union(const float rect[4], const float rx[4], const float ry[4], int mode, float factor, float spread,
                             const float shape[2], float aa, int push, int out_px[12], int* n_out) {
  return guard([&] {
    if (!out_px || !n_out) throw fdh::Error(FDH_ERR_INVALID, "fdh_saturated_core_union: null pointer");
    *n_out = fdh::saturated_core_union_of(rect, rx, ry, mode, factor, spread, shape, aa, push, out_px);
  });
}
int fdh_blur_weight_fragments(float blur_radius, int vertical, float* dense, uint16_t* frag_bits, int* reach, int* k_steps) {
  return guard([&] {
    if (!dense || !frag_bits || !reach || !k_steps) throw fdh::Error(FDH_ERR_INVALID, "fdh_blur_weight_fragments: null pointer");
    fdh::blur_weight_fragments(blur_radius, vertical != 0, dense, frag_bits, reach, k_steps);
  });
}
const char* fdh_version(void) { return "figdraw_hip 0.1.0 (gfx950)"; }
int fdh_sizeof_fig(void) { return (int)sizeof(FdhFig); }
int fdh_sizeof_glyph(void) { return (int)sizeof(FdhGlyph); }
int fdh_sizeof_draw_op(void) { return (int)sizeof(FdhDrawOp); }
int fdh_sizeof_text_rect(void) { return (int)sizeof(FdhTextRect); }

int fdh_create(FdhContext** out, int atlas_size, float pixel_scale, int device, uint32_t flags) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "fdh_create: null out pointer");
    *out = nullptr;
    *out = reinterpret_cast<FdhContext*>(new Context(atlas_size, pixel_scale, device, flags));
  });
}
int fdh_destroy(FdhContext* c) { return guard([&] { delete C(c); }); }
int fdh_set_stream(FdhContext* c, void* s) { return guard([&] { C(c)->set_stream(s); }); }

int fdh_begin_frame(FdhContext* c, int w, int h, int clear, const float rgba[4]) {
  return guard([&] {
    const float white[4] = {1, 1, 1, 1};
    C(c)->begin_frame(w, h, clear != 0, rgba ? rgba : white);
  });
}
int fdh_end_frame(FdhContext* c) { return guard([&] { C(c)->end_frame(); }); }
int fdh_save_transform(FdhContext* c) { return guard([&] { C(c)->save_transform(); }); }
int fdh_restore_transform(FdhContext* c) { return guard([&] { C(c)->restore_transform(); }); }
int fdh_translate(FdhContext* c, float x, float y) { return guard([&] { C(c)->translate(x, y); }); }
int fdh_rotate(FdhContext* c, float a) { return guard([&] { C(c)->rotate(a); }); }
int fdh_scale(FdhContext* c, float sx, float sy) { return guard([&] { C(c)->scale(sx, sy); }); }
int fdh_apply_transform(FdhContext* c, const float m[16]) { return guard([&] { C(c)->apply_transform(m); }); }
int fdh_transform_mirrors_y(FdhContext* c, int* out) { return guard([&] { *out = C(c)->transform_mirrors_y() ? 1 : 0; }); }
int fdh_set_aa_factor(FdhContext* c, float aa) { return guard([&] { C(c)->set_aa(aa); }); }
int fdh_get_aa_factor(FdhContext* c, float* out) { return guard([&] { *out = C(c)->aa(); }); }
int fdh_get_pixel_scale(FdhContext* c, float* out) { return guard([&] { *out = C(c)->pixel_scale(); }); }

int fdh_draw_rounded_rect_sdf(FdhContext* c, const float rect[4], const FdhColor colors[4], const float rx[4], const float ry[4],
                              int mode, float factor, float spread, const float shape[2], int fill_mode, FdhColor mid,
                              FdhColor stop, float mid_pos) {
  return guard([&] {
    const float zero2[2] = {0, 0};
    C(c)->draw_rounded_rect_sdf(rect, colors, rx, ry ? ry : rx, mode, factor, spread, shape ? shape : zero2, fill_mode, mid, stop, mid_pos);
  });
}
int fdh_draw_rounded_rect_fill(FdhContext* c, const float rect[4], const FdhFill* fill, const float rx[4], const float ry[4],
                               int mode, float factor, float spread, const float shape[2]) {
  return guard([&] {
    if (!fill) throw fdh::Error(FDH_ERR_INVALID, "null fill");
    const float zero2[2] = {0, 0};
    C(c)->draw_rounded_rect_fill(rect, *fill, rx, ry ? ry : rx, mode, factor, spread, shape ? shape : zero2);
  });
}
int fdh_draw_image(FdhContext* c, int64_t key, const float pos[2], const FdhColor colors[4], const float size[2], int flip_y) {
  return guard([&] {
    const float zero2[2] = {0, 0};
    C(c)->draw_image(key, pos, colors, size ? size : zero2, flip_y != 0);
  });
}
int fdh_draw_image_adj(FdhContext* c, int64_t key, const float pos[2], FdhColor color, const float size[2]) {
  return guard([&] {
    if (!pos || !size) throw fdh::Error(FDH_ERR_INVALID, "fdh_draw_image_adj: null pointer");
    C(c)->draw_image_adj(key, pos, color, size);
  });
}
int fdh_draw_msdf(FdhContext* c, int64_t key, const float pos[2], FdhColor color, const float size[2], float px_range,
                  float sd_threshold, float stroke_weight, int mtsdf, int flip_y) {
  return guard([&] { C(c)->draw_msdf(key, pos, color, size, px_range, sd_threshold, stroke_weight, mtsdf != 0, flip_y != 0); });
}
int fdh_draw_backdrop_blur(FdhContext* c, const float rect[4], const float rx[4], const float ry[4], float blur_radius) {
  return guard([&] { C(c)->draw_backdrop_blur(rect, rx, ry ? ry : rx, blur_radius); });
}
int fdh_begin_mask(FdhContext* c, const float rect[4], const float rx[4], const float ry[4]) {
  return guard([&] { C(c)->begin_mask(rect, rx, ry ? ry : rx); });
}
int fdh_end_mask(FdhContext* c) { return guard([&] { C(c)->end_mask(); }); }
int fdh_pop_mask(FdhContext* c) { return guard([&] { C(c)->pop_mask(); }); }
int fdh_begin_rect_mask(FdhContext* c, const float rect[4], const float rx[4], const float ry[4]) {
  return guard([&] { C(c)->begin_rect_mask(rect, rx, ry ? ry : rx); });
}
int fdh_pop_rect_mask(FdhContext* c) { return guard([&] { C(c)->pop_rect_mask(); }); }
int fdh_draw_quadratic_bezier_sdf(FdhContext* c, const float rect[4], const FdhFill* fill, const float p0[2], const float p1[2],
                                  const float p2[2], float stroke_weight, int cap) {
  return guard([&] {
    if (!fill) throw fdh::Error(FDH_ERR_INVALID, "null fill");
    C(c)->draw_quadratic_bezier_sdf(rect, *fill, p0, p1, p2, stroke_weight, cap);
  });
}
int fdh_draw_filled_quad(FdhContext* c, const float verts[8], const FdhColor colors[4]) {
  return guard([&] { C(c)->draw_filled_quad(verts, colors); });
}
int fdh_draw_rect(FdhContext* c, const float rect[4], FdhColor color) { return guard([&] { C(c)->draw_rect(rect, color); }); }
int fdh_set_text_subpixel_positioning(FdhContext* c, int e) { return guard([&] { C(c)->set_subpixel_enabled(e != 0); }); }
int fdh_set_text_subpixel_glyph_variants(FdhContext* c, int e) { return guard([&] { C(c)->set_subpixel_variants(e != 0); }); }
int fdh_set_text_subpixel_shift(FdhContext* c, float s) { return guard([&] { C(c)->set_subpixel_shift(s); }); }
int fdh_set_text_lcd_filtering(FdhContext* c, int e) { return guard([&] { C(c)->set_text_lcd_filtering(e != 0); }); }
int fdh_get_text_lcd_filtering(FdhContext* c, int* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "null output");
    *out = C(c)->text_lcd_filtering() ? 1 : 0;
  });
}

int fdh_put_image(FdhContext* c, int64_t key, int w, int h, const uint8_t* rgba, int out_rect[4]) {
  return guard([&] { C(c)->put_image(key, w, h, rgba, out_rect); });
}
int fdh_put_glyph_image(FdhContext* c, int64_t key, int w, int h, const uint8_t* rgba, uint32_t flags, int out_rect[4]) {
  return guard([&] { C(c)->put_glyph_image(key, w, h, rgba, flags, out_rect); });
}
int fdh_put_glyph_outline(FdhContext* c, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]) {
  return guard([&] { C(c)->put_glyph_outline(key, w, h, segs, n, flags, out_rect); });
}
int fdh_put_image_mips(FdhContext* c, int64_t key, int n_levels, const int* widths, const int* heights,
                       const uint8_t* const* premul_rgba8, int out_rect[4]) {
  return guard([&] { C(c)->put_mips(key, n_levels, widths, heights, premul_rgba8, out_rect); });
}
int fdh_put_flippy(FdhContext* c, int64_t key, const uint8_t* bytes, size_t n, int out_rect[4]) {
  return guard([&] { C(c)->put_flippy(key, bytes, n, out_rect); });
}
int fdh_update_image(FdhContext* c, int64_t key, int w, int h, const uint8_t* rgba) {
  return guard([&] { C(c)->update_image(key, w, h, rgba); });
}
int fdh_remove_image(FdhContext* c, int64_t key) { return guard([&] { C(c)->remove_image(key); }); }
int fdh_put_glyph_outline_cubic(FdhContext* c, int64_t key, int w, int h, const float* segs, int n, uint32_t flags, int out_rect[4]) {
  return guard([&] { C(c)->put_glyph_outline_cubic(key, w, h, segs, n, flags, out_rect); });
}
int fdh_put_glyph_outlines(FdhContext* c, const FdhGlyphOutline* glyphs, int n_glyphs, uint32_t flags, int (*out_rects)[4]) {
  return guard([&] { C(c)->put_glyph_outlines(glyphs, n_glyphs, flags, out_rects); });
}
int fdh_put_glyph_outlines_cubic(FdhContext* c, const FdhGlyphOutline* glyphs, int n_glyphs, uint32_t flags, int (*out_rects)[4]) {
  return guard([&] { C(c)->put_glyph_outlines_cubic(glyphs, n_glyphs, flags, out_rects); });
}
int fdh_glyph_batch_stats(FdhContext* c, FdhGlyphBatchStats* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "fdh_glyph_batch_stats: null pointer");
    *out = C(c)->glyph_batch_stats();
  });
}
int fdh_sizeof_glyph_outline(void) { return (int)sizeof(FdhGlyphOutline); }
int fdh_put_glyph_coverage_batch(FdhContext* c, const FdhGlyphOutline* glyphs, int n_glyphs, uint32_t flags, int (*out_rects)[4]) {
  return guard([&] { C(c)->put_glyph_coverage_batch(glyphs, n_glyphs, flags, out_rects); });
}
int fdh_put_glyph_coverage_batch_cubic(FdhContext* c, const FdhGlyphOutline* glyphs, int n_glyphs, uint32_t flags, int (*out_rects)[4]) {
  return guard([&] { C(c)->put_glyph_coverage_batch_cubic(glyphs, n_glyphs, flags, out_rects); });
}
int fdh_put_image_sdf(FdhContext* c, int64_t key, int w, int h, const uint8_t* rgba, int channel, int pad, uint32_t flags, int out_rect[4]) {
  return guard([&] { C(c)->put_image_sdf(key, w, h, rgba, channel, pad, flags, out_rect); });
}
int fdh_put_image_device(FdhContext* c, int64_t key, const FdhDeviceImage* img, int out_rect[4]) {
  return guard([&] { C(c)->put_image_device(key, img, out_rect); });
}
int fdh_update_image_device(FdhContext* c, int64_t key, const FdhDeviceImage* img) {
  return guard([&] { C(c)->update_image_device(key, img); });
}
// batches of them (include_glyphs/figdraw_hip_device_images.h)
int fdh_put_images_device(FdhContext* c, const int64_t* keys, const FdhDeviceImage* images, int n, int (*out_rects)[4]) {
  return guard([&] { C(c)->put_images_device(keys, images, n, out_rects); });
}
int fdh_update_images_device(FdhContext* c, const int64_t* keys, const FdhDeviceImage* images, int n) {
  return guard([&] { C(c)->update_images_device(keys, images, n); });
}
int fdh_image_batch_stats(FdhContext* c, FdhImageBatchStats* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "fdh_image_batch_stats: null pointer");
    *out = C(c)->image_batch_stats();
  });
}
int fdh_sizeof_device_image(void) { return (int)sizeof(FdhDeviceImage); }
// decoded video frames (include_glyphs/figdraw_hip_video_frame.h)
int fdh_put_video_frame(FdhContext* c, int64_t key, const FdhVideoFrame* frame, int out_rect[4]) {
  return guard([&] { C(c)->put_video_frame(key, frame, out_rect); });
}
int fdh_update_video_frame(FdhContext* c, int64_t key, const FdhVideoFrame* frame) {
  return guard([&] { C(c)->update_video_frame(key, frame); });
}
int fdh_put_video_frames(FdhContext* c, const int64_t* keys, const FdhVideoFrame* frames, int n, int (*out_rects)[4]) {
  return guard([&] { C(c)->put_video_frames(keys, frames, n, out_rects); });
}
int fdh_update_video_frames(FdhContext* c, const int64_t* keys, const FdhVideoFrame* frames, int n) {
  return guard([&] { C(c)->update_video_frames(keys, frames, n); });
}
int fdh_video_batch_stats(FdhContext* c, FdhVideoBatchStats* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "fdh_video_batch_stats: null pointer");
    *out = C(c)->video_batch_stats();
  });
}
int fdh_sizeof_video_frame(void) { return (int)sizeof(FdhVideoFrame); }
int fdh_video_coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[7]) {
  return guard([&] { fdh::video_coefficients(format, matrix, range, out); });
}
// the rendered frame out as NV12, P010 or BGRA8 (include_video/figdraw_hip_video_out.h)
int fdh_read_video_frame(FdhContext* c, const FdhVideoTarget* target) {
  return guard([&] { C(c)->read_video_frame(target); });
}
int fdh_check_video_target(const FdhVideoTarget* target, int frame_w, int frame_h) {
  return guard([&] { fdh::video_out::check_target("check_video_target", target, frame_w, frame_h); });
}
int fdh_video_out_coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[11]) {
  return guard([&] { fdh::video_out::coefficients(format, matrix, range, out); });
}
// three-plane video in and out: I420, I010, I444, I410 (include_video/figdraw_hip_video_planar.h)
int fdh_put_video_planes(FdhContext* c, int64_t key, const FdhVideoPlanes* frame, int out_rect[4]) {
  return guard([&] { C(c)->put_video_planes(key, frame, out_rect); });
}
int fdh_update_video_planes(FdhContext* c, int64_t key, const FdhVideoPlanes* frame) {
  return guard([&] { C(c)->update_video_planes(key, frame); });
}
int fdh_read_video_planes(FdhContext* c, const FdhVideoPlanesTarget* target) {
  return guard([&] { C(c)->read_video_planes(target); });
}
int fdh_check_video_planes_target(const FdhVideoPlanesTarget* target, int frame_w, int frame_h) {
  return guard([&] { fdh::video_out::check_planes_target("check_video_planes_target", target, frame_w, frame_h); });
}
// 4:2:2 video in and out: I422, I210, YUY2, UYVY (include_video/figdraw_hip_video_422.h)
int fdh_put_video_422(FdhContext* c, int64_t key, const FdhVideoPlanes* frame, int out_rect[4]) {
  return guard([&] { C(c)->put_video_422(key, frame, out_rect); });
}
int fdh_update_video_422(FdhContext* c, int64_t key, const FdhVideoPlanes* frame) {
  return guard([&] { C(c)->update_video_422(key, frame); });
}
int fdh_read_video_422(FdhContext* c, const FdhVideoPlanesTarget* target) {
  return guard([&] { C(c)->read_video_422(target); });
}
int fdh_check_video_422_target(const FdhVideoPlanesTarget* target, int frame_w, int frame_h) {
  return guard([&] { fdh::video_out::check_422_target("check_video_422_target", target, frame_w, frame_h); });
}
// video with an alpha plane in and out: A420, A444, A410, UYVA (include_video/figdraw_hip_video_alpha.h)
int fdh_put_video_alpha(FdhContext* c, int64_t key, const FdhVideoAlphaPlanes* frame, int out_rect[4]) {
  return guard([&] { C(c)->put_video_alpha(key, frame, out_rect); });
}
int fdh_update_video_alpha(FdhContext* c, int64_t key, const FdhVideoAlphaPlanes* frame) {
  return guard([&] { C(c)->update_video_alpha(key, frame); });
}
int fdh_read_video_alpha(FdhContext* c, const FdhVideoAlphaPlanesTarget* target) {
  return guard([&] { C(c)->read_video_alpha(target); });
}
int fdh_check_video_alpha_target(const FdhVideoAlphaPlanesTarget* target, int frame_w, int frame_h) {
  return guard([&] { fdh::video_out::check_alpha_target("check_video_alpha_target", target, frame_w, frame_h); });
}
int fdh_put_image_sdf_of(FdhContext* c, int64_t src_key, int64_t key, int channel, int pad, uint32_t flags, int out_rect[4]) {
  return guard([&] { C(c)->put_image_sdf_of(src_key, key, channel, pad, flags, out_rect); });
}
int fdh_glyph_coverage_batch_stats(FdhContext* c, FdhGlyphBatchStats* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "fdh_glyph_coverage_batch_stats: null pointer");
    *out = C(c)->glyph_coverage_batch_stats();
  });
}
// atlas compaction (include_glyphs/figdraw_hip_atlas.h)
int fdh_compact_atlas(FdhContext* c, int size, FdhAtlasMoveStats* out) { return guard([&] { C(c)->compact_atlas(size, out); }); }
int fdh_set_atlas_keep(FdhContext* c, int on) { return guard([&] { C(c)->set_atlas_keep(on != 0); }); }
int fdh_get_atlas_keep(FdhContext* c, int* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "fdh_get_atlas_keep: null pointer");
    *out = C(c)->atlas_keep() ? 1 : 0;
  });
}
int fdh_image_rect(FdhContext* c, int64_t key, int out_rect[4]) {
  return guard([&] {
    if (!out_rect) throw fdh::Error(FDH_ERR_INVALID, "fdh_image_rect: null pointer");
    C(c)->image_rect(key, out_rect);
  });
}
int fdh_atlas_usage(FdhContext* c, FdhAtlasUsage* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "fdh_atlas_usage: null pointer");
    C(c)->atlas_usage(out);
  });
}
int fdh_debug_read_atlas_level(FdhContext* c, int level, uint8_t* out, int64_t capacity_bytes) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "fdh_debug_read_atlas_level: null output buffer");
    C(c)->debug_read_atlas_level(level, out, capacity_bytes);
  });
}
int fdh_has_image(FdhContext* c, int64_t key, int* out) { return guard([&] { *out = C(c)->has_image(key) ? 1 : 0; }); }
int fdh_reset_atlas(FdhContext* c, int minimum_size) { return guard([&] { C(c)->reset_atlas(minimum_size); }); }
int fdh_atlas_size(FdhContext* c, int* out) { return guard([&] { *out = C(c)->atlas_size(); }); }
int fdh_atlas_packed_area(FdhContext* c, int64_t* out) { return guard([&] { *out = C(c)->atlas_packed_area(); }); }

int fdh_read_pixels(FdhContext* c, int x, int y, int w, int h, uint8_t* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "null output buffer");
    C(c)->read_pixels(x, y, w, h, out);
  });
}
int fdh_frame_device_ptr(FdhContext* c, void** p, int* w, int* h, int64_t* pitch) {
  return guard([&] { C(c)->frame_device_ptr(p, w, h, pitch); });
}
int fdh_record_begin(FdhContext* c) { return guard([&] { C(c)->record_begin(); }); }
const char* fdh_record_json(FdhContext* c) {
  const char* out = "[]";
  guard([&] { out = C(c)->record_json(); });
  return out;
}
int fdh_debug_read_surface(FdhContext* c, int which, uint8_t* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "null output buffer");
    C(c)->debug_read_surface(which, out);
  });
}
int fdh_sync(FdhContext* c) { return guard([&] { C(c)->sync(); }); }
int fdh_flush(FdhContext* c) { return guard([&] { C(c)->flush(); }); }
int fdh_set_ui_scale(FdhContext* c, float s) { return guard([&] { C(c)->set_ui_scale(s); }); }
int fdh_render_frame(FdhContext* c, const FdhScene* scene, float fw, float fh, int clear, const float rgba[4]) {
  return guard([&] {
    const float white[4] = {1, 1, 1, 1};
    C(c)->render_frame(scene, fw, fh, clear != 0, rgba ? rgba : white);
  });
}
int fdh_scene_retain(FdhContext* c, const FdhScene* scene, float fw, float fh, int clear, const float rgba[4]) {
  return guard([&] {
    const float white[4] = {1, 1, 1, 1};
    C(c)->scene_retain(scene, fw, fh, clear != 0, rgba ? rgba : white);
  });
}
int fdh_scene_update_nodes(FdhContext* c, int layer, int first, int count, const FdhFig* nodes, const FdhScene* side) {
  return guard([&] { C(c)->scene_update_nodes(layer, first, count, nodes, side); });
}
int fdh_scene_replace_root(FdhContext* c, int layer, int slot, const FdhFig* subtree, int n, const FdhScene* side) {
  return guard([&] { C(c)->scene_replace_root(layer, slot, subtree, n, side, false); });
}
int fdh_scene_insert_root(FdhContext* c, int layer, int slot, const FdhFig* subtree, int n, const FdhScene* side) {
  return guard([&] { C(c)->scene_replace_root(layer, slot, subtree, n, side, true); });
}
int fdh_scene_render(FdhContext* c) { return guard([&] { C(c)->scene_render(); }); }
int fdh_last_upload_bytes(FdhContext* c, int64_t* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "null output");
    *out = C(c)->uploaded_bytes();
  });
}
int fdh_scene_stats(FdhContext* c, int64_t* walked, int64_t* reused) {
  return guard([&] {
    if (!walked || !reused) throw fdh::Error(FDH_ERR_INVALID, "null output");
    C(c)->scene_stats(walked, reused);
  });
}
int fdh_debug_record_digest(FdhContext* c, uint64_t* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "null output");
    *out = C(c)->record_digest();
  });
}
int fdh_debug_verify_upload(FdhContext* c, uint32_t out[24]) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "null output");
    C(c)->debug_verify_upload(out);
  });
}
int fdh_debug_staging_store_bytes(int device, int64_t* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "null output");
    *out = (int64_t)fdh::vram_store_bytes(device);
  });
}
int fdh_debug_bin_digest(FdhContext* c, uint64_t out[8]) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "null output");
    C(c)->debug_bin_digest(out);
  });
}
int fdh_stripe_rows(int height, int world, int rank, int* y0, int* y1) {
  return guard([&] {
    if (!y0 || !y1) throw fdh::Error(FDH_ERR_INVALID, "null output");
    fdh::stripe_rows(height, world, rank, y0, y1);
  });
}
int fdh_comm_unique_id(uint8_t out[FDH_COMM_ID_BYTES]) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "null output");
    fdh::comm_unique_id(out);
  });
}
int fdh_comm_init(FdhContext* c, const uint8_t id[FDH_COMM_ID_BYTES], int rank, int world) {
  return guard([&] {
    if (!id) throw fdh::Error(FDH_ERR_INVALID, "null communicator id");
    C(c)->comm_init(id, rank, world);
  });
}
int fdh_comm_info(FdhContext* c, int* rank, int* world) {
  return guard([&] {
    if (!rank || !world) throw fdh::Error(FDH_ERR_INVALID, "null output");
    C(c)->comm_info(rank, world);
  });
}
int fdh_comm_share(FdhContext* c, FdhContext* owner) { return guard([&] { C(c)->comm_share(C(owner)); }); }
int fdh_comm_destroy(FdhContext* c) { return guard([&] { C(c)->comm_destroy(); }); }
int fdh_gather_stripes(FdhContext* c, int dst_rank, void* dst_image) { return guard([&] { C(c)->gather_stripes(dst_rank, dst_image); }); }
int fdh_gather_frames(FdhContext* c, int dst_rank, void* const* dst_images) { return guard([&] { C(c)->gather_frames(dst_rank, dst_images); }); }
int fdh_set_blur_route(FdhContext* c, int route) { return guard([&] { C(c)->set_blur_route(route); }); }
int fdh_set_stripe(FdhContext* c, int y0, int y1) { return guard([&] { C(c)->set_stripe(y0, y1); }); }
int fdh_set_damage_tracking(FdhContext* c, int on) { return guard([&] { C(c)->set_damage_tracking(on != 0); }); }
// picking (include/figdraw_hip_pick.h)
static_assert(sizeof(FdhPickHit) == 16, "FdhPickHit is 16 bytes");
int fdh_set_pick(FdhContext* c, int on) { return guard([&] { C(c)->set_pick(on != 0); }); }
int fdh_set_pick_tag(FdhContext* c, int32_t zlevel, int32_t id) { return guard([&] { C(c)->set_pick_tag(zlevel, id); }); }
int fdh_pick_points(FdhContext* c, const float* xy, int n, int threshold, uint32_t flags, int max_hits, FdhPickHit* out, int* counts) {
  return guard([&] { C(c)->pick_points(xy, n, threshold, flags, max_hits, out, counts); });
}
int fdh_pick_region(FdhContext* c, int x, int y, int w, int h, int threshold, uint32_t flags, int32_t* out_draw) {
  return guard([&] { C(c)->pick_region(x, y, w, h, threshold, flags, out_draw); });
}
int fdh_pick_draw_tags(FdhContext* c, int32_t* zlevels, int32_t* ids, int cap, int* n) {
  return guard([&] { C(c)->pick_draw_tags(zlevels, ids, cap, n); });
}
int fdh_damage_bins(FdhContext* c, uint8_t* mask, int cap, int* bins_x, int* bins_y, int* n_damaged) {
  return guard([&] { C(c)->damage_bins(mask, cap, bins_x, bins_y, n_damaged, false); });
}
int fdh_damage_changed_bins(FdhContext* c, uint8_t* mask, int cap, int* bins_x, int* bins_y, int* n_changed) {
  return guard([&] { C(c)->damage_bins(mask, cap, bins_x, bins_y, n_changed, true); });
}
int fdh_damage_closure(const uint8_t* changed, int bins_x, int bins_y, const int* rects, const float* radii, int n_nodes, uint8_t* out) {
  return guard([&] { fdh::damage_closure(changed, bins_x, bins_y, rects, radii, n_nodes, out); });
}
// damage readback (include/figdraw_hip_readback.h)
static_assert(sizeof(FdhDamageTile) == 16 && FDH_TILE_PITCH == FDH_TILE_PX * 4 && FDH_TILE_BYTES == FDH_TILE_PX * FDH_TILE_PITCH, "a tile is 64 rows of 256 bytes");
int fdh_set_damage_readback(FdhContext* c, int on) { return guard([&] { C(c)->set_damage_readback(on != 0); }); }
int fdh_read_damage(FdhContext* c, const FdhDamageTile** tiles, const uint8_t** pixels, int* n_tiles, int* frame_w, int* frame_h, int* full) {
  return guard([&] { C(c)->read_damage(tiles, pixels, n_tiles, frame_w, frame_h, full); });
}
int fdh_read_damage_into(FdhContext* c, uint8_t* image_rgba8, int64_t pitch_bytes, int w, int h, int* n_tiles) {
  return guard([&] { C(c)->read_damage_into(image_rgba8, pitch_bytes, w, h, n_tiles); });
}
int fdh_apply_damage(uint8_t* image_rgba8, int64_t pitch_bytes, int w, int h, const FdhDamageTile* tiles, const uint8_t* pixels, int n_tiles) {
  return guard([&] { fdh::apply_damage(image_rgba8, pitch_bytes, w, h, tiles, pixels, n_tiles); });
}
// coded damage readback (include/figdraw_hip_stream.h)
static_assert(sizeof(FdhCodedTile) == 24, "a directory entry is 24 bytes");
int fdh_read_damage_coded(FdhContext* c, const FdhCodedTile** tiles, const uint8_t** payload, int* n_tiles, int64_t* payload_bytes, int* frame_w,
                          int* frame_h, int* full) {
  return guard([&] { C(c)->read_damage_coded(tiles, payload, n_tiles, payload_bytes, frame_w, frame_h, full); });
}
int fdh_decode_damage(uint8_t* image_rgba8, int64_t pitch_bytes, int w, int h, const FdhCodedTile* tiles, int n_tiles, const uint8_t* payload,
                      int64_t payload_bytes) {
  return guard([&] { fdh::decode_damage(image_rgba8, pitch_bytes, w, h, tiles, n_tiles, payload, payload_bytes); });
}
int64_t fdh_coded_damage_bound(int w, int h) { return fdh::coded_damage_bound(w, h); }
// exact damage readback (include/figdraw_hip_exact.h)
int fdh_set_damage_exact(FdhContext* c, int on) { return guard([&] { C(c)->set_damage_exact(on != 0); }); }
int fdh_damage_exact_stats(FdhContext* c, int* n_pending, int* n_changed, int* fresh) {
  return guard([&] { C(c)->damage_exact_stats(n_pending, n_changed, fresh); });
}
int fdh_read_damage_moved(FdhContext* c, const FdhDamageMove* moves, int n_moves, const FdhCodedTile** tiles, const uint8_t** payload, int* n_tiles,
                          int64_t* payload_bytes, int* frame_w, int* frame_h, int* full, int* n_copied) {
  return guard([&] { C(c)->read_damage_moved(moves, n_moves, tiles, payload, n_tiles, payload_bytes, frame_w, frame_h, full, n_copied); });
}
int fdh_decode_damage_moved(uint8_t* image_rgba8, int64_t pitch_bytes, int w, int h, const FdhCodedTile* tiles, int n_tiles, const uint8_t* payload,
                            int64_t payload_bytes) {
  return guard([&] { fdh::decode_damage_moved(image_rgba8, pitch_bytes, w, h, tiles, n_tiles, payload, payload_bytes); });
}
int fdh_find_damage_moves(FdhContext* c, int max_shift, FdhDamageMove* out_moves, int* out_votes, int cap, int* n_out) {
  return guard([&] { C(c)->find_damage_moves(max_shift, out_moves, out_votes, cap, n_out); });
}
int fdh_set_cull(FdhContext* c, int mode) { return guard([&] { C(c)->set_cull(mode); }); }
int fdh_debug_host_times(FdhContext* c, int64_t out_ns[12]) {
  return guard([&] {
    if (!out_ns) throw fdh::Error(FDH_ERR_INVALID, "null output");
    for (int i = 0; i < 12; i++) out_ns[i] = C(c)->host_ns_[i];
  });
}
int fdh_set_walk_threads(FdhContext* c, int n) { return guard([&] { C(c)->set_walk_threads(n); }); }
int fdh_walk_stats(FdhContext* c, int* threads, int64_t* parallel_groups) {
  return guard([&] {
    if (threads) *threads = C(c)->walk_threads();
    if (parallel_groups) *parallel_groups = C(c)->parallel_groups();
  });
}
int fdh_culled_draws(FdhContext* c, int64_t* out) {
  return guard([&] {
    if (!out) throw fdh::Error(FDH_ERR_INVALID, "null output");
    *out = C(c)->culled_draws();
  });
}
int fdh_replay(FdhContext* c, int times) { return guard([&] { C(c)->replay(times); }); }
int fdh_replay_async(FdhContext* c, int times) { return guard([&] { C(c)->replay_async(times); }); }
int fdh_replay_timed(FdhContext* c, int times, float* ms_out) { return guard([&] { C(c)->replay_timed(times, ms_out); }); }
int fdh_profile(FdhContext* c, int times) { return guard([&] { C(c)->profile(times); }); }
int fdh_get_frame_stats(FdhContext* c, FdhFrameStats* out) { return guard([&] { C(c)->frame_stats(out); }); }
int fdh_block_wave_bins(FdhContext* c, int* out) { return guard([&] { *out = C(c)->block_wave_bins(); }); }

}  // extern "C"
