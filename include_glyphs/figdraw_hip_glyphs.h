/* figdraw_hip_glyphs.h -- a batch of distance-field glyphs in one call for libfigdraw_hip.so: fdh_put_glyph_outline with FDH_GLYPH_MTSDF
 * (figdraw_hip.h, the comment at that flag, is the specification of the texels) for many outlines at once.  Same conventions as
 * figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says why).  No counterpart in the reference.
 * The header lives in include_glyphs/, beside include/: the set of headers in include/ is pinned (tests/test_damage_exact_host.py lists it),
 * and this one reaches figdraw_hip.h by its relative path, so -I include_glyphs is all a caller adds.
 *
 * Why.  A single put makes one field, with one copy, one or two launches of a few waves, the launches of its level chain and a
 * synchronise: on a small glyph the device is idle almost throughout, and an application that fills an atlas with a font pays that once
 * per glyph.  The batch is one copy, a number of launches that does not depend on the number of glyphs, and one synchronise.
 *
 * The contract.  After fdh_put_glyph_outlines(ctx, glyphs, n, flags, out_rects) the context is what the n calls
 *   fdh_put_glyph_outline(ctx, glyphs[i].key, glyphs[i].width, glyphs[i].height, glyphs[i].segs, glyphs[i].n_segs,
 *                         (flags without its range) | FDH_GLYPH_SDF_RANGE(range of glyph i), out_rects[i])        i = 0 .. n - 1
 * would have left, byte for byte: the directory, the packer, out_rects, the atlas size and every level of the atlas.  The range of glyph
 * i is glyphs[i].sdf_range, or, where that is 0, the range in `flags` (whose 0 is 4).  Two differences:
 * 1. Everything is validated before anything is placed: the flags, n_glyphs < 0, n_glyphs > 0 with glyphs == NULL, every size (1..4096),
 *    every range (at most 64), every outline (n_segs in 0..65535, segs != NULL where n_segs > 0, closed contours) and the batch limits
 *    below.  One bad glyph refuses the whole call with FDH_ERR_INVALID: no entry is made, the epoch does not move, no texel is written.
 *    n_glyphs == 0 is FDH_OK and does nothing.
 * 2. All glyphs are placed first, in order, and then the texels are made.  A placement that grows the atlas drops every entry, as it
 *    does between single calls; the glyphs placed before the batch's LAST growth are therefore not written: their entries are gone,
 *    their out_rects are filled (with the place they had for a while), and `dropped_by_growth` counts them.  All later glyphs are written,
 *    and the atlas is the one single calls leave.  FDH_ERR_ATLAS_FULL at glyph i: the glyphs before i are in the atlas with their texels,
 *    as after single calls, and the error is returned.
 * flags must hold FDH_GLYPH_MTSDF and may hold FDH_GLYPH_MTSDF_CORRECT, FDH_GLYPH_MTSDF_OVERLAP and FDH_GLYPH_SDF_RANGE(R); they
 * apply to every glyph.  Coverage glyphs and the LCD flags are not batched: FDH_ERR_INVALID.  out_rects may be NULL.
 *
 * Batch limits, each FDH_ERR_INVALID: n_glyphs <= 65535; the sum of width * height <= 2^24 texels; the sum of n_segs <= 2^20.
 *
 * A record-only context packs the rectangles, makes no texels and reports launches = 0.
 *
 * Stream.  The call waits for the context's submit thread like every put, works on the context's stream and synchronises once, at its
 * end: the caller's arrays are free when it returns.
 *
 * On the device.  The edge records of all glyphs and a table (one record per glyph, one word per 8 x 8 tile naming its glyph) go over in
 * one copy each.  Then one launch generates all fields (k_msdf_generate_batch, with FDH_GLYPH_MTSDF_OVERLAP k_msdf_generate_union_batch),
 * one corrects them with FDH_GLYPH_MTSDF_CORRECT (k_msdf_correct_batch, k_msdf_correct_union_batch) -- the per-texel code is the single
 * call's, compiled from the same source --, and every level of the atlas takes one blit and one minify for all glyphs
 * (k_atlas_blit_batch, k_minify2_batch; the last level has no minify): 1 or 2, plus 2 * levels - 1 launches, whatever n_glyphs is.
 * Where the rectangles of two glyphs meet in a deep level of the chain -- from level 4 on they can -- the texel is the later glyph's, as
 * after single calls. */
#ifndef FIGDRAW_HIP_GLYPHS_H
#define FIGDRAW_HIP_GLYPHS_H
#include "../include/figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct FdhGlyphOutline {
  int64_t key;
  const float* segs;      /* n_segs x 6 floats, the format of fdh_put_glyph_outline */
  int32_t n_segs;
  int32_t width, height;
  uint32_t sdf_range;     /* 1..64; 0 = the range in `flags` (whose 0 = 4) */
} FdhGlyphOutline;

typedef struct FdhGlyphBatchStats {   /* of the context's last fdh_put_glyph_outlines */
  int32_t glyphs, written, dropped_by_growth;
  int32_t tiles, edges, launches;     /* kernel launches enqueued by the call */
  int64_t bytes_copied;               /* host -> device */
} FdhGlyphBatchStats;

/* out_rects: n_glyphs x {x, y, width, height}, or NULL. */
FDH_API int fdh_put_glyph_outlines(FdhContext*, const FdhGlyphOutline* glyphs, int n_glyphs, uint32_t flags, int (*out_rects)[4]);
/* What the context's last fdh_put_glyph_outlines that passed validation did (glyphs = 0 .. for a call with n_glyphs = 0; tiles, edges:
 * of the glyphs that were written).  All zero before the first one.  A refused call leaves the figures of the call before it. */
FDH_API int fdh_glyph_batch_stats(FdhContext*, FdhGlyphBatchStats* out);
/* sizeof(FdhGlyphOutline) as the library was built, for bindings that lay the array out themselves */
FDH_API int fdh_sizeof_glyph_outline(void);

#ifdef __cplusplus
}
#endif
#endif
