/* figdraw_hip_cubic_batch.h -- the two glyph batches for outlines with CUBIC Bezier segments, for libfigdraw_hip.so: what
 * fdh_put_glyph_outlines (figdraw_hip_glyphs.h) and fdh_put_glyph_coverage_batch (figdraw_hip_coverage.h) are to fdh_put_glyph_outline,
 * these two calls are to fdh_put_glyph_outline_cubic (figdraw_hip_cubic.h, whose comment is the specification of the texels).  Same
 * conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says why).  The header lives in
 * include_glyphs/ beside the three it builds on and reaches them by their relative paths: -I include_glyphs is all a caller adds.
 *
 * Why.  An application that fills an atlas from an OpenType/CFF font pays, per glyph, one copy, one or two launches of a few waves, the
 * launches of a level chain and a synchronise.  The batches took that away for TrueType outlines; these take it away for cubic ones.
 *
 * Segments.  Both calls take FdhGlyphOutline as it is (same layout; fdh_sizeof_glyph_outline covers it), but `segs` is n_segs x 8 floats
 * {x0, y0, c1x, c1y, c2x, c2y, x1, y1}, the format of fdh_put_glyph_outline_cubic: c2x NaN: a quadratic with control point (c1x, c1y);
 * c1x NaN: a line.
 *
 * fdh_put_glyph_outlines_cubic.  After the call the context is what the n calls
 *   fdh_put_glyph_outline_cubic(ctx, glyphs[i].key, glyphs[i].width, glyphs[i].height, glyphs[i].segs, glyphs[i].n_segs,
 *                               (flags without its range) | FDH_GLYPH_SDF_RANGE(range of glyph i), out_rects[i])  i = 0 .. n - 1
 * would have left, byte for byte: the directory, the packer, out_rects, the atlas size and every level of the atlas.  The range of glyph
 * i is figdraw_hip_glyphs.h's: glyphs[i].sdf_range, or, where that is 0, the range in `flags` (whose 0 is 4).  The two differences of
 * fdh_put_glyph_outlines carry over word for word:
 * 1. Everything is validated before anything is placed: the flags, n_glyphs < 0, n_glyphs > 0 with glyphs == NULL, every size (1..4096),
 *    every range (at most 64), every outline (n_segs in 0..65535, segs != NULL where n_segs > 0, closed contours by the cubic rules) and
 *    the batch limits below.  One bad glyph refuses the whole call with FDH_ERR_INVALID: no entry is made, the epoch does not move, no
 *    texel is written, and the figures of both stats calls stay those of the calls before.  n_glyphs == 0 is FDH_OK and does nothing.
 * 2. All glyphs are placed first, in order, and then the texels are made.  A placement that grows the atlas drops every entry, as it
 *    does between single calls; the glyphs placed before the batch's LAST growth are therefore not written: their entries are gone,
 *    their out_rects are filled (with the place they had for a while), and `dropped_by_growth` counts them.  All later glyphs are written,
 *    and the atlas is the one single calls leave.  FDH_ERR_ATLAS_FULL at glyph i: the glyphs before i are in the atlas with their texels,
 *    as after single calls, and the error is returned.
 * flags must hold FDH_GLYPH_MTSDF and may hold FDH_GLYPH_MTSDF_CORRECT and FDH_GLYPH_SDF_RANGE(R); they apply to every glyph.  The LCD
 * flags and unknown bits: FDH_ERR_INVALID.  FDH_GLYPH_MTSDF_OVERLAP is accepted only where NO glyph of the batch holds a cubic (a segment
 * with c1x and c2x both numbers); a cubic in any glyph refuses the whole batch, as the single call refuses the glyph.  out_rects may be NULL.
 * Batch limits, each FDH_ERR_INVALID: n_glyphs <= 65535; the sum of width * height <= 2^24 texels; the sum of n_segs <= 2^20.
 * A batch in which no glyph holds a cubic IS fdh_put_glyph_outlines on six-float copies of the same segments, with every flag that call
 * takes.  In a batch that holds one, a glyph without a cubic still gets the bytes fdh_put_glyph_outline gives it: its edges are lines and
 * quadratics, and those run the same expressions in either kernel.
 *
 * fdh_put_glyph_coverage_batch_cubic.  The same sentence, with fdh_put_glyph_outline_cubic without FDH_GLYPH_MTSDF as the single call and
 * `flags` passed as they are: FDH_GLYPH_LCD_FILTER and FDH_GLYPH_LCD_CONTEXT only (FDH_GLYPH_LCD_CONTEXT: filter iff
 * fdh_set_text_lcd_filtering is on), anything else FDH_ERR_INVALID, and so is a glyph whose sdf_range is not 0.  The two differences are
 * the same two.  Batch limits, those of fdh_put_glyph_coverage_batch: n_glyphs <= 65535; the sum of width * height <= 2^24 texels; the
 * sum of n_segs <= 2^20; the sum of flattened lines <= 2^22.  The lines are the single cubic call's: a line is one, a quadratic 1..64
 * chords by fdh_put_glyph_outline's formula, a cubic k = ceil(sqrt(30 dev)) uniform chords, 1 <= k <= 256 (figdraw_hip_cubic.h).  A glyph
 * 1 texel wide or high is placed and gets no texel, as from the single call.
 *
 * Stats.  fdh_glyph_batch_stats (figdraw_hip_glyphs.h) reports the context's last batch of distance fields and
 * fdh_glyph_coverage_batch_stats (figdraw_hip_coverage.h) its last batch of coverage glyphs, in EITHER segment format: each of the two
 * calls here writes the figures its six-float sibling writes (edges: edge records, or flattened lines).  A refused call leaves both.
 *
 * A record-only context packs the rectangles, makes no texels and reports launches = 0.
 *
 * Stream.  Each call waits for the context's submit thread like every put, works on the context's stream and synchronises once, at its
 * end: the caller's arrays are free when it returns.
 *
 * On the device.  Distance fields: the host builds every glyph's contours, orientation and colours by the cubic rules and one record of
 * 36 floats per edge (lines, quadratics and cubics alike); the records of all glyphs and the batch's table go over in one copy each; one
 * launch generates all fields (k_msdf_generate_cubic_batch), one corrects them with FDH_GLYPH_MTSDF_CORRECT (k_msdf_correct_cubic_batch)
 * -- the per-texel code is the single cubic call's, compiled from the same source --, and every level of the atlas takes one blit and one
 * minify for all glyphs: 1 or 2, plus 2 * levels - 1 launches, whatever n_glyphs is.  Coverage: the host flattens, and the launches are
 * fdh_put_glyph_coverage_batch's (2 or 3, plus 2 * levels - 1); there is no kernel of its own.
 * Out of scope: FDH_GLYPH_MTSDF_OVERLAP together with a cubic. */
#ifndef FIGDRAW_HIP_CUBIC_BATCH_H
#define FIGDRAW_HIP_CUBIC_BATCH_H
#include "figdraw_hip_coverage.h"
#include "figdraw_hip_cubic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* glyphs[i].segs: n_segs x 8 floats.  out_rects: n_glyphs x {x, y, width, height}, or NULL.  Figures: fdh_glyph_batch_stats. */
FDH_API int fdh_put_glyph_outlines_cubic(FdhContext*, const FdhGlyphOutline* glyphs, int n_glyphs, uint32_t flags, int (*out_rects)[4]);
/* glyphs[i].segs: n_segs x 8 floats; glyphs[i].sdf_range must be 0.  Figures: fdh_glyph_coverage_batch_stats. */
FDH_API int fdh_put_glyph_coverage_batch_cubic(FdhContext*, const FdhGlyphOutline* glyphs, int n_glyphs, uint32_t flags, int (*out_rects)[4]);

#ifdef __cplusplus
}
#endif
#endif
