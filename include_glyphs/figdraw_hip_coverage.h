/* figdraw_hip_coverage.h -- a batch of COVERAGE glyphs in one call for libfigdraw_hip.so: fdh_put_glyph_outline without FDH_GLYPH_MTSDF
 * (figdraw_hip.h, the comment at that call, is the specification of the texels) for many outlines at once -- the reference's text path:
 * generateGlyph (common/fontglyphs.nim:61-106) makes one coverage image per glyph and, with sub-pixel variants, one per (glyph, variant),
 * with or without the LCD filter.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus,
 * fdh_last_error() says why).  The header lives in include_glyphs/ beside figdraw_hip_glyphs.h, whose FdhGlyphOutline and
 * FdhGlyphBatchStats it uses and which it reaches by its relative path: -I include_glyphs is all a caller adds.
 *
 * Why.  A single coverage put is one copy, a rasteriser launch of one wave with a lane per pixel row, perhaps the LCD filter, two small
 * launches per level of the chain and a synchronise; an application that fills an atlas with a font at one size pays that once per glyph
 * and variant.  The batch is one copy of lines, one copy of tables, a number of launches that does not depend on the number of glyphs,
 * and one synchronise.
 *
 * The contract.  After fdh_put_glyph_coverage_batch(ctx, glyphs, n, flags, out_rects) the context is what the n calls
 *   fdh_put_glyph_outline(ctx, glyphs[i].key, glyphs[i].width, glyphs[i].height, glyphs[i].segs, glyphs[i].n_segs, flags, out_rects[i])
 *                                                                                                                    i = 0 .. n - 1
 * would have left, byte for byte: the directory, the packer, out_rects, the atlas size and every level of the atlas.  (A glyph 1 texel
 * wide or high is packed and gets no texel, from a single put as from the batch: the level chain stores nothing of such an image.)
 * flags may hold FDH_GLYPH_LCD_FILTER and FDH_GLYPH_LCD_CONTEXT, for every glyph; FDH_GLYPH_LCD_CONTEXT means what it means to the
 * single put: filter iff fdh_set_text_lcd_filtering is on.  Anything else is FDH_ERR_INVALID: FDH_GLYPH_MTSDF, FDH_GLYPH_MTSDF_CORRECT,
 * FDH_GLYPH_MTSDF_OVERLAP, a range in bits 8..15, an unknown bit -- distance fields are fdh_put_glyph_outlines' -- and so is a glyph
 * whose sdf_range is not 0.  Two differences, those of figdraw_hip_glyphs.h:
 * 1. Everything is validated before anything is placed: the flags, n_glyphs < 0, n_glyphs > 0 with glyphs == NULL, every size (1..4096),
 *    every sdf_range (0), every outline (n_segs >= 0, segs != NULL where n_segs > 0) and the batch limits below.  One bad glyph refuses
 *    the whole call with FDH_ERR_INVALID: no entry is made, the epoch does not move, no texel is written, and the figures of both stats
 *    calls stay those of the calls before.  n_glyphs == 0 is FDH_OK and does nothing.
 * 2. All glyphs are placed first, in order, and then the texels are made.  A placement that grows the atlas drops every entry, as it
 *    does between single calls; the glyphs placed before the batch's LAST growth are therefore not written: their entries are gone,
 *    their out_rects are filled (with the place they had for a while), and `dropped_by_growth` counts them.  All later glyphs are
 *    written, and the atlas is the one single calls leave.  FDH_ERR_ATLAS_FULL at glyph i: the glyphs before i are in the atlas with their
 *    texels, as after single calls, and the error is returned.
 * out_rects may be NULL.
 *
 * Batch limits, each FDH_ERR_INVALID: n_glyphs <= 65535; the sum of width * height <= 2^24 texels; the sum of n_segs <= 2^20; the sum of
 * flattened lines (a straight segment is one, a curve 1..64 chords of at most 0.025 px error while |P0 - 2 C + P1| <= 409.6 px, where the
 * cap of 64 is reached) <= 2^22.
 *
 * The texels are the single put's: exact areas of the flattened outline, floor(255 c + 0.5).  The parts of an outline outside the image:
 * what lies left of it (x < 0) covers the rows to its right, what lies right of it (x > width), above or below adds nothing, also where
 * an edge crosses x = 0 or x = width inside a pixel row (figdraw_hip.h, at fdh_put_glyph_outline).
 *
 * A record-only context packs the rectangles, makes no texels and reports launches = 0.
 *
 * Stream.  The call waits for the context's submit thread like every put, works on the context's stream and synchronises once, at its
 * end: the caller's arrays are free when it returns.
 *
 * On the device.  The host flattens every outline with the single put's formula; the lines of all glyphs and a table (one record per
 * glyph, one word per 8 x 8 tile naming its glyph) go over in one copy each.  The single rasteriser scatters: a lane owns a pixel row and
 * every line adds to the accumulator cells it crosses in that row.  The batch gathers: a lane owns one cell, walks the glyph's lines in
 * the same order and adds what each line adds to that cell, the same expressions in the same order (k_coverage_cells_batch, one
 * workgroup per tile, lines that cannot reach a tile skipped for the whole tile); a second launch (k_coverage_sum_batch) carries every
 * row's running sum from left to right through the glyph's tiles, in the single rasteriser's order, and makes the texels.  One launch
 * filters all glyphs with FDH_GLYPH_LCD_FILTER (k_lcd_filter_batch), and every level of the atlas takes one blit and one minify for all
 * glyphs (k_atlas_blit_batch, k_minify2_batch; the last level has no minify): 2 or 3, plus 2 * levels - 1 launches, whatever n_glyphs
 * is.  Where the rectangles of two glyphs meet in a deep level of the chain the texel is the later glyph's, as after single calls. */
#ifndef FIGDRAW_HIP_COVERAGE_H
#define FIGDRAW_HIP_COVERAGE_H
#include "figdraw_hip_glyphs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* glyphs[i].sdf_range must be 0.  out_rects: n_glyphs x {x, y, width, height}, or NULL. */
FDH_API int fdh_put_glyph_coverage_batch(FdhContext*, const FdhGlyphOutline* glyphs, int n_glyphs, uint32_t flags, int (*out_rects)[4]);
/* What the context's last fdh_put_glyph_coverage_batch that passed validation did (glyphs = 0 .. for a call with n_glyphs = 0; tiles, and
 * edges = flattened lines: of the glyphs that were written).  All zero before the first one.  A refused call leaves the figures of the
 * call before it.  Figures of its own: fdh_glyph_batch_stats keeps reporting the last fdh_put_glyph_outlines. */
FDH_API int fdh_glyph_coverage_batch_stats(FdhContext*, FdhGlyphBatchStats* out);

#ifdef __cplusplus
}
#endif
#endif
