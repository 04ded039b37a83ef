/* figdraw_hip_image_sdf.h -- distance fields from coverage IMAGES for libfigdraw_hip.so: what fdh_put_glyph_outline with FDH_GLYPH_MTSDF
 * (figdraw_hip.h) does for an outline, for content that arrives as pixels -- a PNG icon, a nine-patch, a coverage glyph rasterised
 * elsewhere or by fdh_put_glyph_outline itself.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus,
 * fdh_last_error() says why).  The header lives in include_glyphs/ beside figdraw_hip_glyphs.h, figdraw_hip_coverage.h, figdraw_hip_cubic.h
 * and figdraw_hip_cubic_batch.h and reaches figdraw_hip.h by its relative path: -I include_glyphs is all a caller adds.
 *
 * Why.  A field made of such an image scales cleanly, and fdh_draw_msdf outlines it, emboldens it or gives it a soft glow.  Without these
 * calls an application writes its own distance transform on the CPU and uploads the result through fdh_put_image.
 *
 * This comment is the specification.  tests/image_sdf_ref.py implements it in float64 and the device (figdraw_amd/csrc/k_image_sdf.hip)
 * is held to that within 1 LSB on every texel.
 *
 * Source.  width x height RGBA8 texels.  Byte `channel` (0 .. 3; 3 = alpha) of texel q is its coverage, c_q = byte / 255: the fraction of
 * the texel's unit square that the shape covers.  For premultiplied white, as pixie and fdh_put_glyph_outline store glyphs, every channel
 * is that fraction.  Every texel of the plane outside the source has c = 0.  Let e_q = c_q - 0.5.
 *
 * Output.  An image of (width + 2 pad) x (height + 2 pad) texels with the source centred in it.  All four bytes of a texel equal the
 * encoded signed distance d, positive inside: floor(255 * clamp(0.5 + d / R, 0, 1) + 0.5).  R comes from FDH_GLYPH_SDF_RANGE(R) in `flags`:
 * 1 .. 64, 0 = 4 -- the encoding of step 4 of fdh_put_glyph_outline's DISTANCE FIELDS comment.
 * Because all four bytes are equal, fdh_draw_msdf(key, ..., px_range = R, sd_threshold = 0.5, mtsdf = 0 or 1) draws it: the median of
 * three equal channels is the channel.  A px_range below R widens the ramp into a soft glow, a threshold below 0.5 fattens the shape, the
 * stroke modes outline it.
 * The image is packed and its level chain built like any distance field's: nothing premultiplied, nothing filtered, and an image 1 texel
 * wide or high gets its level 0 as under FDH_GLYPH_MTSDF.
 *
 * Distance of output texel p, with |p - q| the Euclidean distance between texel centres (an integer lattice):
 * - if 2 c_p >= 1:  d(p) = +min over all q with c_q < 1 of (|p - q| + e_q);
 * - else:           d(p) = -min over all q with c_q > 0 of (|p - q| - e_q); where no such q exists d(p) = -infinity and the byte is 0.
 * q ranges over the whole plane, so q = p takes part: a partly covered texel can be its own nearest edge, d = e_p.  Texels outside the
 * source take part in the first rule with e = -0.5.
 * Meaning: a texel of coverage c, seen along an axis from a neighbour, has its edge c - 0.5 beyond its own centre.  The rule is exact for
 * axis-aligned edges at any sub-texel position, continuous through c = 0.5, and antisymmetric: c -> 1 - c negates d wherever the plane
 * outside the source plays no part.
 * Measured on an antialiased disc of radius 10.3 (16 x 16 supersampled, centre (20.2, 19.7), 40 x 40), over the texels whose true
 * distance is below 8, in texels:                        mean abs error   max abs error
 *   this rule                                                  0.028           0.24
 *   the squared-offset rule of TinySDF-style generators        0.25            0.64
 *   threshold at 128 plus a binary Euclidean transform         0.23            0.50
 * Not covered: a texel that two edges cross carries one number.
 *
 * What an implementation may skip.  A candidate with |p - q| > R / 2 + 0.5 has a term above R / 2 and can only produce a saturated byte:
 * the search may stop at |dx|, |dy| <= floor(R / 2 + 0.5) + 1, at most 33; the bytes equal those of an unbounded search for R = 1 .. 64.
 * Candidates on the Chebyshev ring k around p have terms >= k - 0.5.  No candidate may be skipped for being "interior": a fully covered
 * texel next to a diagonal can be the minimiser.
 *
 * Refusals.  FDH_ERR_INVALID, refused before anything is packed: width or height < 1; rgba8 NULL; channel outside 0 .. 3; pad outside
 * 0 .. 64; any bit of flags outside bits 8 .. 15; a range above 64.  An output size the atlas cannot take, an existing key, a full atlas
 * and its growth are treated exactly as fdh_put_glyph_image treats them for an image of the output's size.  A record-only context packs
 * the rectangle and makes no texels.
 *
 * fdh_put_image_sdf_of.  The source is level 0 of src_key's rectangle in the atlas as it is when the call is made; nothing crosses the
 * bus, and the call leaves, byte for byte, what fdh_put_image_sdf leaves when handed those same texels from the host.  The source
 * rectangle is copied to scratch BEFORE the new image takes its place: a placement that grows the atlas drops every earlier entry, the
 * source among them, exactly as in the reference -- the field is still made from what was there, out_rect is valid, and src_key is gone
 * like every other key.  An unknown src_key and src_key == key: FDH_ERR_INVALID.  On a record-only context the source's size comes from
 * the directory and no texels are made.
 *
 * Both calls wait for the context's submit thread like every put, work on the context's stream and synchronise once: the caller's array
 * is free when they return.
 *
 * On the device.  k_image_sdf_generate: a workgroup per 16 x 16 tile of the output, a lane per texel.  The coverage of the tile and of a
 * halo of the window's reach is staged once into LDS, as the floats e (at most 82 x 82 of them); the candidates are walked ring by ring
 * outward, and a wave leaves the walk as soon as k - 0.5 is no smaller than every lane's best, or the window ends.  A tile whose staged region is all 0
 * stores zeros without searching; one whose region is all 255 and reaches outside the source nowhere stores 255.  float32 in the form
 * written above; dx^2 + dy^2 is an exact integer. */
#ifndef FIGDRAW_HIP_IMAGE_SDF_H
#define FIGDRAW_HIP_IMAGE_SDF_H
#include "../include/figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rgba8: width x height x 4 bytes, rows packed; flags: FDH_GLYPH_SDF_RANGE(R) or 0; out_rect = the packed rectangle x, y, w, h of the
 * (width + 2 pad) x (height + 2 pad) field (may be NULL). */
FDH_API int fdh_put_image_sdf(FdhContext*, int64_t key, int width, int height, const uint8_t* rgba8, int channel, int pad, uint32_t flags, int out_rect[4]);
/* the same of the texels that src_key holds in the atlas */
FDH_API int fdh_put_image_sdf_of(FdhContext*, int64_t src_key, int64_t key, int channel, int pad, uint32_t flags, int out_rect[4]);

#ifdef __cplusplus
}
#endif
#endif
