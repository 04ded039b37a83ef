/* figdraw_hip_cubic.h -- glyph outlines with CUBIC Bezier segments for libfigdraw_hip.so: fdh_put_glyph_outline (figdraw_hip.h) for the
 * outlines of OpenType/CFF fonts, which are cubics where TrueType's are quadratics.  Same conventions as figdraw_hip.h (plain C, every
 * call returns 0 or a negative FdhStatus, fdh_last_error() says why).  The header lives in include_glyphs/ beside figdraw_hip_glyphs.h,
 * figdraw_hip_coverage.h and figdraw_hip_cubic_batch.h and reaches figdraw_hip.h by its relative path: -I include_glyphs is all a caller adds.
 *
 * Why.  fdh_put_glyph_outline takes lines and quadratics.  A caller with cubics had to flatten them, which multiplies the edges a
 * distance field walks per texel (and the call refuses more than 65535), or to approximate them by quadratics, which puts the
 * approximation's error into the field.  This call takes the cubics as they are.
 *
 * Segments.  segs is n_segs x 8 floats {x0, y0, c1x, c1y, c2x, c2y, x1, y1}, in the units and the orientation of fdh_put_glyph_outline:
 * a cubic with P0 = (x0, y0), P1 = (c1x, c1y), P2 = (c2x, c2y), P3 = (x1, y1), B(t) = (1-t)^3 P0 + 3 (1-t)^2 t P1 + 3 (1-t) t^2 P2 + t^3 P3;
 * c2x NaN: a quadratic with control point (c1x, c1y); c1x NaN: a line.  Contours closed, non-zero winding.
 *
 * Behaviour.
 * - No cubic among the segments (every segment has c1x or c2x NaN): the call IS fdh_put_glyph_outline on the same segments in its 6-float
 *   format, with every flag that call takes, FDH_GLYPH_MTSDF_OVERLAP included, and leaves the same bytes everywhere: directory, packer,
 *   out_rect, every level of the atlas.
 * - Without FDH_GLYPH_MTSDF (coverage): each cubic is flattened on the host into k uniform chords of at most 0.025 px error,
 *   k = ceil(sqrt(30 dev)), dev = max(|P0 - 2 P1 + P2|, |P1 - 2 P2 + P3|), 1 <= k <= 256 (the error of a chord is at most max |B''| / (8 k^2)
 *   and |B''| <= 6 dev: the cap of 256 is reached at dev = 0.025 * 256^2 / 0.75 = 2184.5 px, and the figure holds up to there for exact chord ends; the ends are float32 and lie up to about 1e-6 of the coordinates' size off the
 *   curve, 0.001 px at 1000, which is more than the formula's rounding up leaves below 0.025 once dev passes a few hundred px); lines and quadratics by fdh_put_glyph_outline's own formula; then that call's rasteriser and level chain, and the LCD
 *   flags mean what they mean there.
 * - With FDH_GLYPH_MTSDF: the field of figdraw_hip.h's DISTANCE FIELDS comment, steps 1 to 5, with the rules for cubic edges below;
 *   FDH_GLYPH_SDF_RANGE(R) and FDH_GLYPH_MTSDF_CORRECT are optional and mean what they mean there.  Validation is fdh_put_glyph_outline's
 *   and happens before anything is packed: sizes 1..4096, n_segs 0..65535, a range at most 64 and only with FDH_GLYPH_MTSDF, no LCD flag,
 *   FDH_GLYPH_MTSDF_CORRECT only with FDH_GLYPH_MTSDF, unknown bits, an open contour: FDH_ERR_INVALID.
 * - FDH_GLYPH_MTSDF_OVERLAP on an outline that holds a cubic: FDH_ERR_INVALID, refused before anything is packed.
 * - A record-only context packs the rectangle and makes no texels.
 * - The call waits for the context's submit thread like every put, works on the context's stream and synchronises once: the caller's
 *   array is free when it returns.
 *
 * The cubic rules.  This comment is their specification; it extends steps 1 to 5 of figdraw_hip.h and does not restate them.
 * tests/msdf_cubic_ref.py implements it in float64 and the device (figdraw_amd/csrc/fdh_msdf_cubic_host.h, k_msdf_cubic.hip) is held to
 * that within 1 LSB.  cross(u, v) = ux vy - uy vx.
 * 1. Edges (decisions in double on the float32 input, each product taken and compared on its own), in this order:
 *    A cubic whose four points are equal is dropped.
 *    A cubic whose third difference d = P3 - 3 P2 + 3 P1 - P0 has |d|^2 <= 1e-6 is the quadratic with control point
 *    (3 (P1 + P2) - (P0 + P3)) / 4, rounded to float32, and goes through step 1's quadratic rules (it may become a line there, or be dropped).
 *    A cubic with all four points on one line becomes the line P0 P3 (and that is dropped where P0 = P3): with u = P1 - P0, v = P2 - P0,
 *    w = P3 - P0, when u.x w.y = u.y w.x and v.x w.y = v.y w.x; where w = 0, when u.x v.y = u.y v.x.  Inside the chord or beyond its ends:
 *    what such a curve covers twice encloses nothing.
 *    Every other cubic is an edge; one with P0 = P3 and its control points off that line is an ordinary edge, a closed lobe.
 * 2. Orientation.  A cubic edge contributes the exact value of 1/2 of the integral of (x dy - y dx) along it:
 *    (x0 y3 - x3 y0) / 2 + (3 cross(u, v) + 3 cross(u, w) + 6 cross(v, w)) / 20, u, v, w as above, in double.
 * 3. Colours.  The tangent direction of a cubic at its start is P1 - P0; where that is zero P2 - P0; where that is zero P3 - P0.  At its
 *    end: P3 - P2, then P3 - P1, then P3 - P0.  The corner rule and the colouring are unchanged.  The one-corner contour with m < 3 splits a
 *    cubic in thirds by de Casteljau: with b(r, s, u) = lerp(lerp(lerp(P0, P1, r), lerp(P1, P2, r), s), lerp(lerp(P1, P2, r), lerp(P2, P3, r), s), u),
 *    the part [t0, t1] has the points b(t0, t0, t0), b(t0, t0, t1), b(t0, t1, t1), b(t1, t1, t1), each rounded to float32, the original ends
 *    kept as they are.  The parts are cubic edges as they stand (step 1 is not applied again).
 * 4. The nearest point of a cubic edge is the nearest point of B(t) over t in [0, 1].  The rules of step 4 carry over word for word: at
 *    t = 0 and t = 1 it is the stored end point; an interior point counts only where it is strictly nearer than both ends, and of two ends
 *    equally near it is P0; ties between edges go to the larger orthogonality; the pseudo-distance is used at ends, U step 3's unit tangent
 *    of that end.  The tangent T is B'(t) at an interior t and step 3's tangent direction at t = 0 and t = 1.  Where B'(t) = 0 at an interior
 *    nearest point (a cusp), the orthogonality is 0 and the sign is +.
 * 5. Correction.  Unchanged; d(q) takes the cubic edges by rule 4.
 * Not covered: a cubic that crosses itself, which joins "a contour that crosses itself" of figdraw_hip.h.
 * Many such outlines at once: figdraw_hip_cubic_batch.h -- fdh_put_glyph_outlines_cubic and fdh_put_glyph_coverage_batch_cubic, the two batches
 * (figdraw_hip_glyphs.h, figdraw_hip_coverage.h) for segments of 8 floats.
 * Out of scope: FDH_GLYPH_MTSDF_OVERLAP together with a cubic.
 *
 * On the device.  The host makes contours, orientation, colours and one record of 36 floats per edge; k_msdf_generate_cubic is
 * k_msdf_generate over those records (a lane per texel, a wave per 8 x 8 tile, records by scalar loads, the per-tile cull with the box of
 * the four control points).  Lines and quadratics run the expressions they run there.  A cubic's nearest parameter is a root of the quintic
 * g(t) = (B(t) - p) . B'(t): g is sampled at K + 1 uniform parameters (K per edge, 8 to 32, from the curve's turning and its change of
 * speed), every interval over which g rises through zero is refined by safeguarded Newton steps, and so is the nearest sample.
 * k_msdf_correct_cubic is k_msdf_correct likewise.  The launches are the single distance-field put's: one copy of records, generate,
 * optionally correct, the level chain. */
#ifndef FIGDRAW_HIP_CUBIC_H
#define FIGDRAW_HIP_CUBIC_H
#include "../include/figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* segs: n_segs x 8 floats (NULL where n_segs is 0); flags as for fdh_put_glyph_outline; out_rect = the packed rectangle x, y, w, h. */
FDH_API int fdh_put_glyph_outline_cubic(FdhContext*, int64_t key, int width, int height, const float* segs, int n_segs, uint32_t flags, int out_rect[4]);

#ifdef __cplusplus
}
#endif
#endif
