/* figdraw_hip_pick.h -- exact hit testing ("picking") for libfigdraw_hip.so: which draw, and which scene node, owns a pixel of the last
 * submitted frame.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says
 * why).  The reference answers the question on the CPU from axis-aligned clipped bounds (debugtools.nim hitsAtPoint / topFigAtPoint /
 * figVisibility, `approximate` whenever corners, rotations, clips or partial cover matter); here the answer comes from the
 * compositor's own per-pixel arithmetic, on the GPU.
 *
 * Pixel.  A query point (x, y), in pixels of the frame surface, names the pixel (floor x, floor y), evaluated at its centre as the
 * compositor does.  Points outside the frame get no hits and no error.
 *
 * Effective alpha of a draw at a pixel, a: exactly the source alpha the compositor blends that draw with there -- the shape or texel
 * coverage, times the fill or vertex-colour alpha, times the open clip-mask value (the clip stack stores q8(a * a) per level), times
 * the open rect-mask value.  A backdrop-blur composite (mode 17) counts its shape coverage times the masks: the blurred backdrop's own
 * alpha does not count.  Clip-mask push / pop records and rect-mask begin / end records are never hits: they only change the mask
 * values of the draws that follow.
 *
 * Hit.  A draw hits the pixel when rint(255 a) >= threshold (1..255; the Python binding defaults to 128).  Drop and inset shadows
 * (modes 7 - 10) are not hits unless FDH_PICK_SHADOWS is passed.  Hits are listed front to back: reverse painter's order over every
 * phase of the frame.  FdhPickHit::draw is the record's index among the frame's records in painter's order -- the index
 * fdh_pick_draw_tags reports its tag under.
 *
 * Tags.  Every record carries a tag, two int32 values (zlevel, id).  In frames built by fdh_render_frame and fdh_scene_render the
 * front-end sets it to (the layer's zlevel, the index of the node whose stage issued the draw): that node owns all of its draws --
 * fill, stroke, shadows, glyph quads, image quads, curve spans, the blur composite -- and the clip / rect-mask records it opens.  In
 * a retained scene, id is the node's index in the retained layer as it stands after the latest edit (the index
 * fdh_scene_update_nodes takes).  In call-level frames the application sets the tag with fdh_set_pick_tag; it applies to the draw
 * calls that follow, and fdh_begin_frame resets it to (-1, -1).  An untagged draw still occludes whatever lies behind it.
 *
 * Which frame.  The queries describe the last submitted frame in full, whatever route it took: direct or binned, damage-tracked
 * (partial or full), with the first full-frame panel folded into the clear colour, or fdh_replay.  They wait for that frame on the
 * context's stream.
 *
 * Opt-in.  fdh_set_pick(ctx, 1) takes effect with the next frame begun; while it is off the recorder and the front-end do nothing
 * new and a frame takes exactly the path it takes without this header.  While it is on, each frame keeps its tag table (host memory)
 * until the next frame replaces it.  The queries return FDH_ERR_INVALID for a frame rendered with picking off (or before any
 * frame), and FDH_ERR_NO_DEVICE on a record-only context (FDH_CREATE_RECORD_ONLY), where fdh_set_pick, fdh_set_pick_tag and
 * fdh_pick_draw_tags still work.  Under fdh_set_stripe, a point or region row outside the stripe is FDH_ERR_INVALID. */
#ifndef FIGDRAW_HIP_PICK_H
#define FIGDRAW_HIP_PICK_H
#include "figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of fdh_pick_points / fdh_pick_region */
#define FDH_PICK_SHADOWS 1u /* drop and inset shadows (modes 7 - 10) count as hits */
#define FDH_PICK_MAX_HITS 16

/* One hit, 16 bytes: the record's tag, its index among the frame's records, rint(255 a) and its SDF mode (0 for atlas quads). */
typedef struct FdhPickHit {
  int32_t zlevel, id, draw;
  uint8_t alpha, mode;
  uint16_t reserved;
} FdhPickHit;

/* Turn picking on (on != 0) or off for this context; it takes effect with the next frame begun.  Off by default. */
FDH_API int fdh_set_pick(FdhContext*, int on);
/* The tag of the draw calls that follow (call-level frames; fdh_begin_frame resets it to (-1, -1)). */
FDH_API int fdh_set_pick_tag(FdhContext*, int32_t zlevel, int32_t id);
/* Hits at n points xy[2 i], xy[2 i + 1]: out[n][max_hits] front to back, counts[i] = hits written for point i.  max_hits in 1..16
 * (1 is topFigAtPoint; more is hitsAtPoint, front first), threshold in 1..255, flags FDH_PICK_*. */
FDH_API int fdh_pick_points(FdhContext*, const float* xy, int n, int threshold, uint32_t flags, int max_hits, FdhPickHit* out, int* counts);
/* The front-most hit's draw index for every pixel of the rectangle [x, x + w) x [y, y + h), row-major in out_draw[h][w], -1 where
 * nothing hits (pixels outside the frame: -1). */
FDH_API int fdh_pick_region(FdhContext*, int x, int y, int w, int h, int threshold, uint32_t flags, int32_t* out_draw);
/* Host only: the tag of every record of the last frame, in painter's order.  *n = the number of records; at most cap tags are
 * written (zlevels / ids may be NULL with cap = 0 to ask for the count). */
FDH_API int fdh_pick_draw_tags(FdhContext*, int32_t* zlevels, int32_t* ids, int cap, int* n);

#ifdef __cplusplus
}
#endif
#endif
