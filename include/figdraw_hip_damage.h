/* figdraw_hip_damage.h -- damage tracking ("partial redraw") for libfigdraw_hip.so: a context composites only the 64x64-pixel bins
 * whose inputs changed since its previous frame.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or a negative
 * FdhStatus, fdh_last_error() says why).  No counterpart in the reference.
 *
 * What a bin's pixels depend on: its ordered (phase, bin) draw lists, the content of every listed draw (the 128-byte record and the
 * edge functions of a rotated quad), and frame-level state -- size, clear colour, AA factor, pixel scale, atlas texels, blur route,
 * culling, and the backdrop-blur nodes whose reach covers the bin.  The bin launch's lists are signed on the GPU, per bin, and
 * compared with the previous frame's signatures: a bin whose signature matches is not composited again, its pixels are left as
 * they are.  The frame-level state is hashed on the host into one frame key.
 *
 * What still forces a full frame (every bin composited and reported):
 *   - the context's first tracked frame, and the first after a frame rendered with tracking off;
 *   - a change of the frame key: frame size or bin grid, clear colour (the first full-frame panel the host folds into it included),
 *     AA factor or pixel scale, the atlas (ANY fdh_put_image, fdh_update_image, fdh_remove_image or atlas reset since the last frame:
 *     conservative on purpose), the blur route (fdh_set_blur_route), the culling mode;
 *   - a frame that does not clear (clear_main = 0): its starting pixels are not this frame's to rebuild;
 *   - a frame with a blur node that covers the whole frame and takes the one-kernel route (k_blur_fx renders it out of place, the
 *     frame surface changes hands) -- even when nothing changed; with the two-pass route (fdh_set_blur_route(0)) such a node makes
 *     any change a full frame (the blur rule below) and an unchanged frame composites nothing;
 *   - more than 64 blur nodes, and the frame after such a frame.
 *
 * The blur rule.  A backdrop blur node with footprint F (its quad's pixel bounds) and tap reach r reads the frame as the phases
 * before it left it, over F grown by r on every side.  Outside the damage that intermediate image is not rebuilt, so when any
 * damaged bin meets the bin-rounded F (+) r, all of F (+) r becomes damage; applied until nothing grows (one node's region can reach
 * another's).  A node whose region took no damage keeps its old pixels.  A node covering the frame therefore turns any change into
 * a full frame.  fdh_damage_closure runs this rule on the host; the GPU runs the same function (one definition, compiled
 * for both sides).
 *
 * The frame surface.  Bins that are not composited keep the bytes the previous frame left, so the application must not write into
 * the surface (fdh_frame_device_ptr) between frames of a tracking context.  fdh_frame_device_ptr is right after every frame,
 * partial or full.  Blur passes still run on a partial frame (their nodes' pixels are kept where the rule leaves them).
 *
 * Contract: after any sequence of frames -- fdh_render_frame, fdh_scene_render, fdh_begin_frame .. fdh_end_frame, fdh_replay -- the
 * frame surface is bit for bit what a full render of the last frame gives. */
#ifndef FIGDRAW_HIP_DAMAGE_H
#define FIGDRAW_HIP_DAMAGE_H
#include "figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Turn damage tracking on (on != 0) or off for this context; it takes effect with the next frame submitted.  Off by default: a
 * context that never turns it on renders exactly as before.  FDH_ERR_INVALID on a record-only context (FDH_CREATE_RECORD_ONLY:
 * nothing is composited) and under fdh_set_stripe (row stripes: not supported; fdh_set_stripe refuses a stripe while tracking is
 * on).  Turning it off is always accepted. */
FDH_API int fdh_set_damage_tracking(FdhContext*, int on);
/* Which 64x64 bins the last submitted frame composited (waits for it): mask[bins_y][bins_x], row-major, one byte per bin, 1 =
 * composited (NULL: not wanted; otherwise cap >= bins_x * bins_y bytes), the bin grid in *bins_x / *bins_y and the number of
 * composited bins in *n_damaged (each may be NULL).  A frame rendered in full -- tracking off, or a full frame above -- reports every
 * bin.  An application presents or reads back only these: bin (bx, by) is the pixels [64 bx, min(64 bx + 64, W)) x [64 by,
 * min(64 by + 64, H)) -- figdraw_hip_readback.h brings exactly these to the host, packed, in one transfer, and keeps count of them
 * across frames the application did not read.  FDH_ERR_INVALID before the first frame; FDH_ERR_NO_DEVICE on a record-only context. */
FDH_API int fdh_damage_bins(FdhContext*, uint8_t* mask, int cap, int* bins_x, int* bins_y, int* n_damaged);
/* Diagnostic: the same for the bins whose signature changed, before the blur rule grew them (every bin of a full frame). */
FDH_API int fdh_damage_changed_bins(FdhContext*, uint8_t* mask, int cap, int* bins_x, int* bins_y, int* n_changed);
/* Diagnostic, host-only (no device, no context): the blur rule.  changed[bins_y][bins_x] (non-zero = changed) and n_nodes blur nodes
 * of the frame, node i's footprint rects[4 i .. 4 i + 3] = x0, y0, x1, y1 in pixels (exclusive ends) and its radius radii[i] as
 * given to fdh_draw_backdrop_blur; out[bins_y][bins_x] = 1 where the closed damage is, 0 elsewhere.  n_nodes <= 64. */
FDH_API int fdh_damage_closure(const uint8_t* changed, int bins_x, int bins_y, const int* rects, const float* radii, int n_nodes,
                               uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif
