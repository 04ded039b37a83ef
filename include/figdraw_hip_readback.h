/* figdraw_hip_readback.h -- damage readback for libfigdraw_hip.so: fetch only the 64x64-pixel bins that changed since the application
 * last fetched, packed, in one transfer.  The host-side half of damage tracking (figdraw_hip_damage.h), which makes a context
 * composite only the bins a frame changed; this header moves only those bins to the host.  Same conventions as figdraw_hip.h (plain
 * C, every call returns 0 or a negative FdhStatus, fdh_last_error() says why).  No counterpart in the reference.
 *
 * The pending set.  While the mode is on the context keeps, on the device and in stream order, the set of bins that ANY frame
 * submitted since the last successful fdh_read_damage composited: per tracked frame the mask fdh_damage_bins reports for it (the
 * closed damage; every bin of a full frame), OR-ed in; every bin for a frame rendered with tracking off, for the first frame after
 * the mode is turned on, and after a change of frame size.  An application that skips a read loses nothing: the next read brings
 * every bin that differs from what it last received.  Every way to submit a frame feeds the set: fdh_render_frame, fdh_scene_render,
 * fdh_begin_frame .. fdh_end_frame, fdh_replay*.
 *
 * Tiles.  A read returns the pending bins as tiles, in row-major bin order (by ascending, then bx).  Tile i is bin (bx, by) clipped
 * to the frame: x = 64 bx, y = 64 by, w = min(64, W - x), h = min(64, H - y), in top-down pixels.  Its pixels live in a slot of
 * FDH_TILE_BYTES at pixels + i * FDH_TILE_BYTES: row r at + r * FDH_TILE_PITCH, 4 w bytes of RGBA8 per row; the rest of a clipped
 * tile's slot is zero.
 *
 * Memory.  The tiles and their pixels are in page-locked host memory the context owns, written by the GPU (k_damage_pack stores the
 * packed tiles straight into it: one launch, no copy command).  It is sized for the whole grid -- bins * FDH_TILE_BYTES, 33.4 MB
 * for a 3840 x 2160 frame -- when the first fdh_read_damage after the mode is turned on, or after a change of frame size, needs it;
 * fdh_set_damage_readback(ctx, 0) and fdh_destroy free it.  The CPU's loads from such memory are slower than from ordinary memory:
 * copy out of it once (fdh_apply_damage does), do not compute in it.
 *
 * The invariant: a mirror image that starts as anything and receives every fdh_read_damage_into since the mode was turned on is,
 * after each call, bit for bit what fdh_read_pixels returns for the whole frame. */
#ifndef FIGDRAW_HIP_READBACK_H
#define FIGDRAW_HIP_READBACK_H
#include "figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FDH_TILE_PX = 64, FDH_TILE_PITCH = 256, FDH_TILE_BYTES = 16384 };
typedef struct FdhDamageTile { int32_t x, y, w, h; } FdhDamageTile;   /* a bin clipped to the frame, in top-down pixels */

/* Turn damage readback on (on != 0) or off for this context.  Off by default: a context that never turns it on enqueues exactly the
 * launches it did before.  Turning it on makes every bin pending.  Independent of fdh_set_damage_tracking: with tracking off every
 * frame makes every bin pending, and a read is then a whole-frame read through page-locked memory.  FDH_ERR_INVALID on a record-only
 * context and under fdh_set_stripe when turning on (fdh_set_stripe refuses a stripe while the mode is on); turning it off is always
 * accepted, frees the host buffer and invalidates the pointers fdh_read_damage returned. */
FDH_API int fdh_set_damage_readback(FdhContext*, int on);
/* Wait for the last submitted frame (as fdh_read_pixels does), pack the pending bins out of the frame surface, bring them to the
 * host and empty the pending set.  *tiles / *pixels: n_tiles tiles as described above; *frame_w / *frame_h: the frame's size; *full:
 * 1 when every bin of the grid is in the set.  *n_tiles = 0 is a valid answer (nothing changed): nothing is launched or copied then.
 * The pointers stay valid until the next fdh_read_damage / fdh_read_damage_into on this context, fdh_set_damage_readback(ctx, 0) or
 * fdh_destroy; submitting further frames does not invalidate them.  Any out-pointer may be NULL.  FDH_ERR_NO_DEVICE on a record-only
 * context; FDH_ERR_INVALID before the first frame or while the mode is off. */
FDH_API int fdh_read_damage(FdhContext*, const FdhDamageTile** tiles, const uint8_t** pixels, int* n_tiles,
                            int* frame_w, int* frame_h, int* full);
/* fdh_read_damage, then fdh_apply_damage on the caller's mirror of the frame: a top-down RGBA8 image of w x h pixels with row pitch
 * pitch_bytes.  *n_tiles (may be NULL): how many bins were pending.  FDH_ERR_INVALID, with the pending set left as it was, when the image is
 * null, w x h is not the last frame's size or pitch_bytes < 4 w.  When three tenths of the grid or more are pending, the whole frame is
 * copied into the image in one transfer instead of tile by tile (cheaper from there on: the tiles' second pass on the CPU is saved,
 * and the host buffer is not needed); the image and *n_tiles, the number of pending bins, are the same either way. */
FDH_API int fdh_read_damage_into(FdhContext*, uint8_t* image_rgba8, int64_t pitch_bytes, int w, int h, int* n_tiles);
/* Host only (no context, no device: a receiver on another machine applies what it was sent): copy each tile's rows into a top-down
 * RGBA8 image of w x h with row pitch pitch_bytes; no other byte of the image is touched, and of a slot only the tile's w x h pixels
 * are read.  FDH_ERR_INVALID, with the image untouched, for a null image / tiles / pixels with n_tiles > 0, n_tiles < 0,
 * pitch_bytes < 4 w, or a tile with w or h outside 1 .. 64 or not inside the image. */
FDH_API int fdh_apply_damage(uint8_t* image_rgba8, int64_t pitch_bytes, int w, int h,
                             const FdhDamageTile* tiles, const uint8_t* pixels, int n_tiles);

#ifdef __cplusplus
}
#endif
#endif
