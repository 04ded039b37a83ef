/* figdraw_hip_exact.h -- exact damage readback for libfigdraw_hip.so: a sub-mode of damage readback (figdraw_hip_readback.h,
 * figdraw_hip_stream.h) in which a read returns only the bins whose PIXELS changed since the application last read, not every bin
 * whose inputs changed.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says
 * why).  No counterpart in the reference.
 *
 * Why.  The pending set of figdraw_hip_readback.h is a set of bins that some frame composited: a superset of the bins whose pixels
 * differ from what the application holds.  Every bin of a frame rendered with tracking off, of a tracked frame that is rendered in full
 * (figdraw_hip_damage.h lists the causes) and of a blur node's whole footprint is in it whatever happened to its pixels; so is a bin
 * whose draw moved under opaque siblings, or whose edit was undone before the next read.
 *
 * The mode.  While it is on (and damage readback is on) the context keeps a device mirror of the frame as of the application's last
 * read.  Every read -- fdh_read_damage, fdh_read_damage_into, fdh_read_damage_coded alike -- first runs one launch over the pending
 * bins (k_damage_filter): a bin whose tile is byte for byte the mirror's leaves the pending set; a bin that differs stays, and the
 * mirror takes its pixels.  The read then packs or codes the bins that are left, as it does with the mode off: the tiles, their
 * order, the slots, the coded format and the lifetime of the returned pointers are those of the two headers above.  *n_tiles (and the
 * count fdh_read_damage_into reports, and the one its three-tenths rule weighs) is the number of bins that are left; *full is 1 when
 * that is every bin of the grid.
 *
 * The invariant, on top of the one of figdraw_hip_readback.h: after every read the device mirror is bit for bit what fdh_read_pixels
 * returns for the whole frame, and -- apart from a fresh read -- the tiles of a read are EXACTLY the bins in which the frame differs
 * from what the application held before it: no more, no fewer, in row-major bin order.  An unchanged frame reads as 0 tiles, tracked
 * or not.
 *
 * The fresh read.  The mirror is invalid after the mode is turned on, after damage readback is turned on, after a change of frame
 * size and after a read that failed.  The first read with a pending bin after that is a fresh one: the pending set passes unfiltered
 * -- the tiles are what the read would return with the mode off, never more -- and the mirror is filled from the whole surface in one
 * device-to-device launch.
 *
 * Memory.  One more device buffer of the grid's size, bins * 16384 bytes (33.4 MB for a 3840 x 2160 frame), allocated by the first
 * read that needs it and freed by fdh_set_damage_exact(ctx, 0), fdh_set_damage_readback(ctx, 0) and fdh_destroy.
 *
 * Errors.  A read that fails after the filter ran (the mirror then holds tiles the application never received) invalidates the mirror
 * and makes every bin pending: the next read is a fresh one that returns every bin, so a lost read is never mistaken for a delivered
 * one.  A read that is refused before anything is launched (FDH_ERR_INVALID of fdh_read_damage_into for its image, of
 * fdh_read_damage_coded for the frame's size) leaves the pending set and the mirror as they were.
 *
 * Cost.  With the mode off a context enqueues exactly what it does without this header.  With it on, a read that is not fresh adds
 * one launch that reads the pending tiles from the surface and from the mirror and writes those that differ, and one synchronise. */
#ifndef FIGDRAW_HIP_EXACT_H
#define FIGDRAW_HIP_EXACT_H
#include "figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Turn exact damage readback on (on != 0) or off for this context.  Off by default.  May be called while damage readback is on or
 * off; it acts while damage readback is on, and the setting survives fdh_set_damage_readback(ctx, 0).  Turning it on invalidates the
 * mirror (so does turning damage readback on); turning it on while it is on resets nothing.  Turning it off frees the mirror and is
 * always accepted.  FDH_ERR_INVALID on a record-only context when turning on. */
FDH_API int fdh_set_damage_exact(FdhContext*, int on);
/* The last read of any of the three kinds made with the mode on: *n_pending, the bins that were pending before the filter;
 * *n_changed, the bins it kept (the read's tiles; = *n_pending on a fresh read); *fresh, 1 when the read was a fresh one.  Any
 * out-pointer may be NULL.  FDH_ERR_INVALID before the first such read since the mode, or damage readback, was turned on. */
FDH_API int fdh_damage_exact_stats(FdhContext*, int* n_pending, int* n_changed, int* fresh);

#ifdef __cplusplus
}
#endif
#endif
