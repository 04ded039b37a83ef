/* figdraw_hip_video_frames.h -- a BATCH of decoded video frames into the atlas of libfigdraw_hip.so: what n calls of fdh_put_video_frame
 * (fdh_update_video_frame; figdraw_hip_video_frame.h) do, in a number of launches that does not depend on n and with one wait for the
 * stream.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says why).  The
 * header lives in include_glyphs/ beside its siblings and reaches figdraw_hip_video_frame.h by its relative path.
 *
 * Why.  A single call is a launch or two of a few workgroups and a wait for the stream: its time hardly depends on the frame
 * (profiles/video_frame.txt).  A conference grid or a monitoring wall refreshes 9 to 64 entries per rendered frame; each pays that price
 * per stream and leaves the device idle meanwhile.  fdh_put_images_device (figdraw_hip_device_images.h) is the same idea for RGBA8 and
 * float planes, which no decoder hands out.
 *
 * This comment is the specification.
 *
 * THE FRAMES.  FdhVideoFrame, its formats (NV12, P010, BGRA8), matrices, ranges and flags, the chroma rule, the conversion and its
 * coefficients, the level chain, the ink boxes, the rules for pointers and every refusal are those of figdraw_hip_video_frame.h,
 * unchanged.  A batch may mix formats, matrices, ranges, flags, alignments, pitches and sizes.
 *
 * THE CONTRACT.  After fdh_put_video_frames the context is what the n calls fdh_put_video_frame(ctx, keys[i], &frames[i],
 * out_rects[i]), i = 0 .. n - 1, would have left, byte for byte: the directory, the packer, out_rects, the atlas's size and epoch; every
 * level of the atlas; every entry's sixteen ink boxes.  fdh_update_video_frames is held to the n calls of fdh_update_video_frame in
 * the same way; an entry that has levels of its own becomes a chain entry, as there.  Where the rectangles of two frames of the batch
 * meet in a deep level of the chain (from level 4 on) the texel is the later frame's, as after single calls.  out_rects may be NULL.
 *
 * THE DIFFERENCES, those of the image batch (figdraw_hip_device_images.h), word for word:
 * 1. Everything is validated before anything is placed or bumped: n < 0, or n > 0 with a null array; every struct by the single call's
 *    rules; for updates every key known and every size the entry's; on a context with a device every pointer's address space, and no
 *    source inside the context's own atlas; the batch limits below.  One bad image refuses the whole call with FDH_ERR_INVALID: no entry
 *    is made, the epoch does not move, no texel and no ink box changes, out_rects is not written.  n == 0 is FDH_OK and places nothing.
 * 2. A put batch places all images first, in order, and then makes the texels.  Images placed before the batch's last growth of the atlas
 *    are not written (growth drops every entry, as ever): their out_rects are filled and dropped_by_growth counts them.  On
 *    FDH_ERR_ATLAS_FULL at image i the images before i are in the atlas with their texels, and the error is returned.  In keep mode room
 *    is made once for the whole batch; the rule figdraw_hip_atlas.h states for batches applies unchanged.
 * 3. A key that occurs twice in one batch is refused, in both calls: one launch has no order in which a whole image could replace another.
 * (Read "frame" for "image".)
 *
 * BATCH LIMITS, each FDH_ERR_INVALID: n <= 65535; every width and height at most 2048 (the tail's workgroup holds a 64 x 64 level-5
 * image: a 1920 x 1080 frame fits, a 3840 x 2160 frame keeps the single call); the 32 x 32 tiles of all frames together at most 2^18 (a
 * tile table of 1 MB, page-locked ink blocks of 64 MB).
 *
 * A record-only context validates, places, touches no memory, sets no ink boxes and reports launches = 0.
 *
 * ORDERING.  As for the single calls: the batch waits for the submit thread, reads the planes on the context's stream and returns after
 * that stream is synchronised, once, at its end; the planes may be reused on return.
 *
 * ON THE DEVICE.  k_video_import_batch<format, linear>, the five builds the single kernel has: a workgroup of 256 per 32 x 32 tile, over
 * a 1-D grid of the tiles of all frames of one group -- BGRA8, and NV12 and P010 each without and with FDH_VIDEO_CHROMA_LINEAR; a table
 * word per tile names its frame and its place in it, a record per frame holds what the single kernel gets as arguments.
 * k_image_import_tail_batch, the image batch's, as it stands: a workgroup per frame whose chain goes beyond level 5.  The conversion, the
 * loads and the chain's steps are the functions the single kernel calls; a store into level 4 or deeper happens only where the frame's
 * owner bit is set (the host paints the rectangles in array order).  At most one launch per group present and one for the tails: six,
 * whatever n is.
 * One deliberate difference from the image batch: a frame 1 texel wide or high keeps its tiles in the table.  Nothing of such a frame is
 * stored (the kernel stores no level of it), but its tiles leave their ink blocks as the single call's do, so the host never restates the
 * YUV conversion for lines; `tiles` and `launches` count them. */
#ifndef FIGDRAW_HIP_VIDEO_FRAMES_H
#define FIGDRAW_HIP_VIDEO_FRAMES_H
#include "figdraw_hip_video_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out_rects[i] = the packed rectangle x, y, w, h of frame i (out_rects may be NULL) */
FDH_API int fdh_put_video_frames(FdhContext*, const int64_t* keys, const FdhVideoFrame* frames, int n, int (*out_rects)[4]);
/* new texels for n entries of the same sizes */
FDH_API int fdh_update_video_frames(FdhContext*, const int64_t* keys, const FdhVideoFrame* frames, int n);
/* of the last batch, put or update, that passed validation */
typedef struct FdhVideoBatchStats {
  int32_t frames;             /* n */
  int32_t written;            /* frames whose texels were made (a record-only context: that got a place) */
  int32_t dropped_by_growth;  /* placed before the batch's last growth: not in the atlas any more */
  int32_t tiles;              /* 32 x 32 tiles of the written frames */
  int32_t launches;           /* kernel launches: at most 6 */
  int32_t reserved;
  int64_t bytes_copied;       /* the tables, host to device */
} FdhVideoBatchStats;
FDH_API int fdh_video_batch_stats(FdhContext*, FdhVideoBatchStats* out);
FDH_API int fdh_sizeof_video_frame(void);  /* sizeof(FdhVideoFrame) as the library was built: a binding checks its own layout against it */

#ifdef __cplusplus
}
#endif
#endif
