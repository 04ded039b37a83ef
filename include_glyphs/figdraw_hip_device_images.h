/* figdraw_hip_device_images.h -- a BATCH of atlas images from device memory for libfigdraw_hip.so: what n calls of fdh_put_image_device
 * (fdh_update_image_device; figdraw_hip_device_image.h) do, in a number of launches that does not depend on n and with one wait for the
 * stream.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says why).  The
 * header lives in include_glyphs/ beside its siblings and reaches figdraw_hip_device_image.h by its relative path.
 *
 * Why.  A single call is a launch or two of a few workgroups and a wait for the stream: its time hardly depends on the image
 * (profiles/device_image.txt).  Sixteen live thumbnails refreshed per frame, a wall of decoded streams, a model's N x C x H x W output
 * shown as a grid, an atlas filled with a few hundred icons made on the GPU: each pays that price per image and leaves the device idle
 * meanwhile.  The glyph batches (figdraw_hip_glyphs.h, figdraw_hip_coverage.h) are the same idea for outlines.
 *
 * This comment is the specification.
 *
 * THE IMAGES.  FdhDeviceImage, its formats, FDH_IMAGE_STRAIGHT_ALPHA, the conversion to the RGBA8 texel, the level chain, the ink boxes
 * and the rules for pointers are those of figdraw_hip_device_image.h, unchanged.  A batch may mix formats, channel counts, flags,
 * alignments and sizes.
 *
 * THE CONTRACT.  After fdh_put_images_device the context is what the n calls fdh_put_image_device(ctx, keys[i], &images[i],
 * out_rects[i]), i = 0 .. n - 1, would have left, byte for byte: the directory, the packer, out_rects, the atlas's size and epoch; every
 * level of the atlas; every entry's sixteen ink boxes.  fdh_update_images_device is held to the n calls of fdh_update_image_device in
 * the same way; an entry that has levels of its own becomes a chain entry, as there.  Where the rectangles of two images of the batch
 * meet in a deep level of the chain (from level 4 on; the packer's margin is the same for images as for glyphs) the texel is the later
 * image's, as after single calls.  out_rects may be NULL.
 *
 * THE DIFFERENCES, those of the glyph batches and one more:
 * 1. Everything is validated before anything is placed or bumped: n < 0, or n > 0 with a null array; every struct by the single call's
 *    rules; for updates every key known and every size the entry's; on a context with a device every pointer's address space, and no
 *    source inside the context's own atlas; the batch limits below.  One bad image refuses the whole call with FDH_ERR_INVALID: no entry
 *    is made, the epoch does not move, no texel and no ink box changes, out_rects is not written.  n == 0 is FDH_OK and places nothing.
 * 2. A put batch places all images first, in order, and then makes the texels.  Images placed before the batch's last growth of the atlas
 *    are not written (growth drops every entry, as ever): their out_rects are filled and dropped_by_growth counts them.  On
 *    FDH_ERR_ATLAS_FULL at image i the images before i are in the atlas with their texels, and the error is returned.  In keep mode room
 *    is made once for the whole batch; the rule figdraw_hip_atlas.h states for batches applies unchanged.
 * 3. A key that occurs twice in one batch is refused, in both calls: one launch has no order in which a whole image could replace another.
 *
 * BATCH LIMITS, each FDH_ERR_INVALID: n <= 65535; every width and height at most 2048 (up to there one workgroup finishes an image's
 * chain; larger images keep the single call); the 32 x 32 tiles of all images together at most 2^18 (a tile table of 1 MB, page-locked
 * ink blocks of 64 MB).
 *
 * A record-only context validates, places, touches no memory, sets no ink boxes and reports launches = 0.
 *
 * ORDERING.  As for the single calls: the batch waits for the submit thread, reads the sources on the context's stream and returns after
 * that stream is synchronised, once, at its end; the sources may be reused on return.
 *
 * ON THE DEVICE.  k_image_import_batch<format>: a workgroup of 256 per 32 x 32 tile, over a 1-D grid of the tiles of all images of that
 * format; a table word per tile names its image and its place in it, a record per image holds what the single kernel gets as arguments.
 * k_image_import_tail_batch: a workgroup per image whose chain goes beyond level 5.  The texel code is the single kernels'; a store into
 * level 4 or deeper happens only where the image's owner bit is set (the host paints the rectangles in array order).  At most one launch
 * per format present and one for the tails: four, whatever n is.  An image 1 texel wide or high has no tile -- nothing of it is stored --
 * and its ink boxes are measured on the host, from a copy of its one row or column. */
#ifndef FIGDRAW_HIP_DEVICE_IMAGES_H
#define FIGDRAW_HIP_DEVICE_IMAGES_H
#include "figdraw_hip_device_image.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out_rects[i] = the packed rectangle x, y, w, h of image i (out_rects may be NULL) */
FDH_API int fdh_put_images_device(FdhContext*, const int64_t* keys, const FdhDeviceImage* images, int n, int (*out_rects)[4]);
/* new texels for n entries of the same sizes */
FDH_API int fdh_update_images_device(FdhContext*, const int64_t* keys, const FdhDeviceImage* images, int n);
/* of the last batch, put or update, that passed validation */
typedef struct FdhImageBatchStats {
  int32_t images;             /* n */
  int32_t written;            /* images whose texels were made (a record-only context: that got a place) */
  int32_t dropped_by_growth;  /* placed before the batch's last growth: not in the atlas any more */
  int32_t tiles;              /* 32 x 32 tiles of the written images */
  int32_t launches;           /* kernel launches: at most 4 */
  int32_t reserved;
  int64_t bytes_copied;       /* the tables, host to device */
} FdhImageBatchStats;
FDH_API int fdh_image_batch_stats(FdhContext*, FdhImageBatchStats* out);
FDH_API int fdh_sizeof_device_image(void);  /* sizeof(FdhDeviceImage) as the library was built: a binding checks its own layout against it */

#ifdef __cplusplus
}
#endif
#endif
