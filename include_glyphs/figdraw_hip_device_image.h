/* figdraw_hip_device_image.h -- atlas images from DEVICE memory for libfigdraw_hip.so: what fdh_put_image and fdh_update_image
 * (figdraw_hip.h) do for bytes the host holds, for pictures that were made on the GPU -- a model's output tensor, a decoded video frame, a
 * heat map, another context's rendered frame used as a cached layer.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or
 * a negative FdhStatus, fdh_last_error() says why).  The header lives in include_glyphs/ beside its siblings and reaches figdraw_hip.h by
 * its relative path: -I include_glyphs is all a caller adds.
 *
 * Why.  fdh_put_image takes pageable host bytes, builds the level chain on one CPU thread and sends every level up with a synchronous
 * copy.  A picture that is in device memory already would cross the bus twice on that way.  fdh_frame_device_ptr hands the library's
 * output out without a copy; these two calls are the matching way in.
 *
 * This comment is the specification.  tests/device_image_ref.py restates it in numpy and the device (figdraw_amd/csrc/k_image_import.hip)
 * is held to it byte for byte.
 *
 * THE SOURCE.  `data` points at width x height elements (planar: at `channels` planes of them); consecutive rows are pitch_bytes apart,
 * consecutive planes plane_bytes.
 * - FDH_IMAGE_RGBA8: an element is four bytes R, G, B, A, what fdh_put_image takes; channels = 4; plane_bytes is ignored.
 * - FDH_IMAGE_PLANAR_F32: an element is a float; `channels` (1, 3 or 4) planes, plane after plane: a CHW tensor.
 * - FDH_IMAGE_PLANAR_F16: the same of IEEE half.
 *
 * CONVERSION TO THE RGBA8 TEXEL.
 * - A planar value v (a half is widened to float first, which is exact): NaN gives byte 0.  Any other value gives
 *   rint(min(max(v, 0), 1) * 255.0f), computed in float32, ties to even: -0.0, negative values, denormals and -inf give 0, values from 1 up
 *   and +inf give 255.
 * - One channel: R = G = B = the byte, A = 255.  Three channels: A = 255.
 * - With FDH_IMAGE_STRAIGHT_ALPHA in `flags` the colour is not premultiplied yet: each colour byte c then becomes (c * a) / 255, an integer
 *   division, the rule fdh_put_flippy applies.  Integer arithmetic from there on.  Without the flag the bytes are taken as premultiplied.
 *
 * WHAT IS STORED.  Exactly what fdh_put_image (fdh_update_image) stores when given the converted bytes:
 * - the placement is the same, and so are keep mode (figdraw_hip_atlas.h), growth and the dropping of every entry on growth;
 * - the level chain: level l of the image is ceil(w / 2^l) x ceil(h / 2^l) texels at (x >> l, y >> l) of atlas level l, while both
 *   extents exceed 1 -- nothing at all is stored of an image 1 texel wide or high, not even level 0;
 * - each level is made of the one before with pixie's minifyBy2 on premultiplied RGBA8, per channel: the sum of a 2 x 2 block div 4.
 *   An odd width rounds the result's width up, and its extra column holds, of the last source column's texels a (row 2y) and b (row
 *   2y + 1), (((127 a + 128 b) div 255) * 128) div 255; an odd height likewise with the last row's texels (2x, 2x + 1); where both are odd
 *   the extra corner holds (64 v) div 255 of the last texel v;
 * - fdh_update_image_device of an entry that has levels of its own (fdh_put_flippy, fdh_put_image_mips) turns it into a chain entry;
 * - the atlas's epoch moves as it does for the host calls: retained scenes record the image again.
 *
 * INK BOXES.  For width, height <= 128 the entry gets the sixteen boxes a host put measures: for k = 0 .. 7 the bounding box of the
 * texels whose alpha exceeds 16 k, and of those whose largest colour channel does; a box with no texel is {0, 0, 0, 0}.  They are computed
 * on the device.  A draw of the image shrinks to them exactly as after fdh_put_image.  Larger images have none, as there.
 *
 * ORDERING.  The source is read on the context's stream, and the call returns after that stream is synchronised, like every put: the
 * source may be reused on return.  The caller makes sure that whatever wrote the source has finished, or is ordered on that stream
 * (fdh_set_stream).
 *
 * REFUSALS.  FDH_ERR_INVALID, before anything is placed -- no entry, no epoch bump, the packer untouched:
 * - a null struct or null data; width or height <= 0; an unknown format or flag; reserved != 0; channels outside the format's set;
 * - data or pitch_bytes not a multiple of the element size (4 for RGBA8: a texel is one aligned word; 4 for float, 2 for half), and for
 *   a planar format with more than one channel plane_bytes likewise;
 * - pitch_bytes below a row's bytes; plane_bytes < pitch_bytes * height for a planar format with more than one channel;
 * - fdh_update_image_device: an unknown key, or a size that is not the entry's;
 * - on a context with a device: a pointer that hipPointerGetAttributes reports as neither device memory of the context's device nor
 *   page-locked host memory.
 * A record-only context validates and places, touches no memory and sets no ink boxes.
 * The source must not be the context's own atlas.  A frame surface obtained from fdh_frame_device_ptr, of this or of another context on
 * the same device, is a valid source.
 *
 * ON THE DEVICE.  k_image_import: a workgroup of 256 per 32 x 32 tile of the image, a lane per run of four texels; level 0 goes to the
 * atlas, the tile through LDS down to one texel, each level stored on the way.  k_image_import_tail: one workgroup finishes the chain
 * from the level-5 image.  Two launches for any image up to 2048 x 2048. */
#ifndef FIGDRAW_HIP_DEVICE_IMAGE_H
#define FIGDRAW_HIP_DEVICE_IMAGE_H
#include "../include/figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FDH_IMAGE_RGBA8 = 0,        /* interleaved bytes R,G,B,A: what fdh_put_image takes */
       FDH_IMAGE_PLANAR_F32 = 1,   /* `channels` planes of float, plane after plane (a CHW tensor) */
       FDH_IMAGE_PLANAR_F16 = 2 }; /* the same of IEEE half */
enum { FDH_IMAGE_STRAIGHT_ALPHA = 1 };  /* colour is not premultiplied: premultiply on the way in */
typedef struct FdhDeviceImage {
  const void* data; int32_t width, height;
  int64_t pitch_bytes;   /* between rows (of one plane) */
  int64_t plane_bytes;   /* between planes; ignored for RGBA8 */
  uint32_t format, channels /* planar: 1, 3 or 4; RGBA8: 4 */, flags, reserved /* 0 */;
} FdhDeviceImage;
/* out_rect = the packed rectangle x, y, w, h (may be NULL) */
FDH_API int fdh_put_image_device(FdhContext*, int64_t key, const FdhDeviceImage*, int out_rect[4]);
/* new texels for an entry of the same size */
FDH_API int fdh_update_image_device(FdhContext*, int64_t key, const FdhDeviceImage*);

#ifdef __cplusplus
}
#endif
#endif
