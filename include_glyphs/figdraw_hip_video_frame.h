/* figdraw_hip_video_frame.h -- decoded video frames into the atlas of libfigdraw_hip.so: fdh_put_image_device (figdraw_hip_device_image.h)
 * for the formats decoders, capture and compositing APIs hand out -- NV12 (8 bit), P010 (10 bit) and BGRA8 -- read where they lie in
 * device memory.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says why).
 * The header lives in include_glyphs/ beside its siblings and reaches figdraw_hip.h by its relative path: -I include_glyphs is all a
 * caller adds.
 *
 * Why.  fdh_put_image_device takes RGBA8 and float / half planes.  No decoder produces those: an application that shows video in a scene
 * would run a colour conversion of its own into an RGBA8 buffer first -- four bytes written and four read per pixel, a launch and a buffer
 * more -- where an NV12 frame is 1.5 bytes per pixel.
 *
 * This comment is the specification.  tests/video_frame_ref.py restates it in numpy and the device (figdraw_amd/csrc/k_video_import.hip)
 * is held to it byte for byte.
 *
 * THE SOURCE.  planes[0] is the luma plane of width x height samples, or the BGRA texels; planes[1] is the chroma plane of
 * cw = ceil(width / 2) x ch = ceil(height / 2) pairs Cb, Cr (NULL for BGRA8).  Rows of plane p are pitch_bytes[p] apart (pitch_bytes[1]
 * is 0 for BGRA8).
 * - FDH_VIDEO_NV12: a sample is a byte; b = 8.
 * - FDH_VIDEO_P010: a sample is a little-endian 16-bit word, its value word >> 6: the low six bits are ignored; b = 10.
 * - FDH_VIDEO_BGRA8: a texel is the bytes B, G, R, A.
 * S = 2^(b - 8) below.
 *
 * CHROMA FOR LUMA TEXEL (x, y).  c[j][i] is either component of pair i of chroma row j.
 * - Without FDH_VIDEO_CHROMA_LINEAR: c[y >> 1][x >> 1].
 * - With it, the MPEG-2 / H.264 default siting: chroma is co-sited with the even luma columns and lies midway between luma rows 2j and
 *   2j + 1.  In integers: j = y >> 1; jn = (y odd) ? min(j + 1, ch - 1) : max(j - 1, 0); v(i) = 3 c[j][i] + c[jn][i]; i = x >> 1;
 *   even x: C = (v(i) + 2) >> 2; odd x: C = (v(i) + v(min(i + 1, cw - 1)) + 4) >> 3.
 *
 * CONVERSION.  All arithmetic is int32, >> is an arithmetic shift (floor).  With y = Y - Yoff, u = Cb - Coff, v = Cr - Coff:
 *   R = clamp((cY y + cRV v + 8192) >> 14, 0, 255)
 *   G = clamp((cY y - cGU u - cGV v + 8192) >> 14, 0, 255)
 *   B = clamp((cY y + cBU u + 8192) >> 14, 0, 255)
 *   A = 255
 * The coefficients are 255 * 2^14 times these terms, rounded to the nearest integer, ties to even: cY: 1 / Yden; cRV: 2 (1 - Kr) / Cden;
 * cGU: 2 Kb (1 - Kb) / (Kg Cden); cGV: 2 Kr (1 - Kr) / (Kg Cden); cBU: 2 (1 - Kb) / Cden.  FDH_VIDEO_LIMITED: Yoff = 16 S, Yden = 219 S,
 * Cden = 224 S; FDH_VIDEO_FULL: Yoff = 0, Yden = Cden = 2^b - 1.  Coff = 128 S.  (Kr, Kb) = (0.299, 0.114) for BT601, (0.2126, 0.0722)
 * for BT709, (0.2627, 0.0593) for BT2020 (non-constant luminance); Kg = 1 - Kr - Kb.  That gives {cY, cRV, cGU, cGV, cBU}:
 *
 *            8 bit limited                     8 bit full                        10 bit limited                10 bit full
 *   BT601    19077 26149 6419 13320 33050      16384 22970 5638 11700 29032      4769 6537 1605 3330 8263      4084 5726 1405 2917 7237
 *   BT709    19077 29372 3494  8731 34610      16384 25802 3069  7670 30402      4769 7343  873 2183 8652      4084 6431  765 1912 7578
 *   BT2020   19077 27503 3069 10657 35091      16384 24160 2696  9361 30825      4769 6876  767 2664 8773      4084 6022  672 2333 7684
 *
 * fdh_video_coefficients hands a row out.  A coefficient is off by at most 2^-15 of its unit, an operand is at most 1023 and there are three
 * terms: the unrounded sum lies within 3 * 1023 / 32768 < 0.094 of the exact value, so the byte is never more than 1 from the rounded
 * float64 value and equal to it wherever that value lies more than 0.094 from a half.  No sum reaches 2^31.
 *
 * BGRA8.  R, G, B, A are the texel's bytes 2, 1, 0, 3; `matrix` and `range` must be 0.  FDH_VIDEO_IGNORE_ALPHA sets A = 255 (BGRX).
 * FDH_VIDEO_STRAIGHT_ALPHA: the colour is not premultiplied yet and each colour byte c becomes (c * a) / 255, the rule of
 * FDH_IMAGE_STRAIGHT_ALPHA.  Without either flag the bytes are taken as premultiplied.
 *
 * WHAT IS STORED.  Exactly what fdh_put_image / fdh_update_image store when given the converted RGBA8 bytes -- placement, keep mode and
 * growth, the level chain, the ink boxes of images up to 128 x 128, the epoch, and an update of an entry with levels of its own turning it
 * into a chain entry: the sections WHAT IS STORED and INK BOXES of figdraw_hip_device_image.h hold word for word.
 *
 * ORDERING.  As fdh_put_image_device: the planes are read on the context's stream, and the call returns after that stream is
 * synchronised; the planes may be reused on return.
 *
 * REFUSALS.  FDH_ERR_INVALID, before anything is placed -- no entry, no epoch bump, the packer untouched:
 * - a null struct or null planes[0]; null planes[1] for NV12 / P010; width or height <= 0;
 * - an unknown format, matrix, range or flag; reserved != 0;
 * - BGRA8 with matrix or range != 0, with planes[1] or pitch_bytes[1] set, with FDH_VIDEO_CHROMA_LINEAR, or with both alpha flags; NV12 /
 *   P010 with either alpha flag;
 * - a pointer or pitch that is not a multiple of the plane's element size: BGRA8 4; NV12 luma 1, chroma pair 2; P010 luma 2, chroma pair 4;
 * - pitch_bytes[0] below a luma row's bytes; pitch_bytes[1] below cw pairs;
 * - fdh_update_video_frame: an unknown key, or a size that is not the entry's;
 * - on a context with a device: either plane that hipPointerGetAttributes reports as neither device memory of the context's device nor
 *   page-locked host memory; a plane that overlaps the context's own atlas.
 * A record-only context validates and places, touches no memory and sets no ink boxes.
 *
 * ON THE DEVICE.  k_video_import: the tile shape of k_image_import -- a workgroup of 256 per 32 x 32 tile of the image, a lane per run
 * of four texels, which is one load of four luma bytes and one of two chroma pairs for NV12 where pointers and pitches allow it.  Level 0
 * goes to the atlas, the tile through LDS down to one texel; k_image_import_tail finishes the chain. */
#ifndef FIGDRAW_HIP_VIDEO_FRAME_H
#define FIGDRAW_HIP_VIDEO_FRAME_H
#include "../include/figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FDH_VIDEO_BGRA8 = 0,   /* interleaved bytes B,G,R,A */
       FDH_VIDEO_NV12 = 1,    /* a plane of luma bytes, a plane of Cb,Cr byte pairs at half the size each way */
       FDH_VIDEO_P010 = 2 };  /* the same of 16-bit words that hold 10 bits at the top */
enum { FDH_VIDEO_BT601 = 0, FDH_VIDEO_BT709 = 1, FDH_VIDEO_BT2020 = 2 };   /* non-constant luminance */
enum { FDH_VIDEO_LIMITED = 0, FDH_VIDEO_FULL = 1 };
enum { FDH_VIDEO_CHROMA_LINEAR = 1,    /* NV12 / P010: interpolate chroma (MPEG-2 siting) where the default repeats it */
       FDH_VIDEO_STRAIGHT_ALPHA = 2,   /* BGRA8: colour is not premultiplied: premultiply on the way in */
       FDH_VIDEO_IGNORE_ALPHA = 4 };   /* BGRA8: the fourth byte is padding (BGRX): A = 255 */
typedef struct FdhVideoFrame {
  const void* planes[2];     /* [0] luma, or the BGRA texels; [1] interleaved Cb,Cr (NULL for BGRA8) */
  int64_t pitch_bytes[2];    /* between rows of each plane ([1] is 0 for BGRA8) */
  int32_t width, height;     /* of the luma plane; the chroma plane is ceil(w/2) x ceil(h/2) pairs */
  uint32_t format, matrix, range, flags;
  uint32_t reserved[2];      /* 0 */
} FdhVideoFrame;
/* out_rect = the packed rectangle x, y, w, h (may be NULL) */
FDH_API int fdh_put_video_frame(FdhContext*, int64_t key, const FdhVideoFrame*, int out_rect[4]);
/* new texels for an entry of the same size */
FDH_API int fdh_update_video_frame(FdhContext*, int64_t key, const FdhVideoFrame*);
/* host only, needs no context: out = Yoff, Coff, cY, cRV, cGU, cGV, cBU of the conversion above for FDH_VIDEO_NV12 or FDH_VIDEO_P010 */
FDH_API int fdh_video_coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[7]);

#ifdef __cplusplus
}
#endif
#endif
