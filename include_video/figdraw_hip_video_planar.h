/* figdraw_hip_video_planar.h -- three-plane video in and out of libfigdraw_hip.so: what figdraw_hip_video_frame.h (frames into the atlas)
 * and figdraw_hip_video_out.h (the rendered frame out) do for the semi-planar formats of hardware decoders, for the planar formats of
 * software codecs and screen-content encoders -- I420 (ffmpeg's yuv420p; YV12 is the same with the two chroma pointers swapped), I010
 * (yuv420p10le), I444 (yuv444p) and I410 (yuv444p10le).  It reuses the matrix, range and flag enums of its two siblings and adds four
 * values to the format enum's space.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus,
 * fdh_last_error() says why).  -I include_video is all a caller adds.
 *
 * Why.  libavcodec, dav1d and libvpx on the way in and x264, SVT-AV1 and libaom on the way out speak planar 4:2:0; with two plane pointers
 * a caller had to interleave the chroma planes (and shift, for 10 bit) with a kernel of their own in front of fdh_put_video_frame, and
 * split them again behind fdh_read_video_frame: one more pass over the frame each way and a private restatement of a layout.  And every
 * route out halved the chroma resolution, which smears the coloured text and one-pixel borders this library renders: screen-content
 * encoders (H.264 High 4:4:4, HEVC RExt, AV1) take planar 4:4:4, which no semi-planar format offers.
 *
 * This comment is the specification.  tests/video_planar_ref.py restates it in numpy and the device
 * (figdraw_amd/csrc/k_video_planar_import.hip, k_video_planar_export.hip) is held to it byte for byte.
 *
 * THE PLANES.  planes[0] is Y, planes[1] Cb, planes[2] Cr; rows of plane p are pitch_bytes[p] apart.  Y is w x h samples.  For
 * FDH_VIDEO_I420 and FDH_VIDEO_I010 (4:2:0) Cb and Cr are cw = ceil(w / 2) x ch = ceil(h / 2) samples each; for FDH_VIDEO_I444 and
 * FDH_VIDEO_I410 (4:4:4) they are w x h.
 * - FDH_VIDEO_I420, FDH_VIDEO_I444: a sample is a byte; b = 8.
 * - FDH_VIDEO_I010, FDH_VIDEO_I410: a sample is a little-endian 16-bit word that holds its 10 bits at the BOTTOM (P010 holds them at the
 *   top); b = 10.  On the way in the sample is word & 1023: the six high bits are ignored, as P010 ignores its six low bits.  On the way
 *   out the six high bits are written as 0.
 *
 * THE WAY IN: fdh_put_video_planes, fdh_update_video_planes.  The arithmetic of figdraw_hip_video_frame.h for every texel, word for
 * word -- CHROMA FOR LUMA TEXEL, CONVERSION, the coefficients, A = 255 --; only the source of c[j][i] changes: it is sample i of row j of
 * planes[1] for Cb and of planes[2] for Cr.  I420 and I010 obey both chroma rules, the repeat and FDH_VIDEO_CHROMA_LINEAR, exactly as
 * NV12 and P010 do; I444 and I410 take c[y][x].  An 8-bit planar format uses the NV12 row of that header's table, a 10-bit one the P010
 * row (fdh_video_coefficients hands them out).  WHAT IS STORED is that header's too: placement, keep mode and growth, every level, the
 * ink boxes, the epoch, an update turning an entry into a chain entry.  It follows that an I420 frame leaves, byte for byte, what
 * fdh_put_video_frame leaves of the NV12 frame with the same samples interleaved, and an I010 frame what it leaves of the P010 frame of
 * value << 6.
 *
 * THE WAY OUT: fdh_read_video_planes.  THE SOURCE, the rectangle rule (rect x, y, w, h; w <= 0 or h <= 0: the whole frame; every clamp
 * is to the rectangle), the luma formula, the two 4:2:0 chroma rules and the coefficients are those of figdraw_hip_video_out.h; an 8-bit
 * planar format uses the NV12 row of that header's table, a 10-bit one the P010 row (fdh_video_out_coefficients).
 * - I420 and I010 write the Cb and the Cr of that specification's pair (i, j) to sample (i, j) of planes[1] and planes[2]: the I420
 *   planes are the NV12 export de-interleaved, the I010 planes the P010 export >> 6.
 * - I444 and I410 write one chroma sample per texel, the N = 1 case of the same formula, with R, G, B the texel's own colour bytes:
 *     Cb = clamp(Coff + ((kUR R + kUG G + kUB B + 8192) >> 14), 0, 2^b - 1); Cr the same with the kV row.
 *   The clamp is still needed: pure blue in 8-bit full range reaches 256.  The bound of figdraw_hip_video_out.h for N = 1: kUB and kUR are
 *   off by at most 1/2, kUG by at most 1, an operand is at most 255: the unrounded sum lies within 2 * 255 / 16384 < 0.032 of the exact
 *   value, so a sample is never more than 1 from the rounded float64 value and equal to it wherever that lies further from a half.
 * The bytes between a row's end and the pitch are never written.
 *
 * ORDERING.  As the siblings.  The way in reads the planes on the context's stream and returns after that stream is synchronised: the
 * planes may be reused on return.  The way out drains the submit thread, runs behind the frame and returns after a synchronise: the
 * planes are complete on return and the frame is untouched.
 *
 * REFUSALS.  FDH_ERR_INVALID, with nothing placed (no entry, no epoch bump, the packer untouched) or written:
 * - a null struct, or any of the three planes null;
 * - a format outside FDH_VIDEO_I420 .. FDH_VIDEO_I410, or an unknown matrix, range or flag; reserved != 0;
 * - either alpha flag (FDH_VIDEO_STRAIGHT_ALPHA, FDH_VIDEO_IGNORE_ALPHA); FDH_VIDEO_CHROMA_LINEAR with I444 or I410;
 * - on the way in: width or height <= 0;
 * - a pointer or pitch that is not a multiple of the sample size: 1 for the 8-bit formats, 2 for the 10-bit formats;
 * - a pitch below the plane's row bytes;
 * - fdh_update_video_planes: an unknown key, or a size that is not the entry's;
 * - on the way out: a rectangle that is not inside the frame; an odd x or y of the rectangle for I420 / I010 (odd w and h are fine; I444
 *   and I410 accept any rectangle); any two of the three planes' byte ranges overlapping;
 * - fdh_read_video_planes in addition: no frame submitted yet, a record-only context, a context under fdh_set_stripe;
 * - on a context with a device: a plane that hipPointerGetAttributes reports as neither device memory of the context's device nor
 *   page-locked host memory; a plane that overlaps one of the context's own surfaces (the way out) or its atlas (both ways).
 * On the way in the planes may alias each other: they are only read.  A record-only context validates and places, touches no memory and
 * sets no ink boxes.  fdh_check_video_planes_target applies every rule of the way out that needs no device.  The siblings' calls keep
 * refusing every format value above FDH_VIDEO_P010.
 *
 * NOT HERE.  4:2:2 (I422, I210, YUY2, UYVY) has calls of its own, with these structs: figdraw_hip_video_422.h; its formats take the values
 * from 7 on, which the calls here refuse.  Alpha planes (A420, A444, A410, UYVA) have calls of their own too: figdraw_hip_video_alpha.h, values
 * from 11 on.  Transfer functions and calls that do not wait for the stream are out of scope.
 *
 * ON THE DEVICE.  One kernel each way, a lane per run of EIGHT texels, so that a lane's narrowest access is the four bytes of an I420
 * chroma run (a run of four texels, the siblings' shape, would touch two bytes of either chroma plane).  The way in,
 * k_video_planar_import: a workgroup of 128 per 32 x 32 tile of the image; level 0 goes to the atlas, the tile through LDS down to one
 * texel; k_image_import_tail finishes the chain.  The way out, k_video_planar_export: a workgroup of 256 per 256 x 16 tile of the
 * rectangle, a lane per run of eight texels by two rows. */
#ifndef FIGDRAW_HIP_VIDEO_PLANAR_H
#define FIGDRAW_HIP_VIDEO_PLANAR_H
#include "figdraw_hip_video_out.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FDH_VIDEO_I420 = 3,   /* three planes of bytes: Y w x h; Cb and Cr ceil(w/2) x ceil(h/2) each */
       FDH_VIDEO_I010 = 4,   /* the same of little-endian 16-bit words, the 10-bit value in the LOW bits */
       FDH_VIDEO_I444 = 5,   /* three planes of bytes, w x h each */
       FDH_VIDEO_I410 = 6 }; /* the same of 16-bit words, 10 bits in the low bits */
typedef struct FdhVideoPlanes {
  const void* planes[3];     /* Y, Cb, Cr */
  int64_t pitch_bytes[3];    /* between rows of each plane */
  int32_t width, height;     /* of the luma plane */
  uint32_t format, matrix, range, flags;
  uint32_t reserved[2];      /* 0 */
} FdhVideoPlanes;
typedef struct FdhVideoPlanesTarget {
  void* planes[3];           /* Y, Cb, Cr */
  int64_t pitch_bytes[3];    /* between rows of each plane */
  int32_t rect[4];           /* x, y, w, h of the frame, top-down; w <= 0 or h <= 0: the whole frame */
  uint32_t format, matrix, range, flags;
  uint32_t reserved[2];      /* 0 */
} FdhVideoPlanesTarget;
/* out_rect = the packed rectangle x, y, w, h (may be NULL) */
FDH_API int fdh_put_video_planes(FdhContext*, int64_t key, const FdhVideoPlanes*, int out_rect[4]);
/* new texels for an entry of the same size */
FDH_API int fdh_update_video_planes(FdhContext*, int64_t key, const FdhVideoPlanes*);
FDH_API int fdh_read_video_planes(FdhContext*, const FdhVideoPlanesTarget*);
/* host only, no context: every rule of the way out that needs no device, for a frame of frame_w x frame_h */
FDH_API int fdh_check_video_planes_target(const FdhVideoPlanesTarget*, int frame_w, int frame_h);

#ifdef __cplusplus
}
#endif
#endif
