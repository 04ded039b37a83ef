/* figdraw_hip_video_422.h -- 4:2:2 video in and out of libfigdraw_hip.so: what figdraw_hip_video_planar.h does for planar 4:2:0 and
 * 4:4:4, for the formats with a chroma sample per two texels of EVERY row -- I422 (ffmpeg's yuv422p), I210 (yuv422p10le), YUY2 (yuyv422)
 * and UYVY (uyvy422).  It reuses that header's two structs, FdhVideoPlanes and FdhVideoPlanesTarget, the matrix, range and flag enums of
 * its siblings, and adds four values to the format enum's space.  Same conventions as figdraw_hip.h (plain C, every call returns 0 or a
 * negative FdhStatus, fdh_last_error() says why).  -I include_video is all a caller adds.
 *
 * Why.  Capture cards, webcams and v4l2 hand out YUY2 or UYVY; ProRes, DNxHR and broadcast contribution codecs decode to yuv422p and
 * yuv422p10le; SDI and NDI sinks take UYVY; intermediate and mezzanine encoders take I422 and I210.  Without these calls such a caller
 * resamples vertically to 4:2:0 with a kernel of their own -- a lossy pass that no specification here covers -- or goes through RGBA8,
 * four bytes per pixel where two would do.  And for what this library renders, 4:2:2 out keeps the full vertical chroma: one-pixel
 * horizontal rules and text baselines keep their colour, at two thirds of I444's bytes.
 *
 * This comment is the specification.  tests/video_422_ref.py restates it in numpy and the device
 * (figdraw_amd/csrc/k_video_422_import.hip, k_video_422_export.hip) is held to it byte for byte.
 *
 * THE PLANES.  Y is w x h samples; there is one chroma row per luma row: cw = ceil(w / 2), ch = h.
 * - FDH_VIDEO_I422, FDH_VIDEO_I210: three planes as I420 and I010 have them -- planes[0] is Y, planes[1] Cb, planes[2] Cr, rows of
 *   plane p pitch_bytes[p] apart --, Cb and Cr cw x h samples each.  An I422 sample is a byte, b = 8.  An I210 sample is a little-endian
 *   16-bit word that holds its 10 bits at the BOTTOM, b = 10: on the way in the sample is word & 1023 (the six high bits are ignored),
 *   on the way out the six high bits are written as 0.
 * - FDH_VIDEO_YUY2, FDH_VIDEO_UYVY: ONE plane, planes[0], b = 8.  A row is cw groups of four bytes; group i holds the luma of columns 2 i
 *   and 2 i + 1 and chroma sample i: Y0 Cb Y1 Cr for YUY2, Cb Y0 Cr Y1 for UYVY.  planes[1], planes[2], pitch_bytes[1] and pitch_bytes[2]
 *   must be 0.  At an odd w the last group has one column: on the way in its second luma byte is ignored; on the way out it is written
 *   with the luma of column w - 1 -- the four-byte group is the format's unit, and a consumer reads it whole.  The bytes beyond 4 cw of a
 *   row are never written.
 *
 * THE WAY IN: fdh_put_video_422, fdh_update_video_422.  The arithmetic of figdraw_hip_video_frame.h for every texel, word for word --
 * CONVERSION, the coefficients, A = 255 --; the 8-bit formats use the NV12 row of that header's table, I210 the P010 row
 * (fdh_video_coefficients hands them out).  Only the source of the chroma sample changes.  c[y][i] is sample i of chroma row y (of
 * planes[1] for Cb, of planes[2] for Cr; of group i of row y for the packed formats); for the luma texel (x, y), with i = x >> 1:
 * - without FDH_VIDEO_CHROMA_LINEAR: C = c[y][i];
 * - with it the chroma is co-sited with the even luma columns, horizontally only (there is nothing to interpolate down a column):
 *     even x:  C = c[y][i]
 *     odd x:   C = (c[y][i] + c[y][min(i + 1, cw - 1)] + 1) >> 1
 *   This is the 4:2:0 rule of figdraw_hip_video_frame.h with the far chroma row equal to the near one, as integers:
 *   (3 c + c + 2) >> 2 = c and (3 c + c + 3 c' + c' + 4) >> 3 = (4 c + 4 c' + 4) >> 3 = (c + c' + 1) >> 1.  So an I422 frame whose chroma
 *   is constant down every column converts to what the I420 frame of every second chroma row converts to, under both rules.
 * WHAT IS STORED is fdh_put_image's of the converted bytes, as for every sibling: placement, keep mode and growth, every level, the ink
 * boxes, the epoch, an update turning an entry into a chain entry.
 *
 * THE WAY OUT: fdh_read_video_422.  THE SOURCE, the rectangle rule (rect x, y, w, h; w <= 0 or h <= 0: the whole frame; every clamp is
 * to the rectangle) and the luma formula are those of figdraw_hip_video_out.h; the 8-bit formats use the NV12 row of that header's table,
 * I210 the P010 row (fdh_video_out_coefficients).  Chroma sample (i, y), one per luma row, from the colour bytes p(x, y) of row y alone:
 * - without FDH_VIDEO_CHROMA_LINEAR: xa = 2 i, xb = min(2 i + 1, w - 1); s = p(xa, y) + p(xb, y); N = 2;
 * - with it: xl = max(2 i - 1, 0), xc = 2 i, xr = min(2 i + 1, w - 1); s = p(xl, y) + 2 p(xc, y) + p(xr, y); N = 4;
 * then that header's one formula:
 *     Cb = clamp(Coff + ((kUR sR + kUG sG + kUB sB + (N << 13)) >> (14 + log2 N)), 0, 2^b - 1); Cr the same with the kV row.
 * The bound is that header's, unchanged: an operand is at most 255 N under a shift that is log2 N longer, so the unrounded value lies
 * within 2 * 255 / 16384 < 0.032 of the exact value of the averaged colour -- a sample is never more than 1 from the rounded float64
 * value and equal to it wherever that lies further from a half --, and N <= 8 already proved that no sum reaches 2^31.  It follows that
 * the I422 chroma planes of a frame whose rows 2 j and 2 j + 1 are equal are the I420 chroma planes of that frame with every row
 * doubled: s of 4:2:0 is then twice s of 4:2:2 under a shift one longer, with twice the rounding term.  YUY2 and UYVY out are the I422
 * samples interleaved.  The bytes between a row's end and the pitch are never written.
 *
 * ORDERING.  As the siblings.  The way in reads the planes on the context's stream and returns after that stream is synchronised: the
 * planes may be reused on return.  The way out drains the submit thread, runs behind the frame and returns after a synchronise: the
 * planes are complete on return and the frame is untouched.
 *
 * REFUSALS.  FDH_ERR_INVALID, with nothing placed (no entry, no epoch bump, the packer untouched) or written:
 * - a null struct, a null planes[0]; for I422 / I210 a null planes[1] or planes[2]; for YUY2 / UYVY any of planes[1], planes[2],
 *   pitch_bytes[1], pitch_bytes[2] set;
 * - a format outside FDH_VIDEO_I422 .. FDH_VIDEO_UYVY, or an unknown matrix, range or flag; reserved != 0;
 * - either alpha flag (FDH_VIDEO_STRAIGHT_ALPHA, FDH_VIDEO_IGNORE_ALPHA);
 * - on the way in: width or height <= 0;
 * - a pointer or pitch that is not a multiple of the element size: 1 for I422, 2 for I210, 4 -- the group -- for YUY2 / UYVY;
 * - a pitch below the row's bytes: w samples of luma, cw samples of chroma, 4 cw bytes of a packed row;
 * - fdh_update_video_422: an unknown key, or a size that is not the entry's;
 * - on the way out: a rectangle that is not inside the frame; an odd x of the rectangle (any y, and odd w and h, are fine); any two of
 *   the three planes' byte ranges overlapping;
 * - fdh_read_video_422 in addition: no frame submitted yet, a record-only context, a context under fdh_set_stripe;
 * - on a context with a device: a plane that hipPointerGetAttributes reports as neither device memory of the context's device nor
 *   page-locked host memory; a plane that overlaps one of the context's own surfaces (the way out) or its atlas (both ways).
 * On the way in the planes may alias each other: they are only read.  A record-only context validates and places, touches no memory and
 * sets no ink boxes.  fdh_check_video_422_target applies every rule of the way out that needs no device.  The three sibling families keep
 * refusing every format value from FDH_VIDEO_I422 on, and these calls refuse every value outside FDH_VIDEO_I422 .. FDH_VIDEO_UYVY.
 *
 * NOT HERE.  The semi-planar 4:2:2 formats NV16 and P210 / P216, the packed 10-bit formats Y210 and v210, transfer functions, and calls
 * that do not wait for the stream.  Alpha planes are in figdraw_hip_video_alpha.h: UYVA there is this header's UYVY plane and an alpha plane.
 *
 * ON THE DEVICE.  One kernel each way, a lane per run of EIGHT texels of one row: eight luma samples and four of either chroma plane, or
 * the four groups, 16 bytes, of a packed row.  The way in, k_video_422_import: a workgroup of 128 per 32 x 32 tile of the image; level 0
 * goes to the atlas, the tile through LDS down to one texel; k_image_import_tail finishes the chain.  The way out, k_video_422_export: a
 * workgroup of 256 per 256 x 8 tile of the rectangle. */
#ifndef FIGDRAW_HIP_VIDEO_422_H
#define FIGDRAW_HIP_VIDEO_422_H
#include "figdraw_hip_video_planar.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FDH_VIDEO_I422 = 7,    /* three planes of bytes: Y w x h; Cb and Cr ceil(w/2) x h each (yuv422p) */
       FDH_VIDEO_I210 = 8,    /* the same of little-endian 16-bit words, 10 bits at the bottom (yuv422p10le) */
       FDH_VIDEO_YUY2 = 9,    /* one plane: per two texels the bytes Y0 Cb Y1 Cr (yuyv422) */
       FDH_VIDEO_UYVY = 10 }; /* one plane: per two texels the bytes Cb Y0 Cr Y1 (uyvy422) */
/* out_rect = the packed rectangle x, y, w, h (may be NULL) */
FDH_API int fdh_put_video_422(FdhContext*, int64_t key, const FdhVideoPlanes*, int out_rect[4]);
/* new texels for an entry of the same size */
FDH_API int fdh_update_video_422(FdhContext*, int64_t key, const FdhVideoPlanes*);
FDH_API int fdh_read_video_422(FdhContext*, const FdhVideoPlanesTarget*);
/* host only, no context: every rule of the way out that needs no device, for a frame of frame_w x frame_h */
FDH_API int fdh_check_video_422_target(const FdhVideoPlanesTarget*, int frame_w, int frame_h);

#ifdef __cplusplus
}
#endif
#endif
