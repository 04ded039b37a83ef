/* figdraw_hip_video_out.h -- the rendered frame of libfigdraw_hip.so out as NV12 (8 bit), P010 (10 bit) or BGRA8, written where an encoder,
 * a capture sink or a compositing API reads it: device memory or page-locked host memory.  The inverse direction of
 * figdraw_hip_video_frame.h, whose format / matrix / range / flag enums it reuses.  Same conventions as figdraw_hip.h (plain C, every
 * call returns 0 or a negative FdhStatus, fdh_last_error() says why).  The header lives in include_video/ and reaches its siblings by
 * their relative paths: -I include_video is all a caller adds.
 *
 * Why.  fdh_read_pixels copies RGBA8 to pageable host memory and fdh_frame_device_ptr hands out the RGBA8 surface.  No encoder takes
 * RGBA8: an application that streams what this library renders would run a conversion launch of its own on the surface -- a second
 * statement of the BT.601 / 709 / 2020 arithmetic that does not invert the one fdh_put_video_frame documents, four bytes written per
 * pixel where NV12 is 1.5.  With this call "decode, composite over the video, encode" stays on the device.
 *
 * This comment is the specification.  tests/video_out_ref.py restates it in numpy and the device (figdraw_amd/csrc/k_video_export.hip)
 * is held to it byte for byte.
 *
 * THE SOURCE.  The RGBA8 bytes that fdh_read_pixels returns for `rect` (x, y, w, h; top-down; w <= 0 or h <= 0: the whole frame) of the
 * last submitted frame: p(x, y) for 0 <= x < w, 0 <= y < h, relative to the rectangle.  Colour bytes are taken as stored (the surface is
 * premultiplied; an opaque frame's colours are the colours); for NV12 / P010 the alpha byte is ignored.  Every clamp below is to the
 * rectangle, not to the frame: a rectangle's export is the export of a frame cropped to it.
 *
 * THE PLANES.  planes[0] takes w x h luma samples, or the BGRA texels; planes[1] takes cw = ceil(w / 2) x ch = ceil(h / 2) pairs Cb, Cr
 * (NULL for BGRA8).  Rows of plane p are pitch_bytes[p] apart (pitch_bytes[1] is 0 for BGRA8).  The bytes between a row's end and the
 * pitch are never written.
 * - FDH_VIDEO_NV12: a sample is a byte; b = 8.
 * - FDH_VIDEO_P010: a sample is a little-endian 16-bit word value << 6, its low six bits zero; b = 10.
 * - FDH_VIDEO_BGRA8: a texel is the bytes B, G, R, A = the source's R, G, B, A swapped; FDH_VIDEO_IGNORE_ALPHA stores A = 255 (BGRX).
 *   `matrix` and `range` must be 0.
 *
 * LUMA AND CHROMA.  All arithmetic is int32, >> is an arithmetic shift (floor).  R, G, B are a texel's colour bytes.
 *   luma sample (x, y):  Y = Yoff + ((kYR R + kYG G + kYB B + 8192) >> 14)
 * Chroma pair (i, j) uses the rows ya = 2 j and yb = min(2 j + 1, h - 1).
 * - Without FDH_VIDEO_CHROMA_LINEAR chroma sits at the centre of the 2 x 2 block: columns xa = 2 i and xb = min(2 i + 1, w - 1); s is
 *   the component-wise sum of the four texels; N = 4.
 * - With it the siting is the one fdh_put_video_frame assumes under the same flag -- co-sited with the even luma columns, midway
 *   between the two rows: columns xl = max(2 i - 1, 0), xc = 2 i, xr = min(2 i + 1, w - 1); s is the sum over both rows of
 *   p(xl) + 2 p(xc) + p(xr); N = 8.
 *   Cb = clamp(Coff + ((kUR sR + kUG sG + kUB sB + (N << 13)) >> (14 + log2 N)), 0, 2^b - 1); Cr the same with the kV row.
 *
 * COEFFICIENTS.  Yoff, Yden, Cden, Coff, Kr, Kb, Kg exactly as in figdraw_hip_video_frame.h (FDH_VIDEO_LIMITED: Yoff = 16 S, Yden = 219 S,
 * Cden = 224 S; FDH_VIDEO_FULL: Yoff = 0, Yden = Cden = 2^b - 1; Coff = 128 S; S = 2^(b - 8)).  TY = Yden 2^14 / 255, TC = Cden 2^14 / 255;
 * rne rounds an exact rational to the nearest integer, ties to even.
 *   kYR = rne(Kr TY)    kYB = rne(Kb TY)    kYG = rne(TY) - kYR - kYB
 *   kUB = kVR = rne(TC / 2)
 *   kUR = -rne(Kr TC / (2 (1 - Kb)))    kUG = -(kUB + kUR)
 *   kVB = -rne(Kb TC / (2 (1 - Kr)))    kVG = -(kVR + kVB)
 * Each chroma row sums to exactly 0, so any grey gives Coff; the luma row sums to rne(TY), so white gives Yoff + Yden and black Yoff.
 * That gives {kYR kYG kYB  kUR kUG kUB  kVR kVG kVB}:
 *
 *    8 bit limited  BT601   4207  8260 1604   -2428  -4768  7196   7196  -6026 -1170
 *                   BT709   2991 10064 1016   -1649  -5547  7196   7196  -6536  -660
 *                   BT2020  3696  9541  834   -2010  -5186  7196   7196  -6617  -579
 *    8 bit full     BT601   4899  9617 1868   -2765  -5427  8192   8192  -6860 -1332
 *                   BT709   3483 11718 1183   -1877  -6315  8192   8192  -7441  -751
 *                   BT2020  4304 11108  972   -2288  -5904  8192   8192  -7533  -659
 *   10 bit limited  BT601  16829 33039 6416   -9714 -19070 28784  28784 -24103 -4681
 *                   BT709  11966 40254 4064   -6596 -22188 28784  28784 -26145 -2639
 *                   BT2020 14786 38160 3338   -8038 -20746 28784  28784 -26469 -2315
 *   10 bit full     BT601  19653 38583 7493  -11091 -21773 32864  32864 -27519 -5345
 *                   BT709  13974 47009 4746   -7531 -25333 32864  32864 -29851 -3013
 *                   BT2020 17267 44564 3898   -9178 -23686 32864  32864 -30221 -2643
 *
 * fdh_video_out_coefficients hands a row out.  The bound is coefficient error times the largest operand, summed over the three terms.
 * Luma: kYR and kYB are off by at most 1/2, kYG -- a difference of three roundings -- by at most 3/2, an operand is at most 255: the
 * unrounded sum lies within 2.5 * 255 / 16384 < 0.039 of the exact value.  Chroma: kUB and kUR are off by at most 1/2, kUG by at most 1,
 * an operand is at most 255 N under a shift that is log2 N longer: within 2 * 255 / 16384 < 0.032.  So a sample is never more than 1
 * from the rounded float64 value (of the exactly averaged colour, for chroma) and equal to it wherever that value lies further from a
 * half than the bound.  The largest sum of absolute terms is 134 085 120: no sum reaches 2^31.  The chroma clamp is needed: 8 bit full
 * range reaches 256 before it (pure blue).
 *
 * ORDERING.  As fdh_read_pixels and fdh_put_video_frame: the call drains the submit thread, runs on the context's stream behind the
 * frame, and returns after that stream is synchronised: the planes are complete on return and the frame is untouched.
 *
 * REFUSALS.  FDH_ERR_INVALID, nothing written.  fdh_check_video_target applies every rule that needs no device:
 * - a null struct or null planes[0]; null planes[1] for NV12 / P010;
 * - an unknown format, matrix, range or flag; reserved != 0;
 * - BGRA8 with matrix or range != 0, with planes[1] or pitch_bytes[1] set, or with FDH_VIDEO_CHROMA_LINEAR; NV12 / P010 with
 *   FDH_VIDEO_IGNORE_ALPHA; FDH_VIDEO_STRAIGHT_ALPHA with any format (the surface is premultiplied, and nothing divides here);
 * - a rectangle that is not inside the frame; for NV12 / P010 an odd x or y of the rectangle (odd w, h are fine);
 * - a pointer or pitch that is not a multiple of the plane's element size: BGRA8 4; NV12 luma 1, chroma pair 2; P010 luma 2, chroma pair 4;
 * - pitch_bytes[0] below a luma row's bytes; pitch_bytes[1] below cw pairs;
 * - the two planes' byte ranges overlapping each other.
 * fdh_read_video_frame in addition: no frame submitted yet; a record-only context; under fdh_set_stripe; a plane
 * that hipPointerGetAttributes reports as neither device memory of the context's device nor page-locked host memory; a plane that
 * overlaps one of the context's own surfaces or its atlas.
 *
 * ON THE DEVICE.  k_video_export, one launch: a workgroup of 256 per 128 x 16 tile of the rectangle, a lane per run of four texels by
 * two rows -- two 16-byte loads, a 4-byte (NV12) or 8-byte (P010) store per luma row and one for the two chroma pairs, where pointers
 * and pitches allow it. */
#ifndef FIGDRAW_HIP_VIDEO_OUT_H
#define FIGDRAW_HIP_VIDEO_OUT_H
#include "../include_glyphs/figdraw_hip_video_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct FdhVideoTarget {
  void* planes[2];           /* [0] luma, or the BGRA texels; [1] interleaved Cb,Cr (NULL for BGRA8) */
  int64_t pitch_bytes[2];    /* between rows of each plane ([1] is 0 for BGRA8) */
  int32_t rect[4];           /* x, y, w, h of the frame, top-down; w <= 0 or h <= 0: the whole frame */
  uint32_t format, matrix, range, flags;   /* the enums of figdraw_hip_video_frame.h */
  uint32_t reserved[2];      /* 0 */
} FdhVideoTarget;
FDH_API int fdh_read_video_frame(FdhContext*, const FdhVideoTarget*);
/* host only, no context: every rule above that needs no device, for a frame of frame_w x frame_h */
FDH_API int fdh_check_video_target(const FdhVideoTarget*, int frame_w, int frame_h);
/* host only, no context: out = Yoff, Coff, kYR, kYG, kYB, kUR, kUG, kUB, kVR, kVG, kVB for FDH_VIDEO_NV12 or FDH_VIDEO_P010 */
FDH_API int fdh_video_out_coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[11]);

#ifdef __cplusplus
}
#endif
#endif
