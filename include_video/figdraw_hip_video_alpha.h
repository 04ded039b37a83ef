/* figdraw_hip_video_alpha.h -- video WITH AN ALPHA PLANE in and out of libfigdraw_hip.so: what figdraw_hip_video_planar.h and
 * figdraw_hip_video_422.h do for opaque video, for the formats that carry a key beside the fill -- A420 (ffmpeg's yuva420p), A444
 * (yuva444p), A410 (yuva444p10le) and UYVA (NDI's UYVY plane followed by an alpha plane).  It adds two structs, the planar structs
 * with four slots, and four values to the format enum's space; matrix, range and flag enums are the siblings'.  Same conventions as
 * figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says why).  -I include_video is all a caller
 * adds.
 *
 * Why.  The library renders premultiplied RGBA8, and its most common non-opaque output is an overlay -- a lower third, a scoreboard, a
 * HUD over a clear with alpha 0 -- that a mixer or an encoder composites over video.  Every sibling drops the alpha byte on the way out
 * and stores A = 255 on the way in; BGRA8, the one route that keeps alpha, is four bytes a texel and no codec, NDI sender or key / fill
 * chain takes it.  VP9 / AV1 alpha decode to yuva420p, ProRes 4444 to yuva444p10le, NDI hands out UYVA: YUV planes plus an alpha plane.
 * Without these calls an overlay caller restates the colour arithmetic in a kernel of their own, or loses the key.
 *
 * This comment is the specification.  tests/video_alpha_ref.py restates it in numpy and the device
 * (figdraw_amd/csrc/k_video_alpha_import.hip, k_video_alpha_export.hip) is held to it byte for byte.
 *
 * THE PLANES.  planes[0 .. 2] are the base format's, planes[3] is A: one sample per texel, w x h, rows pitch_bytes[3] apart.
 * - FDH_VIDEO_A420: I420's three planes (figdraw_hip_video_planar.h) and A of w x h bytes; b = 8.
 * - FDH_VIDEO_A444: I444's three planes and A of w x h bytes; b = 8.
 * - FDH_VIDEO_A410: I410's three planes and A of w x h little-endian 16-bit words with their 10 bits at the BOTTOM; b = 10.
 * - FDH_VIDEO_UYVA: planes[0] is a UYVY plane (figdraw_hip_video_422.h: cw = ceil(w / 2) four-byte groups Cb Y0 Cr Y1 a row, an odd
 *   width's last group as that header has it), planes[3] is A of w x h bytes; planes[1], planes[2], pitch_bytes[1] and pitch_bytes[2]
 *   must be 0; b = 8.  NDI's buffer is the UYVY plane with the alpha plane right behind it, one block.
 *
 * THE ALPHA SAMPLE.  All arithmetic is int32; `/` is floor division of non-negative numbers.  A is the alpha byte of a texel.
 * - 8-bit formats: the sample is the byte, both ways.
 * - A410 out: a10 = (1023 A + 127) / 255; the six high bits of the word are written as 0.
 * - A410 in:  a10 = word & 1023 (the six high bits are ignored), A = (255 a10 + 511) / 1023.
 * Both are the exact rational rounded to nearest -- floor((2 p x + q) / (2 q)) = floor((p x + (q - 1) / 2) / q) for odd q --, and no
 * tie exists because 255 and 1023 are odd.  |a10 - 1023 A / 255| <= 1/2 gives |255 a10 / 1023 - A| <= 255 / 2046 < 1/2: 8 -> 10 -> 8
 * is the identity.
 *
 * THE WAY IN: fdh_put_video_alpha, fdh_update_video_alpha.  Y, Cb, Cr become R, G, B by the arithmetic of figdraw_hip_video_frame.h,
 * word for word -- CONVERSION, the coefficients (the NV12 row for b = 8, the P010 row for b = 10; fdh_video_coefficients), the chroma for
 * a luma texel: A420 takes I420's two rules (repeat, or FDH_VIDEO_CHROMA_LINEAR), UYVA takes UYVY's two rules, A444 and A410 take
 * c[y][x].  A is the alpha sample of texel (x, y) itself: alpha is never interpolated.
 * - without FDH_VIDEO_STRAIGHT_ALPHA the converted colour is taken as premultiplied and stored as converted (BGRA8's rule in
 *   figdraw_hip_video_frame.h); nothing clamps it to A;
 * - with it each colour byte becomes (c * A) / 255, the rule of FDH_IMAGE_STRAIGHT_ALPHA.
 * WHAT IS STORED is exactly what fdh_put_image / fdh_update_image store of the converted RGBA8 bytes: placement, keep mode and growth,
 * every level, the ink boxes, the epoch, an update turning an entry into a chain entry.  It follows that a frame whose alpha plane is
 * all 255 (1023 for A410) leaves, under either setting of the flag, byte for byte what the sibling call leaves of the first three
 * planes: fdh_put_video_planes for I420 / I444 / I410, fdh_put_video_422 for UYVY.
 *
 * THE WAY OUT: fdh_read_video_alpha.  THE SOURCE, the rectangle rule (rect x, y, w, h; w <= 0 or h <= 0: the whole frame; every clamp
 * is to the rectangle), the luma formula, the chroma formula and the coefficients are those of figdraw_hip_video_out.h
 * (fdh_video_out_coefficients).  The chroma rules -- which texels a sample takes, with which weights w_k, summing to N -- are each
 * base format's own: A420 uses I420's two (N = 4, or 8 with FDH_VIDEO_CHROMA_LINEAR), UYVA uses UYVY's (N = 2, or 4), A444 and A410
 * have N = 1, the texel.  The alpha plane takes the alpha sample of every texel of the rectangle.
 * - Without FDH_VIDEO_STRAIGHT_ALPHA the surface's colour bytes go out as stored: a "shaped" fill, what a premultiplied key / fill mixer
 *   and NDI expect.  Planes 0 .. 2 are then, byte for byte, the sibling export (fdh_read_video_planes, fdh_read_video_422) of the same
 *   frame, target and flags, and plane 3 is fdh_read_pixels' alpha bytes, or their a10.
 * - With it the colour is un-premultiplied first: what VP9 / AV1 alpha and most ProRes 4444 consumers expect.  One rule covers every
 *   sample.  Per channel, with c_k the stored premultiplied bytes and a_k the alpha bytes of the sample's texels,
 *       sc = sum of w_k c_k,   sa = sum of w_k a_k,
 *       s  = (sa == 0) ? 0 : min(255 N, (510 N sc + sa) / (2 sa))
 *   which is N times the alpha-weighted average straight colour, (sum of w_k a_k u_k) / sa with u_k = 255 c_k / a_k, rounded half up:
 *   N * 255 sc / sa + 1/2 = (510 N sc + sa) / (2 sa).  A transparent neighbour adds nothing to either sum, so the edges of text get no
 *   dark chroma fringe.  For N = 1 this is the texel's straight byte u = min(255, (510 c + a) / (2 a)), and 0 at a = 0.  Luma is the
 *   sibling's luma formula of the texel's (u_R, u_G, u_B); chroma is the sibling's one chroma formula of s, with the same N, shift and
 *   clamp.  The min is needed: nothing guarantees c <= a on the surface.  The largest numerator is 510 * 8 * 2040 + 2040, below 2^24.
 *   With every a = 255, sa = 255 N and s = (510 N sc + 255 N) / (510 N) = sc: on an opaque frame the straight export is the
 *   premultiplied export, which is the sibling's.
 * The bound.  u lies within 1/2 of 255 c / a (clamped).  Given the 8-bit straight colour, luma and 4:4:4 chroma are the siblings'
 * formulas of a byte and carry their bounds unchanged: the unrounded chroma value lies within 2 * 255 / 16384 < 0.032 of the exact value
 * of that colour.  A subsampled s lies within 1/2, in units of 1/N byte, of the exact N-fold weighted average, each channel on its own; the absolute
 * values of a chroma row's three coefficients sum to one sample per byte in the full range of an 8-bit format (1/2 + 1/2; less in the
 * limited range), so that is at most 0.5 / N <= 0.25 of a sample on top of the sibling's 0.032.  So a sample is never more than 1 from
 * the rounded float64 value of the exactly un-premultiplied weighted average, and equal to it wherever that lies further from a half
 * than 0.032 + 0.5 / N.
 * The limit of the straight path: the straight colour is an 8-bit quantity, so A410 out of an 8-bit surface carries no more than that.
 * The bound above holds for A410 given the 8-bit straight colour u; against the exactly un-premultiplied colour its samples lie within
 * 0.5 * 1023 / 255 + 0.032 < 2.04 before rounding, a byte being 4.01 ten-bit samples.
 *
 * ORDERING.  As the siblings.  The way in reads the planes on the context's stream and returns after that stream is synchronised: the
 * planes may be reused on return.  The way out drains the submit thread, runs behind the frame and returns after a synchronise: the
 * planes are complete on return and the frame is untouched.  The bytes between a row's end and the pitch are never written; at an odd
 * width the last UYVY group is written whole, as fdh_read_video_422 writes it.
 *
 * REFUSALS.  FDH_ERR_INVALID, with nothing placed (no entry, no epoch bump, the packer untouched) or written:
 * - a null struct; a null planes[0] or planes[3]; for A420 / A444 / A410 a null planes[1] or planes[2]; for UYVA any of planes[1],
 *   planes[2], pitch_bytes[1], pitch_bytes[2] set;
 * - a format outside FDH_VIDEO_A420 .. FDH_VIDEO_UYVA; an unknown matrix, range or flag; reserved != 0;
 * - FDH_VIDEO_IGNORE_ALPHA (that is the sibling call); FDH_VIDEO_CHROMA_LINEAR with A444 or A410;
 * - a pointer or pitch that is not a multiple of the element size (1; 2 for A410; 4, the group, for the UYVY plane); a pitch below a
 *   row's bytes;
 * - on the way in: width or height <= 0; fdh_update_video_alpha: an unknown key, or a size that is not the entry's;
 * - on the way out: a rectangle that is not inside the frame; an odd x or y of the rectangle for A420; an odd x for UYVA; any two of the
 *   planes' byte ranges overlapping;
 * - fdh_read_video_alpha in addition: no frame submitted yet, a record-only context, a context under fdh_set_stripe;
 * - on a context with a device: a plane that hipPointerGetAttributes reports as neither device memory of the context's device nor
 *   page-locked host memory; a plane that overlaps one of the context's own surfaces (the way out) or its atlas (both ways).
 * NDI's contiguous UYVA buffer does not overlap itself and passes.  On the way in the planes may alias each other: they are only read.
 * A record-only context validates and places, touches no memory and sets no ink boxes.  fdh_check_video_alpha_target applies every rule
 * of the way out that needs no device.  The four older families keep refusing every format value from FDH_VIDEO_A420 on, and these
 * calls refuse every value outside FDH_VIDEO_A420 .. FDH_VIDEO_UYVA.
 *
 * NOT HERE.  A010 / A422 / A210, NV12 plus an alpha plane, packed AYUV / VUYA / Y410, a limited-range key signal, transfer functions,
 * and calls that do not wait for the stream.
 *
 * ON THE DEVICE.  One kernel each way, a lane per run of EIGHT texels.  The way in, k_video_alpha_import: a workgroup of 128 per
 * 32 x 32 tile of the image, the base format's loads and one more of the run's alpha samples; level 0 goes to the atlas, the tile
 * through LDS down to one texel; k_image_import_tail finishes the chain.  The way out, k_video_alpha_export: a workgroup of 256 per
 * 256 x 16 tile for A420 (a lane takes its run in two rows), per 256 x 8 tile for the others (one row); the alpha run is packed from
 * the texels already in registers.  The straight quotient is the language's integer division. */
#ifndef FIGDRAW_HIP_VIDEO_ALPHA_H
#define FIGDRAW_HIP_VIDEO_ALPHA_H
#include "figdraw_hip_video_422.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FDH_VIDEO_A420 = 11,   /* I420's three planes and A, w x h bytes (yuva420p) */
       FDH_VIDEO_A444 = 12,   /* I444's three planes and A, w x h bytes (yuva444p) */
       FDH_VIDEO_A410 = 13,   /* I410's three planes and A, w x h 16-bit words, 10 bits at the bottom (yuva444p10le) */
       FDH_VIDEO_UYVA = 14 }; /* planes[0] a UYVY plane, planes[3] A, w x h bytes (NDI) */
typedef struct FdhVideoAlphaPlanes {
  const void* planes[4];     /* Y, Cb, Cr, A */
  int64_t pitch_bytes[4];    /* between rows of each plane */
  int32_t width, height;     /* of the luma and of the alpha plane */
  uint32_t format, matrix, range, flags;
  uint32_t reserved[2];      /* 0 */
} FdhVideoAlphaPlanes;
typedef struct FdhVideoAlphaPlanesTarget {
  void* planes[4];           /* Y, Cb, Cr, A */
  int64_t pitch_bytes[4];    /* between rows of each plane */
  int32_t rect[4];           /* x, y, w, h of the frame, top-down; w <= 0 or h <= 0: the whole frame */
  uint32_t format, matrix, range, flags;
  uint32_t reserved[2];      /* 0 */
} FdhVideoAlphaPlanesTarget;
/* out_rect = the packed rectangle x, y, w, h (may be NULL) */
FDH_API int fdh_put_video_alpha(FdhContext*, int64_t key, const FdhVideoAlphaPlanes*, int out_rect[4]);
/* new texels for an entry of the same size */
FDH_API int fdh_update_video_alpha(FdhContext*, int64_t key, const FdhVideoAlphaPlanes*);
FDH_API int fdh_read_video_alpha(FdhContext*, const FdhVideoAlphaPlanesTarget*);
/* host only, no context: every rule of the way out that needs no device, for a frame of frame_w x frame_h */
FDH_API int fdh_check_video_alpha_target(const FdhVideoAlphaPlanesTarget*, int frame_w, int frame_h);

#ifdef __cplusplus
}
#endif
#endif
