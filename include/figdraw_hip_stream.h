/* figdraw_hip_stream.h -- coded damage readback for libfigdraw_hip.so: the pending bins of damage readback (figdraw_hip_readback.h),
 * coded losslessly on the GPU so that only the coded bytes cross the link -- and whatever lies behind the host: a socket, a pipe, a
 * recorder.  A host-only decoder rebuilds the frame on any machine.  Same conventions as figdraw_hip.h (plain C, every call returns 0
 * or a negative FdhStatus, fdh_last_error() says why).  No counterpart in the reference.  THIS HEADER IS THE SPECIFICATION OF THE FORMAT.
 *
 * Pixels are little-endian uint32 values R | G << 8 | B << 16 | A << 24; every multi-byte field below is little-endian.
 *
 * Tiles.  A tile is a bin (bx, by) clipped to the frame, as in figdraw_hip_readback.h: x = 64 bx, y = 64 by, w = min(64, W - x),
 * h = min(64, H - y), 1 <= w, h <= 64.  Its pixels are taken TIGHT in row-major order: pixel i is row i / w, column i % w of the tile;
 * there is no pitch padding.  Each tile is coded on its own, in the mode with the smallest payload; ties go to the lower mode number.
 *
 *   0 FDH_TILE_SOLID  one colour.  No payload: the colour is the entry's `solid`.
 *   1 FDH_TILE_PAL    n distinct colours, 2 <= n <= 256.  Payload: the n colours in ascending order as unsigned uint32; then the
 *                     pixels' indices (a colour's rank in that order) at b bits per pixel, b the smallest of 1, 2, 4, 8 with
 *                     2^b >= n: pixel i in bits [(i b) % 32, (i b) % 32 + b) of 32-bit word (i b) / 32; ceil(w h b / 32) words, unused
 *                     bits zero.  size = 4 n + 4 ceil(w h b / 32).
 *   2 FDH_TILE_RUNS   n maximal runs over the tight order (a run may cross a row end; neighbouring runs differ in colour).  Payload:
 *                     the n colours, then n uint16 values of length - 1, zero-padded to a multiple of 4 bytes.
 *                     size = 4 ceil(6 n / 4).
 *   3 FDH_TILE_RAW    the w h pixels, tight.  size = 4 w h.
 *
 * The palette order and the runs are canonical: a tile's entry (mode, bits, n, size, solid) and its payload bytes are a function of
 * its pixels alone -- a receiver can hash what it gets, and the tests compare bytes.
 *
 * The directory is one FdhCodedTile of 24 bytes per tile, in row-major bin order (the order fdh_read_damage lists tiles in).  `offset`
 * is where the tile's payload starts in the payload blob, a multiple of 16; payloads do not overlap and need not lie in directory order
 * (on the GPU a workgroup claims its space with one atomic add).  Each payload occupies its size rounded up to 16 bytes; the bytes of
 * that round-up are zero, and payload_bytes is the end of the last space claimed, so the blob has no byte that was not written.  A
 * field that a mode does not use is zero: bits outside PAL, n outside PAL and RUNS, solid outside SOLID, offset and size for SOLID.
 *
 * On a wire: { frame_w, frame_h, n_tiles, payload_bytes }, then the directory, then payload[0 .. payload_bytes).  As in
 * figdraw_hip_readback.h, a mirror image that receives every fdh_read_damage_coded through fdh_decode_damage is, after each, bit for
 * bit what fdh_read_pixels returns for the whole frame. */
#ifndef FIGDRAW_HIP_STREAM_H
#define FIGDRAW_HIP_STREAM_H
#include "figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FDH_TILE_SOLID = 0, FDH_TILE_PAL = 1, FDH_TILE_RUNS = 2, FDH_TILE_RAW = 3 };
typedef struct FdhCodedTile {
  int16_t x, y, w, h; /* the tile, in top-down pixels */
  uint8_t mode;       /* FDH_TILE_* */
  uint8_t bits;       /* PAL: bits per index (1, 2, 4, 8); else 0 */
  uint16_t n;         /* PAL: colours (2 .. 256); RUNS: runs (2 .. 4096); else 0 */
  uint32_t offset;    /* of the payload in the blob, a multiple of 16 */
  uint32_t size;      /* of the payload in bytes, as the mode's rule above gives it */
  uint32_t solid;     /* SOLID: the colour; else 0 */
} FdhCodedTile;

/* Needs fdh_set_damage_readback(ctx, 1).  The third way to read the pending set, beside fdh_read_damage / fdh_read_damage_into and over
 * the same set: waits for the last submitted frame, codes the pending bins (k_damage_encode: one launch, which stores the directory and
 * the payloads straight into page-locked host memory the context owns -- sized once for the whole grid, 24 + 16384 bytes per bin -- and
 * freed by fdh_set_damage_readback(ctx, 0) and fdh_destroy), and empties the set: each read, of whichever kind, returns the bins pending
 * since the previous read of any kind.  *n_tiles = 0 is a valid answer (nothing changed): nothing is launched then and *payload_bytes is
 * 0.  *full: 1 when every bin of the grid is among the tiles.  The pointers stay valid until the next read of any of the three kinds on
 * this context, fdh_set_damage_readback(ctx, 0) or fdh_destroy; submitting further frames does not invalidate them.  The memory is
 * page-locked: send or copy out of it, do not compute in it.  Any out-pointer may be NULL.  FDH_ERR_NO_DEVICE on a record-only context;
 * FDH_ERR_INVALID before the first frame, while the mode is off, or for a frame wider or higher than 32767 pixels. */
FDH_API int fdh_read_damage_coded(FdhContext*, const FdhCodedTile** tiles, const uint8_t** payload, int* n_tiles, int64_t* payload_bytes,
                                  int* frame_w, int* frame_h, int* full);
/* Host only (no context, no device: the receiver's side): decode the tiles into a top-down RGBA8 image of w x h pixels with row pitch
 * pitch_bytes; no other byte of the image is touched.  The stream may come from anywhere: EVERYTHING is validated before the first byte
 * is written, nothing outside tiles[0 .. n_tiles) and payload[0 .. payload_bytes) is read, and FDH_ERR_INVALID leaves the image as it
 * was.  Refused: a null image / tiles with n_tiles > 0, a null payload with payload_bytes > 0, n_tiles < 0, payload_bytes < 0,
 * pitch_bytes < 4 w; a tile with w or h outside 1 .. 64 or not inside the image; a mode above 3; PAL with n outside 1 .. 256 or bits
 * that are not the smallest of 1, 2, 4, 8 with 2^bits >= n; RUNS with n outside 1 .. w h; a field that the mode does not use and that
 * is not zero; a size that is not what (mode, n, w, h) give; an offset that is not a multiple of 16, or offset + size > payload_bytes;
 * a palette index >= n; run lengths that do not sum to w h.  A stream that is decodable but not canonical (an unsorted palette, split
 * runs, a mode that is not the smallest) is accepted. */
FDH_API int fdh_decode_damage(uint8_t* image_rgba8, int64_t pitch_bytes, int w, int h,
                              const FdhCodedTile* tiles, int n_tiles, const uint8_t* payload, int64_t payload_bytes);
/* Host only: an upper bound of payload_bytes for a w x h frame -- 16384 bytes per bin of its grid -- that a receiver may size its
 * buffer with; 0 when w or h is not positive. */
FDH_API int64_t fdh_coded_damage_bound(int w, int h);

#ifdef __cplusplus
}
#endif
#endif
