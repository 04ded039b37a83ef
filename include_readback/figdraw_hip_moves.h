/* figdraw_hip_moves.h -- moved damage readback for libfigdraw_hip.so: coded damage readback (figdraw_hip_stream.h) with a fifth tile
 * mode, COPY, for content that scrolled -- a tile that equals a shifted rectangle of the image the receiver already holds crosses the
 * link as its 24-byte directory entry and nothing else -- and a mover that finds a frame's scroll vectors on the GPU.  Same conventions
 * as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says why).  No counterpart in the reference.
 * THIS HEADER IS THE SPECIFICATION OF WHAT IT ADDS TO THE FORMAT OF figdraw_hip_stream.h.
 *
 * Stream version 2 = the modes 0 .. 3 of figdraw_hip_stream.h exactly as they are, plus
 *
 *   4 FDH_TILE_COPY   the tile's pixels are the pixels of the rectangle (x + dx, y + dy, w, h) of the image AS THE RECEIVER HELD IT BEFORE
 *                     THIS READ.  That rectangle lies wholly inside the frame.  No payload: bits = n = offset = size = 0, and
 *                     solid = (uint16_t)dx | (uint32_t)(uint16_t)dy << 16 (two's complement, 16 bits each).
 *
 * The rule of version 1 stands: the smallest payload wins, ties go to the lower mode number.  A one-colour tile is therefore SOLID,
 * never COPY; any other tile that matches a move is COPY.  Among the moves the caller gives, the first in array order whose source
 * rectangle lies inside the frame and equals the tile wins.  The stream stays canonical: entries and payload bytes are a function of the
 * new tile, the previous image and the move list.
 *
 * The wire header { frame_w, frame_h, n_tiles, payload_bytes } gains nothing: A RECEIVER MUST KNOW THAT IT IS READING VERSION 2 (it asked
 * for it: fdh_read_damage_moved is the only producer), and decodes it with fdh_decode_damage_moved; fdh_decode_damage refuses mode 4.
 * Every COPY source is read from the image as it was before the decode, and a source may overlap tiles the same stream writes (a scroll
 * by 17 rows: every tile's source reaches into the tile below), so a decoder stages the sources first.
 *
 * The device mirror exact damage readback keeps (figdraw_hip_exact.h) is the image the receiver holds; moved reads need that mode. */
#ifndef FIGDRAW_HIP_MOVES_H
#define FIGDRAW_HIP_MOVES_H
#include "../include/figdraw_hip_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct FdhDamageMove { int16_t dx, dy; } FdhDamageMove; /* tile (x, y) now holds what (x + dx, y + dy) held */
enum { FDH_TILE_COPY = 4 };
#define FDH_DAMAGE_MOVES_MAX 8   /* moves a read takes */
#define FDH_DAMAGE_SHIFT_MAX 256 /* the largest |d| the mover probes */

/* Needs fdh_set_damage_readback(ctx, 1) and fdh_set_damage_exact(ctx, 1).  The fourth kind of read over the same pending set: the tiles
 * are exact mode's tiles -- the bins whose pixels changed, in row-major order -- coded in version 2 against moves[0 .. n_moves).  Three
 * launches: k_damage_move_match compares each pending tile with the mirror at each move (before the filter, which overwrites the mirror),
 * k_damage_filter as it is, k_damage_encode_moved.  *n_copied: the COPY tiles among *n_tiles.  With n_moves = 0, or on a fresh read (no
 * valid mirror: the first read, another frame size, after a lost read), the answer is byte for byte fdh_read_damage_coded's and
 * *n_copied = 0.  Pointer lifetime, the emptying of the pending set and the lost-read rule are those of fdh_read_damage_coded and
 * figdraw_hip_exact.h.  Any out-pointer may be NULL.  FDH_ERR_NO_DEVICE on a record-only context.  FDH_ERR_INVALID -- the pending set
 * and the mirror stay as they were -- before the first frame, while either mode is off, for n_moves outside 0 .. FDH_DAMAGE_MOVES_MAX,
 * null moves with n_moves > 0, a move of (0, 0), or a frame wider or higher than 32767 pixels. */
FDH_API int fdh_read_damage_moved(FdhContext*, const FdhDamageMove* moves, int n_moves, const FdhCodedTile** tiles, const uint8_t** payload,
                                  int* n_tiles, int64_t* payload_bytes, int* frame_w, int* frame_h, int* full, int* n_copied);
/* Host only: fdh_decode_damage with mode 4 accepted, under the same promise -- EVERYTHING is validated before the first byte is written,
 * FDH_ERR_INVALID leaves the image as it was.  Refused beyond what fdh_decode_damage refuses: a COPY entry with a non-zero bits, n,
 * offset or size, or whose source rectangle (x + dx, y + dy, w, h) is not inside the image.  A move of (0, 0) is accepted: decodable,
 * not canonical.  Every COPY source is taken from the image as it was before the call. */
FDH_API int fdh_decode_damage_moved(uint8_t* image_rgba8, int64_t pitch_bytes, int w, int h,
                                    const FdhCodedTile* tiles, int n_tiles, const uint8_t* payload, int64_t payload_bytes);
/* The mover.  Needs both modes, as the read does.  Compares the surface of the last submitted frame with the mirror over the pending set
 * as it stands, and changes neither (k_damage_move_votes: one launch).  Votes are integers:
 *   - the probing bins are the pending bins whose tile is whole (64 x 64); (x0, y0) is such a tile's corner;
 *   - its vertical probe is the 64 pixels (x0 .. x0 + 63, y0 + 32) of the frame; it counts only if they are not all equal.  For each d
 *     in [-max_shift, max_shift], d != 0, with row y0 + 32 + d inside the frame: Vv[d] gains 1 when the probe equals the mirror's pixels
 *     (x0 .. x0 + 63, y0 + 32 + d);
 *   - its horizontal probe is the 64 pixels (x0 + 32, y0 .. y0 + 63), under the same rule, compared with the mirror's column
 *     x0 + 32 + d: Vh[d].
 * The candidates are (0, d) with Vv[d] > 0 and (d, 0) with Vh[d] > 0, ordered by votes descending, then |d| ascending, then vertical
 * before horizontal, then negative d first.  The first min(cap, count) go to out_moves / out_votes, and *n_out says how many.  With no
 * valid mirror or nothing pending *n_out = 0 and nothing is launched.  Votes only propose: the read confirms every COPY tile pixel for
 * pixel, so a wrong proposal costs time, never correctness.  FDH_ERR_INVALID for max_shift outside 1 .. FDH_DAMAGE_SHIFT_MAX, cap < 0,
 * null arrays with cap > 0, or either mode off; FDH_ERR_NO_DEVICE on a record-only context. */
FDH_API int fdh_find_damage_moves(FdhContext*, int max_shift, FdhDamageMove* out_moves, int* out_votes, int cap, int* n_out);

#ifdef __cplusplus
}
#endif
#endif
