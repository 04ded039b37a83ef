"""Stream version 2 and the mover of include_readback/figdraw_hip_moves.h in plain numpy, written from that header's text and from nothing
else: the reference fdh_decode_damage_moved, k_damage_move_match / k_damage_encode_moved and k_damage_move_votes are held against.  Modes
0 .. 3 are tests/tilecode_ref.py's.  Frames are uint8 (H, W, 4); a move is (dx, dy): tile (x, y) now holds what (x + dx, y + dy) held."""
import numpy as np

import tilecode_ref as T

COPY = 4
MOVES_MAX, SHIFT_MAX = 8, 256


def move_word(dx, dy):
    """a COPY entry's `solid`: (uint16_t)dx | (uint32_t)(uint16_t)dy << 16"""
    return (int(dx) & 0xFFFF) | (int(dy) & 0xFFFF) << 16


def word_move(solid):
    dx, dy = int(solid) & 0xFFFF, int(solid) >> 16 & 0xFFFF
    return dx - 0x10000 if dx >= 0x8000 else dx, dy - 0x10000 if dy >= 0x8000 else dy


def copy_entry(x, y, w, h, dx, dy):
    e = np.zeros((), T.ENTRY)
    e["x"], e["y"], e["w"], e["h"], e["mode"], e["solid"] = x, y, w, h, COPY, move_word(dx, dy)
    return e


def matching_move(old_px, tile, x, y, moves):
    """the first move in order whose source rectangle lies inside the frame and equals the tile -> its index, or None"""
    H, W = old_px.shape
    h, w = tile.shape
    for k, (dx, dy) in enumerate(moves):
        sx, sy = x + dx, y + dy
        if sx < 0 or sy < 0 or sx + w > W or sy + h > H:
            continue
        if np.array_equal(old_px[sy:sy + h, sx:sx + w], tile):
            return k
    return None


def encode_frame_moved(old, new, moves, tiles):
    """the tiles (x, y, w, h) of frame `new`, coded against `old` (the image the receiver holds) and the moves
    -> (directory: ENTRY array, payload blob: bytes in directory order, the number of COPY tiles)"""
    old_px, new_px = T.as_u32(old), T.as_u32(new)
    assert old_px.shape == new_px.shape and len(moves) <= MOVES_MAX and all((dx, dy) != (0, 0) for dx, dy in moves)
    entries, blob, copied = [], bytearray(), 0
    for x, y, w, h in tiles:
        tile = new_px[y:y + h, x:x + w]
        one_colour = bool((tile == tile.flat[0]).all())  # SOLID: its payload is as empty as COPY's, and it is the lower mode
        k = None if one_colour else matching_move(old_px, tile, x, y, moves)
        if k is not None:
            entries.append(copy_entry(x, y, w, h, *moves[k]))
            copied += 1
            continue
        mode, n, solid, data = T.encode(tile)
        entries.append(T.entry(x, y, w, h, mode, n, solid, len(data), len(blob)))
        blob += data + bytes(T.ceil16(len(data)) - len(data))
    return np.array(entries, T.ENTRY).reshape(-1), bytes(blob), copied


def decode_moved(image, directory, blob):
    """decodes into `image` in place.  Every COPY source is the image as it was before the call (a snapshot).  Trusts its input."""
    before = T.as_u32(image).copy()
    out = T.as_u32(image).copy()
    for e in directory:
        x, y, w, h = (int(e[f]) for f in "xywh")
        if e["mode"] == COPY:
            dx, dy = word_move(e["solid"])
            out[y:y + h, x:x + w] = before[y + dy:y + dy + h, x + dx:x + dx + w]
        else:
            off = int(e["offset"])
            out[y:y + h, x:x + w] = T.decode(int(e["mode"]), int(e["n"]), int(e["solid"]), blob[off:off + int(e["size"])], w, h)
    image[...] = T.as_rgba(out)


def votes(old, new, pending_bins, max_shift):
    """-> (Vv, Vh): dicts d -> votes, as the header defines them.  pending_bins: (bins_y, bins_x) bool"""
    old_px, new_px = T.as_u32(old), T.as_u32(new)
    H, W = new_px.shape
    Vv, Vh = {}, {}
    for by, bx in zip(*np.nonzero(pending_bins)):
        x0, y0 = 64 * int(bx), 64 * int(by)
        if x0 + 64 > W or y0 + 64 > H:
            continue  # the tile is not whole: no probes
        probe = new_px[y0 + 32, x0:x0 + 64]
        if (probe != probe[0]).any():
            for d in range(-max_shift, max_shift + 1):
                y = y0 + 32 + d
                if d != 0 and 0 <= y < H and np.array_equal(probe, old_px[y, x0:x0 + 64]):
                    Vv[d] = Vv.get(d, 0) + 1
        probe = new_px[y0:y0 + 64, x0 + 32]
        if (probe != probe[0]).any():
            for d in range(-max_shift, max_shift + 1):
                x = x0 + 32 + d
                if d != 0 and 0 <= x < W and np.array_equal(probe, old_px[y0:y0 + 64, x]):
                    Vh[d] = Vh.get(d, 0) + 1
    return Vv, Vh


def find_moves(old, new, pending_bins, max_shift):
    """-> [((dx, dy), votes)]: votes descending, then |d| ascending, then vertical before horizontal, then negative d first"""
    Vv, Vh = votes(old, new, pending_bins, max_shift)
    cands = [(-v, abs(d), 0, d) for d, v in Vv.items()] + [(-v, abs(d), 1, d) for d, v in Vh.items()]
    return [(((d, 0) if hz else (0, d)), -nv) for nv, _, hz, d in sorted(cands)]
