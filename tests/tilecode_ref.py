"""The tile code of include/figdraw_hip_stream.h in plain numpy, written from the header's text and from nothing else: the reference the C
decoder (fdh_decode_damage) and the GPU encoder (k_damage_encode) are held against.  A tile is a uint32 array (h, w) of pixels
R | G << 8 | B << 16 | A << 24; everything is little-endian."""
import numpy as np

SOLID, PAL, RUNS, RAW = 0, 1, 2, 3
TILE = 64
ENTRY = np.dtype([("x", "<i2"), ("y", "<i2"), ("w", "<i2"), ("h", "<i2"), ("mode", "u1"), ("bits", "u1"), ("n", "<u2"), ("offset", "<u4"),
                  ("size", "<u4"), ("solid", "<u4")])
assert ENTRY.itemsize == 24


def ceil16(v):
    return (int(v) + 15) // 16 * 16


def pal_bits(n):
    """the smallest of 1, 2, 4, 8 with 2^b >= n"""
    return next(b for b in (1, 2, 4, 8) if (1 << b) >= n)


def as_u32(rgba):
    """uint8 (h, w, 4) -> uint32 (h, w)"""
    return np.ascontiguousarray(rgba, np.uint8).view("<u4")[..., 0]


def as_rgba(px):
    """uint32 (h, w) -> uint8 (h, w, 4)"""
    return np.ascontiguousarray(px, "<u4")[..., None].view(np.uint8)


def _pack_indices(idx, b):
    """pixel i in bits [(i b) % 32, +b) of word (i b) / 32; unused bits zero"""
    words = np.zeros((len(idx) * b + 31) // 32, np.uint64)
    at = np.arange(len(idx), dtype=np.uint64) * np.uint64(b)
    np.bitwise_or.at(words, (at // np.uint64(32)).astype(np.intp), idx.astype(np.uint64) << (at % np.uint64(32)))
    return words.astype("<u4").tobytes()


def _runs(flat):
    """the maximal runs of the tight order -> (colours, lengths)"""
    starts = np.flatnonzero(np.concatenate(([True], flat[1:] != flat[:-1])))
    return flat[starts], np.diff(np.concatenate((starts, [len(flat)])))


def payloads(tile):
    """every mode that can code the tile -> {mode: (n, payload bytes)}"""
    h, w = tile.shape
    assert 1 <= w <= TILE and 1 <= h <= TILE
    flat = np.ascontiguousarray(tile, "<u4").reshape(-1)
    out = {RAW: (0, flat.tobytes())}
    colours, lengths = _runs(flat)
    pad = b"\0\0" if len(colours) % 2 else b""
    out[RUNS] = (len(colours), colours.astype("<u4").tobytes() + (lengths - 1).astype("<u2").tobytes() + pad)
    pal, idx = np.unique(flat, return_inverse=True)  # ascending as unsigned; idx = rank
    if len(pal) == 1:
        out[SOLID] = (0, b"")
    elif len(pal) <= 256:
        out[PAL] = (len(pal), pal.astype("<u4").tobytes() + _pack_indices(idx.reshape(-1), pal_bits(len(pal))))
    return out


def encode(tile):
    """-> (mode, n, solid, payload bytes): the mode with the smallest payload, ties to the lower mode number"""
    cand = payloads(tile)
    mode = min(cand, key=lambda m: (len(cand[m][1]), m))
    n, data = cand[mode]
    h, w = tile.shape
    want = {SOLID: 0, PAL: 4 * n + 4 * ((w * h * (pal_bits(n) if mode == PAL else 0) + 31) // 32), RUNS: 4 * ((6 * n + 3) // 4), RAW: 4 * w * h}[mode]
    assert len(data) == want, "the payload is not the size the header's rule gives"
    return mode, n, int(tile.flat[0]) if mode == SOLID else 0, data


def decode(mode, n, solid, data, w, h):
    """-> uint32 (h, w).  Trusts its input (the C decoder is the one that validates)."""
    if mode == SOLID:
        return np.full((h, w), solid, "<u4")
    if mode == RAW:
        return np.frombuffer(data, "<u4", w * h).reshape(h, w).copy()
    if mode == RUNS:
        colours = np.frombuffer(data, "<u4", n)
        lengths = np.frombuffer(data, "<u2", n, offset=4 * n).astype(np.int64) + 1
        return np.repeat(colours, lengths).reshape(h, w)
    b = pal_bits(n)
    pal = np.frombuffer(data, "<u4", n)
    words = np.frombuffer(data, "<u4", (w * h * b + 31) // 32, offset=4 * n)
    at = np.arange(w * h) * b
    return pal[(words[at // 32] >> (at % 32).astype(np.uint32)) & ((1 << b) - 1)].reshape(h, w)


def tiles_of(w, h):
    """the bins of a w x h frame clipped to it, row-major: (x, y, w, h)"""
    return [(x, y, min(TILE, w - x), min(TILE, h - y)) for y in range(0, h, TILE) for x in range(0, w, TILE)]


def entry(x, y, w, h, mode, n, solid, size, offset):
    e = np.zeros((), ENTRY)
    e["x"], e["y"], e["w"], e["h"] = x, y, w, h
    e["mode"], e["bits"], e["n"] = mode, pal_bits(n) if mode == PAL else 0, n
    e["offset"], e["size"], e["solid"] = 0 if mode == SOLID else offset, size, solid
    return e


def encode_frame(rgba, rects=None):
    """a frame (uint8 (H, W, 4)) -> (directory: ENTRY array, payload blob: bytes); rects: the tiles to code, default every bin.  Payloads
    lie in directory order, each on a multiple of 16 with zeros up to the next."""
    px = as_u32(rgba)
    H, W = px.shape
    rects = tiles_of(W, H) if rects is None else rects
    entries, blob = [], bytearray()
    for x, y, w, h in rects:
        mode, n, solid, data = encode(px[y:y + h, x:x + w])
        entries.append(entry(x, y, w, h, mode, n, solid, len(data), len(blob)))
        blob += data + bytes(ceil16(len(data)) - len(data))
    return np.array(entries, ENTRY).reshape(-1), bytes(blob)


def wire_bytes(directory):
    """24 bytes of directory per tile plus each payload rounded up to 16 bytes"""
    return 24 * len(directory) + sum(ceil16(s) for s in directory["size"].tolist())
