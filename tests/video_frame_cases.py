"""The frames that the video-frame tests share (tests/test_video_frame_host.py: the kernel's source under the host shim;
tests/test_video_frame.py: the device): sizes at which the tile, the chroma plane's odd edge, the chain and the ink limit change their way;
seeded noise in every plane and a few structured frames; memory layouts that allow the one-load runs and layouts that force the
element-by-element loads.  A covering set over three formats, three matrices, both ranges, both upsamplings and the BGRA8 flags, not their
product.  A case is (name, format, matrix, range, flags, luma, chroma, layout); luma and chroma are what video_frame_ref.convert takes."""
import numpy as np

import video_frame_ref as REF

SIZES = [(1, 1), (1, 9),                  # nothing stored
         (2, 2), (3, 3), (5, 7),          # odd both ways: the last chroma pair serves one column / row
         (32, 32),                        # one full tile
         (33, 31),                        # a run cut by the right edge; CHROMA_LINEAR clamps across a tile edge
         (34, 66), (64, 64),
         (127, 129),                      # no ink boxes by one row
         (128, 128),                      # ink boxes, 16 tiles
         (130, 70)]
LARGEST = (514, 258)  # a level-5 image of 17 x 9: the only case that the sanitizer build of the shim leaves out
LAYOUTS = ("tight", "padded")  # padded: pitches and pointers that are multiples of the element size and of nothing more
# (format, matrix, range, flags), dealt out over sizes x layouts: every NV12 / P010 combination of matrix, range and upsampling occurs
YUV_KINDS = [(f, m, r, l) for f in (REF.NV12, REF.P010) for m in (REF.BT601, REF.BT709, REF.BT2020) for r in (REF.LIMITED, REF.FULL) for l in (0, REF.CHROMA_LINEAR)]
BGRA_FLAGS = (0, REF.STRAIGHT_ALPHA, REF.IGNORE_ALPHA)


def noise_yuv(rng, fmt, w, h):
    """every sample value, those below Yoff and above Yoff + Yden among them; P010: garbage in the six low bits"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if fmt == REF.NV12:
        return rng.integers(0, 256, size=(h, w)).astype(np.uint8), rng.integers(0, 256, size=(ch, cw, 2)).astype(np.uint8)
    return rng.integers(0, 65536, size=(h, w)).astype(np.uint16), rng.integers(0, 65536, size=(ch, cw, 2)).astype(np.uint16)


def noise_bgra(rng, w, h):
    img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
    kind = rng.integers(0, 4, size=(h, w))
    img[kind == 0, 3] = 255
    img[kind == 1] = 0
    return img


def structured(fmt, w, h):
    """-> [(what, luma, chroma)]: a chroma checkerboard of the extreme values under mid grey; a luma ramp through every value (below Yoff
    and above Yoff + Yden) under neutral chroma; planes of one value each"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    dt, top, shift = (np.uint8, 255, 0) if fmt == REF.NV12 else (np.uint16, 1023, 6)
    jj, ii = np.mgrid[0:ch, 0:cw]
    board = np.where((ii + jj) & 1, top, 0)
    checker = np.stack([board, top - board], axis=2)
    ramp = (np.arange(w * h).reshape(h, w) * 7) % (top + 1)
    mid, neutral = np.full((h, w), (top + 1) // 2), np.full((ch, cw, 2), (top + 1) // 2)
    equal = np.stack([np.full((ch, cw), 90 << (2 if shift else 0)), np.full((ch, cw), 240 << (2 if shift else 0))], axis=2)
    out = [("chroma checkerboard", mid, checker), ("luma ramp", ramp, neutral), ("equal planes", np.full((h, w), 81 << (2 if shift else 0)), equal)]
    return [(what, (y << shift).astype(dt), (c << shift).astype(dt)) for what, y, c in out]


def cases(largest=True, again=False):
    """`again`: the same list with other noise in it, case for case of the same size, format and layout (what an update brings)"""
    rng = np.random.default_rng(20261022 if again else 20261021)
    out = []
    n = 0
    for w, h in SIZES + ([LARGEST] if largest else []):
        for layout in LAYOUTS:
            fmt, matrix, rgn, flags = YUV_KINDS[(n * 7) % len(YUV_KINDS)]  # (7 and 24 are coprime: the first 24 cases take every kind)
            luma, chroma = noise_yuv(rng, fmt, w, h)
            out.append((f"noise {w} x {h} {'NV12' if fmt == REF.NV12 else 'P010'} m{matrix} r{rgn} f{flags} {layout}", fmt, matrix, rgn, flags, luma, chroma, layout))
            n += 1
    assert n >= len(YUV_KINDS)
    for k, (w, h) in enumerate(((3, 3), (33, 31), (64, 64), (130, 70), (32, 32), (5, 7))):
        out.append((f"noise {w} x {h} BGRA8 f{BGRA_FLAGS[k % 3]} {LAYOUTS[k & 1]}", REF.BGRA8, 0, 0, BGRA_FLAGS[k % 3], noise_bgra(rng, w, h), None, LAYOUTS[k & 1]))
    for k, fmt in enumerate((REF.NV12, REF.P010)):
        for m, (what, luma, chroma) in enumerate(structured(fmt, 33, 31)):
            for flags in (0, REF.CHROMA_LINEAR):
                out.append((f"{what} {'NV12' if fmt == REF.NV12 else 'P010'} f{flags}", fmt, (m + k) % 3, (m + k + flags) & 1, flags, luma, chroma, LAYOUTS[(m + flags) & 1]))
    # a tile whose runs are whole and aligned, under every kernel build: the one-load paths, with certainty
    for k, (fmt, flags) in enumerate(((REF.NV12, 0), (REF.NV12, 1), (REF.P010, 0), (REF.P010, 1))):
        luma, chroma = noise_yuv(rng, fmt, 64, 34)
        out.append((f"aligned 64 x 34 {'NV12' if fmt == REF.NV12 else 'P010'} f{flags}", fmt, k % 3, k & 1, flags, luma, chroma, "aligned"))
    out.append(("aligned 36 x 34 BGRA8", REF.BGRA8, 0, 0, 0, noise_bgra(rng, 36, 34), None, "aligned"))
    if again:  # the noise is new; a structured frame is not, so cases 2 k and 2 k + 1 swap where format and size allow: other flags, matrix or planes
        def partner(i):
            j = i ^ 1
            return out[j] if j < len(out) and out[j][1] == out[i][1] and size_of(out[j]) == size_of(out[i]) else out[i]
        out = [(out[i][0] + " again",) + partner(i)[1:] for i in range(len(out))]
    return out


def size_of(case):
    return case[5].shape[1], case[5].shape[0]


_texels = {}


def texels(case):
    """the (h, w, 4) uint8 texels the reference makes of the case's frame: what fdh_put_image gets on the host path (computed once)"""
    if case[0] not in _texels:
        t = REF.convert(case[5], case[6], case[1], case[2], case[3], case[4])
        t.setflags(write=False)
        _texels[case[0]] = t
    return _texels[case[0]]


def element_sizes(fmt):
    """bytes of a luma sample (or BGRA texel) and of a chroma pair"""
    return {REF.BGRA8: (4, 0), REF.NV12: (1, 2), REF.P010: (2, 4)}[fmt]


def _pack_plane(rows, es, run, layout, seed):
    """rows: (n, row_bytes) uint8 of elements of `es` bytes; a lane's one-load run is `run` elements -> (the bytes from the plane's pointer to its last element's end, the pointer's remainder mod 16, pitch).
    What lies between the rows is seeded garbage."""
    n, row = rows.shape
    if layout == "tight":
        pitch, align = row, 0
    elif layout == "aligned":
        pitch, align = (row + 15) // 16 * 16 + 16, 0
    else:  # multiples of the element size, and not of a run's `run` elements
        pad = next(k for k in (1, 2, 3) if (row // es + k) % run)
        pitch, align = row + pad * es, es
        assert pitch % (run * es) and align % (run * es)
    buf = np.random.default_rng(seed).integers(0, 256, size=(n - 1) * pitch + row, dtype=np.uint8)
    for y in range(n):
        buf[y * pitch:y * pitch + row] = rows[y]
    return buf.tobytes(), align, pitch


def pack(case):
    """-> ((luma bytes, align, pitch), (chroma bytes, align, pitch) or None)"""
    name, fmt, _, _, _, luma, chroma, layout = case
    es, pair = element_sizes(fmt)
    h = luma.shape[0]
    y = _pack_plane(np.ascontiguousarray(luma).view(np.uint8).reshape(h, -1), es, 4, layout, len(name) * 7919 + h)
    if chroma is None:
        return y, None
    ch = chroma.shape[0]
    return y, _pack_plane(np.ascontiguousarray(chroma).view(np.uint8).reshape(ch, -1), pair, 2, layout, len(name) * 104729 + ch)
