"""The frames and destinations that the video-out tests share (tests/test_video_out_host.py: the kernel's source under the host shim;
tests/test_video_out.py: the device): the smallest sizes at which the run of four texels by two rows, the odd chroma edge and the
128 x 16 tile change their way; seeded noise with a varying alpha byte; destination layouts that allow the wide stores and layouts that
force the element stores.  A case is (name, source w, source h, rect or None, format, matrix, range, flags, layout)."""
import numpy as np

import video_out_ref as REF

TILE_W, TILE_H = 128, 16  # fdh_video_export.h: kTileW, kTileH
SMALL = [(1, 1), (2, 1), (1, 2), (3, 3), (4, 2), (5, 7), (8, 2)]
AROUND_THE_TILE = [(w, h) for w in (TILE_W - 1, TILE_W, TILE_W + 1) for h in (TILE_H - 1, TILE_H, TILE_H + 1)]
SIZES = SMALL + AROUND_THE_TILE
# tight: pitch = a row's bytes, pointer on a 16-byte boundary; padded: pitch and pointer multiples of the element size and of nothing more
# (the element stores); aligned: pitch a multiple of 16 beyond the row, pointer on a 16-byte boundary (the wide stores, with padding)
LAYOUTS = ("tight", "padded", "aligned")
MATRIX_RANGE = [(m, r) for m in (REF.BT601, REF.BT709, REF.BT2020) for r in (REF.LIMITED, REF.FULL)]
# (format, flags): every format, both chroma rules, both BGRA8 alphas
KINDS = [(REF.NV12, 0), (REF.NV12, REF.CHROMA_LINEAR), (REF.P010, 0), (REF.P010, REF.CHROMA_LINEAR), (REF.BGRA8, 0), (REF.BGRA8, REF.IGNORE_ALPHA)]
# rectangles inside a 140 x 40 source: even offsets; a source run that starts on a 16-byte boundary and one that does not; the tile +- 1
RECT_SOURCE = (140, 40)
RECTS = [(4, 6, 128, 16), (2, 2, 129, 17), (8, 0, 127, 15), (12, 4, 5, 7), (0, 2, 3, 3), (136, 38, 4, 2), (6, 8, 1, 1)]
ODD_RECTS = [(3, 5, 7, 9), (1, 1, 130, 18)]  # BGRA8 only


def name_of(fmt):
    return {REF.BGRA8: "BGRA8", REF.NV12: "NV12", REF.P010: "P010"}[fmt]


def cases():
    out = []
    for si, (w, h) in enumerate(SIZES):
        for ki, (fmt, flags) in enumerate(KINDS):
            m, r = (0, 0) if fmt == REF.BGRA8 else MATRIX_RANGE[(si + ki) % 6]  # (16 sizes: every kind meets every row of the table)
            for layout in LAYOUTS:
                out.append((f"{w} x {h} {name_of(fmt)} m{m} r{r} f{flags} {layout}", w, h, None, fmt, m, r, flags, layout))
    for k, rect in enumerate(RECTS + ODD_RECTS):
        for fmt, flags in KINDS:
            if rect in ODD_RECTS and fmt != REF.BGRA8:
                continue
            m, r = (0, 0) if fmt == REF.BGRA8 else MATRIX_RANGE[(k + fmt + flags) % 6]
            layout = LAYOUTS[(k + fmt + flags) % 3]
            out.append((f"rect {rect} {name_of(fmt)} m{m} r{r} f{flags} {layout}", RECT_SOURCE[0], RECT_SOURCE[1], rect, fmt, m, r, flags, layout))
    return out


_sources = {}


def source(w, h):
    """the frame of a case: seeded noise, every byte value in every channel, the alpha byte among them (computed once, read-only)"""
    if (w, h) not in _sources:
        img = np.random.default_rng(w * 1000 + h).integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        img.setflags(write=False)
        _sources[(w, h)] = img
    return _sources[(w, h)]


def rect_of(case):
    """-> x, y, w, h, the whole frame where the case has no rectangle"""
    return case[3] if case[3] is not None else (0, 0, case[1], case[2])


def cropped(img, rect):
    x, y, w, h = rect
    return img[y:y + h, x:x + w]


def element_sizes(fmt):
    """bytes of a luma sample (or BGRA texel) and of a chroma pair"""
    return {REF.BGRA8: (4, 0), REF.NV12: (1, 2), REF.P010: (2, 4)}[fmt]


def plane_layout(row_bytes, es, run, layout):
    """a plane of rows of row_bytes bytes, elements of `es` bytes, a wide store of `run` elements -> (the pointer's remainder mod 16, pitch)"""
    if layout == "tight":
        return 0, row_bytes
    if layout == "aligned":
        return 0, (row_bytes + 15) // 16 * 16 + 16
    pad = next(k for k in (1, 2, 3) if (row_bytes // es + k) % run)
    pitch, align = row_bytes + pad * es, es
    assert pitch % (run * es) and align % (run * es)
    return align, pitch


def layouts(case):
    """-> [(align, pitch, rows, row_bytes)] for planes[0] and, for NV12 / P010, planes[1]"""
    _, _, w, h = rect_of(case)
    fmt, layout = case[4], case[8]
    es, pair = element_sizes(fmt)
    out = [plane_layout(w * es, es, 4, layout) + (h, w * es)]
    if pair:
        cw, ch = (w + 1) // 2, (h + 1) // 2
        out.append(plane_layout(cw * pair, pair, 2, layout) + (ch, cw * pair))
    return out


def plane_bytes(pitch, rows, row_bytes):
    """from the plane's pointer to its last element's end"""
    return (rows - 1) * pitch + row_bytes


FILL = 0xEE


def expected_planes(case, frame=None):
    """-> per plane the bytes from its pointer to its last element's end: the reference's rows, FILL between a row's end and the pitch.
    `frame`: the case's frame where it is not source(w, h) (the device tests: what fdh_read_pixels returned)"""
    fmt, m, r, flags = case[4:8]
    frame = source(case[1], case[2]) if frame is None else frame
    assert frame.shape == (case[2], case[1], 4)
    planes = REF.export(cropped(frame, rect_of(case)), fmt, m, r, flags)
    out = []
    for plane, (_, pitch, rows, row_bytes) in zip(planes, layouts(case)):
        rows_of = np.ascontiguousarray(plane).view(np.uint8).reshape(rows, row_bytes)
        buf = np.full(plane_bytes(pitch, rows, row_bytes), FILL, np.uint8)
        for y in range(rows):
            buf[y * pitch:y * pitch + row_bytes] = rows_of[y]
        out.append(buf)
    return out
