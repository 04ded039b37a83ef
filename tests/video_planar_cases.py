"""The frames, sources and destinations that the planar-video tests share (tests/test_video_planar_host.py: the kernels' sources under the
host shim; tests/test_video_planar.py: the device).  Both directions take their sizes from the siblings' lists (video_frame_cases.SIZES;
video_out_cases.SMALL, its 128 x 16 tile +- 1, its rectangles) and add what the planar kernels' own shape asks for: their run of eight
texels +- 1 and, on the way out, their 256 x 16 tile +- 1.  Seeded noise throughout; on the way in the 10-bit words carry garbage in their
six high bits and every sample value occurs, those below Yoff and above Yoff + Yden among them.
A way-in case is (name, format, matrix, range, flags, (Y, Cb, Cr), layout); a way-out case is video_out_cases' tuple
(name, source w, source h, rect or None, format, matrix, range, flags, layout)."""
import numpy as np

import video_frame_cases as FC
import video_out_cases as OC
import video_planar_ref as REF

RUN = 8                                  # fdh_video_planar.h: kRun
OUT_TILE_W, OUT_TILE_H = 256, 16         # ... kOutTileW, kOutTileH
LAYOUTS = ("tight", "padded", "aligned")  # as video_out_cases has them; padded: multiples of the sample size and of nothing more
MATRIX_RANGE = [(m, r) for m in (REF.BT601, REF.BT709, REF.BT2020) for r in (REF.LIMITED, REF.FULL)]
# (format, flags): every kernel build of either direction
KINDS = [(REF.I420, 0), (REF.I420, REF.CHROMA_LINEAR), (REF.I010, 0), (REF.I010, REF.CHROMA_LINEAR), (REF.I444, 0), (REF.I410, 0)]

# ---------------------------------------------------------------------------------------------------------------------- the way in
AROUND_THE_RUN = [(RUN - 1, 5), (RUN, RUN), (RUN + 1, 3)]
IN_SIZES = FC.SIZES + AROUND_THE_RUN
IN_LARGEST = FC.LARGEST  # the only size that the sanitizer build of the shim leaves out
ALIGNED_SIZE = (64, 34)  # a tile whose runs are whole and aligned, under every kernel build: the one-load paths, with certainty


def noise_planes(rng, fmt, w, h):
    cw, ch = REF.chroma_size(fmt, w, h)
    top = 256 if REF.bits_of(fmt) == 8 else 65536
    return tuple(rng.integers(0, top, size=s).astype(REF.dtype_of(fmt)) for s in ((h, w), (ch, cw), (ch, cw)))


def in_cases(largest=True, again=False):
    """a covering set: every size in the tight and the padded layout, the kinds dealt out over them so that every kind meets every row of
    the coefficient table (the aligned cases take each kind's sixth row).  `again`: the same list with other noise (what an update brings)"""
    rng = np.random.default_rng(20261122 if again else 20261121)
    out, n = [], 0
    for w, h in IN_SIZES + ([IN_LARGEST] if largest else []):
        for layout in LAYOUTS[:2]:
            (fmt, flags), (m, r) = KINDS[n % 6], MATRIX_RANGE[(n // 6 + n) % 6]
            out.append((f"noise {w} x {h} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", fmt, m, r, flags, noise_planes(rng, fmt, w, h), layout))
            n += 1
    for k, (fmt, flags) in enumerate(KINDS):
        m, r = MATRIX_RANGE[(5 + k) % 6]
        out.append((f"aligned {ALIGNED_SIZE[0]} x {ALIGNED_SIZE[1]} {REF.NAMES[fmt]} m{m} r{r} f{flags}", fmt, m, r, flags, noise_planes(rng, fmt, *ALIGNED_SIZE), "aligned"))
    if again:
        out = [(c[0] + " again",) + c[1:] for c in out]
    return out


def size_of(case):
    return case[5][0].shape[1], case[5][0].shape[0]


_texels = {}


def texels(case):
    """the (h, w, 4) uint8 texels the reference makes of the case's frame: what fdh_put_image gets on the host path (computed once)"""
    if case[0] not in _texels:
        t = REF.convert(case[5], case[1], case[2], case[3], case[4])
        t.setflags(write=False)
        _texels[case[0]] = t
    return _texels[case[0]]


def run_of(fmt, p):
    """the samples of plane p that are one wide access"""
    return RUN // 2 if p and not REF.full_chroma(fmt) else RUN


def pack(case):
    """-> per plane (the bytes from the plane's pointer to its last sample's end, the pointer's remainder mod 16, pitch); what lies between
    the rows is seeded garbage"""
    name, fmt, layout = case[0], case[1], case[6]
    es = 1 if REF.bits_of(fmt) == 8 else 2
    out = []
    for p, plane in enumerate(case[5]):
        rows = np.ascontiguousarray(plane).view(np.uint8).reshape(plane.shape[0], -1)
        out.append(FC._pack_plane(rows, es, run_of(fmt, p), layout, len(name) * 7919 + 31 * p + plane.shape[0]))
    return out


def interleaved(case):
    """the semi-planar frame with the same samples, as video_frame_ref.convert takes it: (NV12 or P010, luma, chroma).  I420 -> NV12; I010 ->
    P010 of value << 6 (the garbage of the high bits is gone: P010 has its own, in the low bits, which stay zero here)"""
    fmt = case[1]
    assert not REF.full_chroma(fmt)
    y, cb, cr = case[5]
    if fmt == REF.I420:
        return 1, y, np.stack([cb, cr], axis=2)
    return 2, ((y & 1023) << 6).astype(np.uint16), ((np.stack([cb, cr], axis=2) & 1023) << 6).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------- the way out
AROUND_THE_OUT_TILE = [(w, h) for w in (OUT_TILE_W - 1, OUT_TILE_W, OUT_TILE_W + 1) for h in (OUT_TILE_H - 1, OUT_TILE_H, OUT_TILE_H + 1)]
OUT_SIZES = OC.SMALL + [(RUN - 1, 3), (RUN + 1, 2)] + OC.AROUND_THE_TILE + AROUND_THE_OUT_TILE
RECT_SOURCE, RECTS, ODD_RECTS = OC.RECT_SOURCE, OC.RECTS, OC.ODD_RECTS  # ODD_RECTS: the 4:4:4 formats only
FILL = OC.FILL
source, rect_of, cropped, plane_bytes = OC.source, OC.rect_of, OC.cropped, OC.plane_bytes


def out_cases():
    out = []
    for si, (w, h) in enumerate(OUT_SIZES):
        for ki, (fmt, flags) in enumerate(KINDS):
            m, r = MATRIX_RANGE[(si + ki) % 6]
            for layout in LAYOUTS:
                out.append((f"{w} x {h} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", w, h, None, fmt, m, r, flags, layout))
    for k, rect in enumerate(RECTS + ODD_RECTS):
        for ki, (fmt, flags) in enumerate(KINDS):
            if rect in ODD_RECTS and not REF.full_chroma(fmt):
                continue
            m, r = MATRIX_RANGE[(k + ki) % 6]
            layout = LAYOUTS[(k + ki) % 3]
            out.append((f"rect {rect} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", RECT_SOURCE[0], RECT_SOURCE[1], rect, fmt, m, r, flags, layout))
    return out


def layouts(case):
    """-> [(align, pitch, rows, row_bytes)] for the planes Y, Cb, Cr"""
    _, _, w, h = rect_of(case)
    fmt, layout = case[4], case[8]
    es = 1 if REF.bits_of(fmt) == 8 else 2
    cw, ch = REF.chroma_size(fmt, w, h)
    return [OC.plane_layout(pw * es, es, run_of(fmt, p), layout) + (ph, pw * es) for p, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch)))]


def expected_planes(case, frame=None):
    """-> per plane the bytes from its pointer to its last sample's end: the reference's rows, FILL between a row's end and the pitch.
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


def planes_of(bufs, case):
    """the stored planes back as arrays (Y, Cb, Cr): the inverse of expected_planes' layout"""
    fmt = case[4]
    out = []
    for buf, (_, pitch, rows, row_bytes) in zip(bufs, layouts(case)):
        a = np.stack([buf[y * pitch:y * pitch + row_bytes] for y in range(rows)])
        out.append(np.ascontiguousarray(a).view(REF.dtype_of(fmt)))
    return out
