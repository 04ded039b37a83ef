"""The frames, sources and destinations that the 4:2:2 video tests share (tests/test_video_422_host.py: the kernels' sources under the host
shim; tests/test_video_422.py: the device).  Both directions take the siblings' sizes (video_frame_cases.SIZES; video_out_cases.SMALL and
its rectangles) and add what the 4:2:2 kernels' own shape asks for: their run of eight texels +- 1, the way in's 32 x 32 tile +- 1 and the
way out's 256 x 8 tile +- 1 in every combination, and rectangles with an even x and an odd y, w and h.  Seeded noise throughout; on the
way in the 10-bit words carry garbage in their six high bits, an odd width's last packed group carries garbage in its second luma byte, and
every sample value occurs, those below Yoff and above Yoff + Yden among them.
A way-in case is (name, format, matrix, range, flags, stored, layout, w): `stored` is (Y, Cb, Cr) or (the packed plane,), what
video_422_ref.convert takes; a way-out case is video_out_cases' tuple (name, source w, source h, rect or None, format, matrix, range,
flags, layout)."""
import numpy as np

import video_frame_cases as FC
import video_out_cases as OC
import video_422_ref as REF

RUN = 8                                  # fdh_video_422.h: kRun
IN_TILE = 32                             # fdh_image_import.h: kTile
OUT_TILE_W, OUT_TILE_H = 256, 8          # fdh_video_422.h: kOutTileW, kOutTileH
LAYOUTS = ("tight", "padded", "aligned")  # as video_out_cases has them; padded: multiples of the element size and of nothing more
MATRIX_RANGE = [(m, r) for m in (REF.BT601, REF.BT709, REF.BT2020) for r in (REF.LIMITED, REF.FULL)]
# (format, flags): every format under both chroma rules
KINDS = [(f, fl) for f in REF.FORMATS for fl in (0, REF.CHROMA_LINEAR)]


def build_of(fmt, flags):
    """which of the six builds of either kernel takes the launch: (kTen, kPacked, kLinear); YUY2 and UYVY share theirs"""
    return (REF.bits_of(fmt) == 10, REF.packed(fmt), bool(flags & REF.CHROMA_LINEAR))


BUILDS = sorted({build_of(*k) for k in KINDS})
assert len(BUILDS) == 6


def element_bytes(fmt):
    """what pointers and pitches are multiples of: a sample, or a packed format's group"""
    return 4 if REF.packed(fmt) else 1 if REF.bits_of(fmt) == 8 else 2


def run_of(fmt, p):
    """the elements of plane p that are one wide access: eight luma samples, four chroma samples, four groups"""
    return RUN // 2 if p or REF.packed(fmt) else RUN


def row_bytes(fmt, p, w):
    cw = REF.chroma_width(w)
    return 4 * cw if REF.packed(fmt) else (cw if p else w) * element_bytes(fmt)


def is_wide(fmt, p, align, pitch, w):
    """the host's rule for plane p: a run is one access"""
    run = run_of(fmt, p) * element_bytes(fmt)
    return align % run == 0 and pitch % run == 0 and row_bytes(fmt, p, w) >= run


# ---------------------------------------------------------------------------------------------------------------------- the way in
AROUND_THE_RUN = [(RUN - 1, 5), (RUN, RUN), (RUN + 1, 3)]
AROUND_THE_IN_TILE = [(IN_TILE - 1, IN_TILE + 1), (IN_TILE + 1, IN_TILE - 1)]
IN_SIZES = FC.SIZES + AROUND_THE_RUN + [s for s in AROUND_THE_IN_TILE if s not in FC.SIZES]
IN_LARGEST = FC.LARGEST  # the only size that the sanitizer build of the shim leaves out
ALIGNED_SIZE = (64, 34)  # a tile whose runs are whole and aligned, under every kernel build: the one-load paths, with certainty
FILLER_SIZES = [(33, 31), (9, 3), (70, 5)]  # for the rows of the table a kind has not met yet


def noise_stored(rng, fmt, w, h):
    cw = REF.chroma_width(w)
    if REF.packed(fmt):
        return (rng.integers(0, 256, size=(h, 4 * cw)).astype(np.uint8),)
    top = 256 if REF.bits_of(fmt) == 8 else 65536
    return tuple(rng.integers(0, top, size=s).astype(REF.dtype_of(fmt)) for s in ((h, w), (h, cw), (h, cw)))


def _in_case(rng, what, w, h, fmt, flags, m, r, layout):
    return (f"{what} {w} x {h} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", fmt, m, r, flags, noise_stored(rng, fmt, w, h), layout, w)


def in_cases(largest=True, again=False):
    """a covering set: every size in the tight and the padded layout, the kinds dealt out over them; then, per kind, a small case for
    every row of the coefficient table it has not met; then every kind in the aligned layout.  `again`: the same list with other noise
    (what an update brings)"""
    rng = np.random.default_rng(20261222 if again else 20261221)
    out, n = [], 0
    for w, h in IN_SIZES + ([IN_LARGEST] if largest else []):
        for layout in LAYOUTS[:2]:
            (fmt, flags), (m, r) = KINDS[n % len(KINDS)], MATRIX_RANGE[(n // len(KINDS) + n) % 6]
            out.append(_in_case(rng, "noise", w, h, fmt, flags, m, r, layout))
            n += 1
    for k, (fmt, flags) in enumerate(KINDS):
        met = {(c[2], c[3]) for c in out if (c[1], c[4]) == (fmt, flags)}
        for i, (m, r) in enumerate(row for row in MATRIX_RANGE if row not in met):
            out.append(_in_case(rng, "filler", *FILLER_SIZES[(i + k) % 3], fmt, flags, m, r, LAYOUTS[(i + k) % 2]))
    for k, (fmt, flags) in enumerate(KINDS):
        m, r = MATRIX_RANGE[(5 + k) % 6]
        out.append(_in_case(rng, "aligned", *ALIGNED_SIZE, fmt, flags, m, r, "aligned"))
    if again:
        out = [(c[0] + " again",) + c[1:] for c in out]
    return out


def size_of(case):
    return case[7], case[5][0].shape[0]


_texels = {}


def texels(case):
    """the (h, w, 4) uint8 texels the reference makes of the case's frame: what fdh_put_image gets on the host path (computed once)"""
    if case[0] not in _texels:
        t = REF.convert(case[5], case[1], case[2], case[3], case[4], w=case[7])
        t.setflags(write=False)
        _texels[case[0]] = t
    return _texels[case[0]]


def pack(case):
    """-> per plane (the bytes from the plane's pointer to its last element's end, the pointer's remainder mod 16, pitch); what lies between
    the rows is seeded garbage"""
    name, fmt, layout = case[0], case[1], case[6]
    out = []
    for p, plane in enumerate(case[5]):
        rows = np.ascontiguousarray(plane).view(np.uint8).reshape(plane.shape[0], -1)
        out.append(FC._pack_plane(rows, element_bytes(fmt), run_of(fmt, p), layout, len(name) * 7919 + 31 * p + plane.shape[0]))
    return out


def wide_in(case, p):
    """the host's decision for plane p of a way-in case: one load per run"""
    _, align, pitch = pack(case)[p]
    return is_wide(case[1], p, align, pitch, case[7])


def as_444(case):
    """the frame as the three-plane 4:4:4 frame that converts to the same texels: luma as it is, the chroma the reference's own rule
    gives every texel -- the repeat rule, or the case's FDH_VIDEO_CHROMA_LINEAR -- as a sample per texel.  -> (I444 or I410, (Y, Cb, Cr))"""
    import video_planar_ref as PL

    fmt, w = case[1], case[7]
    y, cb, cr = (REF.samples(p, fmt) for p in REF.as_planes(case[5], fmt, w))
    linear = bool(case[4] & REF.CHROMA_LINEAR)
    dt = REF.dtype_of(fmt)
    return (PL.I444 if REF.bits_of(fmt) == 8 else PL.I410), tuple(np.ascontiguousarray(p.astype(dt)) for p in (y, REF.chroma_at_texels(cb, w, linear), REF.chroma_at_texels(cr, w, linear)))


# ---------------------------------------------------------------------------------------------------------------------- the way out
AROUND_THE_OUT_TILE = [(w, h) for w in (OUT_TILE_W - 1, OUT_TILE_W, OUT_TILE_W + 1) for h in (OUT_TILE_H - 1, OUT_TILE_H, OUT_TILE_H + 1)]
OUT_SIZES = OC.SMALL + [(RUN - 1, 3), (RUN + 1, 2)] + AROUND_THE_OUT_TILE
RECT_SOURCE = OC.RECT_SOURCE
ODD_Y_RECTS = [(4, 5, 7, 9), (2, 1, 129, 17), (136, 39, 3, 1)]  # an even x; y, w and h odd
RECTS = OC.RECTS + ODD_Y_RECTS
FILL = OC.FILL
source, rect_of, cropped, plane_bytes = OC.source, OC.rect_of, OC.cropped, OC.plane_bytes


def out_cases():
    out = []
    for si, (w, h) in enumerate(OUT_SIZES):
        for ki, (fmt, flags) in enumerate(KINDS):
            m, r = MATRIX_RANGE[(si + ki) % 6]
            for layout in LAYOUTS:
                out.append((f"{w} x {h} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", w, h, None, fmt, m, r, flags, layout))
    for k, rect in enumerate(RECTS):
        for ki, (fmt, flags) in enumerate(KINDS):
            m, r = MATRIX_RANGE[(k + ki) % 6]
            layout = LAYOUTS[(k + ki) % 3]
            out.append((f"rect {rect} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", RECT_SOURCE[0], RECT_SOURCE[1], rect, fmt, m, r, flags, layout))
    return out


def layouts(case):
    """-> [(align, pitch, rows, row_bytes)] for the planes Y, Cb, Cr, or for the one packed plane"""
    _, _, w, h = rect_of(case)
    fmt, layout = case[4], case[8]
    return [OC.plane_layout(row_bytes(fmt, p, w), element_bytes(fmt), run_of(fmt, p), layout) + (h, row_bytes(fmt, p, w)) for p in range(1 if REF.packed(fmt) else 3)]


def wide_out(case, p):
    """the host's decision for plane p of a way-out case: one store per run"""
    align, pitch, _, _ = layouts(case)[p]
    return is_wide(case[4], p, align, pitch, rect_of(case)[2])


def expected_planes(case, frame=None):
    """-> per plane the bytes from its pointer to its last row's end: the reference's rows, FILL between a row's end and the pitch.
    `frame`: the case's frame where it is not source(w, h) (the device tests: what fdh_read_pixels returned)"""
    fmt, m, r, flags = case[4:8]
    frame = source(case[1], case[2]) if frame is None else frame
    assert frame.shape == (case[2], case[1], 4)
    planes = REF.export(cropped(frame, rect_of(case)), fmt, m, r, flags)
    out = []
    for plane, (_, pitch, rows, row) in zip(planes, layouts(case)):
        rows_of = np.ascontiguousarray(plane).view(np.uint8).reshape(rows, row)
        buf = np.full(plane_bytes(pitch, rows, row), FILL, np.uint8)
        for y in range(rows):
            buf[y * pitch:y * pitch + row] = rows_of[y]
        out.append(buf)
    return out


def stored_of(bufs, case):
    """the stored planes back as arrays -- (Y, Cb, Cr) or (the packed plane,) --: the inverse of expected_planes' layout"""
    fmt = case[4]
    out = []
    for buf, (_, pitch, rows, row) in zip(bufs, layouts(case)):
        a = np.stack([buf[y * pitch:y * pitch + row] for y in range(rows)])
        out.append(np.ascontiguousarray(a).view(REF.dtype_of(fmt)))
    return tuple(out)
