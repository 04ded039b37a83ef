"""The frames, sources and destinations that the tests of video with an alpha plane share (tests/test_video_alpha_host.py: the kernels'
sources under the host shim; tests/test_video_alpha.py: the device).  Both directions take the 4:2:2 tests' sizes (video_422_cases) --
the run of eight texels +- 1, the way in's 32 x 32 tile +- 1, the way out's 256-wide tile +- 1 -- and add the heights around A420's
tile of 16 rows; layouts `tight`, `padded` (multiples of the element size and of nothing more: element by element) and `aligned` (the
wide accesses, with padding).  Seeded noise throughout.  On the way in the 10-bit words carry garbage in their six high bits, an odd
width's last UYVY group carries garbage in its second luma byte, and the alpha plane holds 0, the top value and everything between.  On
the way out the shim's source is raw noise -- colour bytes above their alpha among them, which a rendered frame cannot promise -- whose
first three texels hold alpha 0, 255 and a value between.
A way-in case is (name, format, matrix, range, flags, stored, layout, w): `stored` is (Y, Cb, Cr, A) or (the UYVY plane, A), what
video_alpha_ref.convert takes; a way-out case is video_out_cases' tuple (name, source w, source h, rect or None, format, matrix, range,
flags, layout)."""
import numpy as np

import video_422_cases as C2
import video_frame_cases as FC
import video_out_cases as OC
import video_alpha_ref as REF

RUN = 8                                   # fdh_video_alpha.h: kRun
IN_TILE = 32                              # fdh_image_import.h: kTile
OUT_TILE_W = 256                          # fdh_video_alpha.h: kOutTileW
LAYOUTS = ("tight", "padded", "aligned")
MATRIX_RANGE = [(m, r) for m in (REF.BT601, REF.BT709, REF.BT2020) for r in (REF.LIMITED, REF.FULL)]
L, S = REF.CHROMA_LINEAR, REF.STRAIGHT_ALPHA
# (format, flags): every format under the chroma rules it has, premultiplied and straight -- the twelve builds of either kernel
KINDS = [(f, fl | st) for f in REF.FORMATS for fl in ((0, L) if REF.linear_allowed(f) else (0,)) for st in (0, S)]
BUILDS = KINDS
assert len(KINDS) == 12


def out_tile_h(fmt):
    """fdh_video_alpha.h: out_tile_h"""
    return 16 if fmt == REF.A420 else 8


def build_index(fmt, flags):
    """the programs' number of a build"""
    kind = {REF.A420: 0, REF.A444: 2, REF.A410: 3, REF.UYVA: 4}[fmt] + (1 if flags & L else 0)
    return 2 * kind + (1 if flags & S else 0)


def plane_ids(fmt):
    return (0, 3) if REF.packed(fmt) else (0, 1, 2, 3)


def element_bytes(fmt, p):
    """what plane p's pointer and pitch are multiples of: a sample, or the UYVY plane's group"""
    return 4 if REF.packed(fmt) and p == 0 else 1 if REF.bits_of(fmt) == 8 else 2


def run_of(fmt, p):
    """the elements of plane p that are one wide access: eight luma or alpha samples, four or eight chroma samples, four groups"""
    if REF.packed(fmt) and p == 0:
        return RUN // 2
    return RUN // 2 if p in (1, 2) and not REF.full_chroma(fmt) else RUN


def plane_size(fmt, p, w, h):
    """-> a row's bytes, the rows"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if REF.packed(fmt) and p == 0:
        return 4 * cw, h
    if p in (1, 2) and not REF.full_chroma(fmt):
        return cw * element_bytes(fmt, p), ch
    return w * element_bytes(fmt, p), h


def is_wide(fmt, p, align, pitch, w):
    """the host's rule for plane p: a run is one access"""
    run = run_of(fmt, p) * element_bytes(fmt, p)
    return align % run == 0 and pitch % run == 0 and plane_size(fmt, p, w, 1)[0] >= run


# ---------------------------------------------------------------------------------------------------------------------- the way in
IN_SIZES = C2.IN_SIZES
IN_LARGEST = C2.IN_LARGEST  # the only size that the sanitizer build of the shim leaves out
ALIGNED_SIZE = C2.ALIGNED_SIZE
FILLER_SIZES = C2.FILLER_SIZES


def noise_alpha(rng, fmt, w, h):
    """an alpha plane: a quarter 0, a quarter the top value, the rest anything; 10-bit words with garbage in their six high bits"""
    top = (1 << REF.bits_of(fmt)) - 1
    a = rng.integers(0, top + 1, size=(h, w))
    kind = rng.integers(0, 4, size=(h, w))
    a[kind == 0], a[kind == 1] = 0, top
    if REF.bits_of(fmt) == 10:
        a |= rng.integers(0, 64, size=(h, w)) << 10
    return a.astype(REF.dtype_of(fmt))


def noise_stored(rng, fmt, w, h):
    ref, base = REF.BASE[fmt]
    if REF.packed(fmt):
        colour = C2.noise_stored(rng, base, w, h)
    else:
        cw, ch = ref.chroma_size(base, w, h)
        top = 256 if REF.bits_of(fmt) == 8 else 65536
        colour = tuple(rng.integers(0, top, size=s).astype(REF.dtype_of(fmt)) for s in ((h, w), (ch, cw), (ch, cw)))
    return colour + (noise_alpha(rng, fmt, w, h),)


def _in_case(rng, what, w, h, fmt, flags, m, r, layout):
    return (f"{what} {w} x {h} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", fmt, m, r, flags, noise_stored(rng, fmt, w, h), layout, w)


def in_cases(largest=True, again=False):
    """a covering set: every size in the tight and the padded layout, the kinds dealt out over them; then, per kind, a small case for
    every row of the coefficient table it has not met; then every kind in the aligned layout.  `again`: the same list with other noise
    (what an update brings)"""
    rng = np.random.default_rng(20270122 if again else 20270121)
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
    return case[7], case[5][-1].shape[0]


_texels = {}


def texels(case):
    """the (h, w, 4) uint8 texels the reference makes of the case's frame: what fdh_put_image gets on the host path (computed once)"""
    if case[0] not in _texels:
        t = REF.convert(case[5], case[1], case[2], case[3], case[4], w=case[7])
        t.setflags(write=False)
        _texels[case[0]] = t
    return _texels[case[0]]


def pack(case):
    """-> per plane the format has, in the order of plane_ids, (the bytes from the plane's pointer to its last element's end, the
    pointer's remainder mod 16, pitch); what lies between the rows is seeded garbage"""
    name, fmt, layout = case[0], case[1], case[6]
    out = []
    for p, plane in zip(plane_ids(fmt), case[5]):
        rows = np.ascontiguousarray(plane).view(np.uint8).reshape(plane.shape[0], -1)
        out.append(FC._pack_plane(rows, element_bytes(fmt, p), run_of(fmt, p), layout, len(name) * 7919 + 31 * p + plane.shape[0]))
    return out


def four_of(fmt, values, nothing=0):
    """per-plane values in the order of plane_ids -> the four slots of the struct"""
    out = [nothing] * 4
    for p, v in zip(plane_ids(fmt), values):
        out[p] = v
    return out


def wide_in(case, p):
    """the host's decision for plane p of a way-in case: one load per run"""
    _, align, pitch = pack(case)[plane_ids(case[1]).index(p)]
    return is_wide(case[1], p, align, pitch, case[7])


def opaque(case):
    """the case with its alpha plane all 255 (1023 for A410, garbage in the six high bits kept)"""
    fmt = case[1]
    a = case[5][-1] | REF.dtype_of(fmt)((1 << REF.bits_of(fmt)) - 1)
    return (case[0] + " opaque",) + case[1:5] + (case[5][:-1] + (a,),) + case[6:]


# ---------------------------------------------------------------------------------------------------------------------- the way out
SMALL = OC.SMALL + [(RUN - 1, 3), (RUN + 1, 2)]
RECT_SOURCE = OC.RECT_SOURCE
FILL = OC.FILL
rect_of, cropped, plane_bytes = OC.rect_of, OC.cropped, OC.plane_bytes


def around_the_tile(fmt):
    t = out_tile_h(fmt)
    return [(w, h) for w in (OUT_TILE_W - 1, OUT_TILE_W, OUT_TILE_W + 1) for h in (t - 1, t, t + 1)]


def out_sizes(fmt):
    return SMALL + around_the_tile(fmt)


def rects(fmt):
    """A420: x and y even; UYVA: x even, an odd y too; A444, A410: anything"""
    if fmt == REF.A420:
        return OC.RECTS
    return OC.RECTS + C2.ODD_Y_RECTS + ([] if REF.packed(fmt) else OC.ODD_RECTS)


_sources = {}


def source(w, h):
    """the shim's frame of a case: seeded noise in every byte -- colour bytes above their alpha among them -- with alpha 0, 255 and 128 in
    its first three texels, and a quarter of the rest alpha 0, a quarter 255 (computed once, read-only)"""
    if (w, h) not in _sources:
        rng = np.random.default_rng(w * 1000 + h + 77)
        img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        kind = rng.integers(0, 4, size=(h, w))
        img[kind == 0, 3], img[kind == 1, 3] = 0, 255
        flat = img.reshape(-1, 4)
        flat[:3, 3] = np.array([0, 255, 128], np.uint8)[:len(flat)]
        img.setflags(write=False)
        _sources[(w, h)] = img
    return _sources[(w, h)]


def out_cases():
    out = []
    for ki, (fmt, flags) in enumerate(KINDS):
        for si, (w, h) in enumerate(out_sizes(fmt)):
            m, r = MATRIX_RANGE[(si + ki) % 6]
            for layout in LAYOUTS:
                out.append((f"{w} x {h} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", w, h, None, fmt, m, r, flags, layout))
        for k, rect in enumerate(rects(fmt)):
            m, r = MATRIX_RANGE[(k + ki) % 6]
            layout = LAYOUTS[(k + ki) % 3]
            out.append((f"rect {rect} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", RECT_SOURCE[0], RECT_SOURCE[1], rect, fmt, m, r, flags, layout))
    return out


def layouts(case):
    """-> [(align, pitch, rows, row_bytes)] for the planes the format has, in the order of plane_ids"""
    _, _, w, h = rect_of(case)
    fmt, layout = case[4], case[8]
    out = []
    for p in plane_ids(fmt):
        row, rows = plane_size(fmt, p, w, h)
        out.append(OC.plane_layout(row, element_bytes(fmt, p), run_of(fmt, p), layout) + (rows, row))
    return out


def wide_out(case, p):
    """the host's decision for plane p of a way-out case: one store per run"""
    align, pitch, _, _ = layouts(case)[plane_ids(case[4]).index(p)]
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
    """the stored planes back as arrays -- (Y, Cb, Cr, A) or (the UYVY plane, A) --: the inverse of expected_planes' layout"""
    fmt = case[4]
    out = []
    for buf, (_, pitch, rows, row) in zip(bufs, layouts(case)):
        a = np.stack([buf[y * pitch:y * pitch + row] for y in range(rows)])
        out.append(np.ascontiguousarray(a).view(REF.dtype_of(fmt)))
    return tuple(out)


def quotient_surface():
    """256 x 256: texel (c, a) -- column c, row a -- holds colour c in all three channels and alpha a: every (c, a), c above a included"""
    img = np.empty((256, 256, 4), np.uint8)
    img[..., :3] = np.arange(256, dtype=np.uint8)[None, :, None]
    img[..., 3] = np.arange(256, dtype=np.uint8)[:, None]
    return img
