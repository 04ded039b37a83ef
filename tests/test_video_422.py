"""4:2:2 video in and out on the device (fdh_put_video_422, fdh_update_video_422, fdh_read_video_422; k_video_422_import,
k_video_422_export; include_video/figdraw_hip_video_422.h).  The bar is identity both ways.  The way in: a context that gets I422, I210,
YUY2 and UYVY frames from device memory against one that gets, through fdh_put_image, the bytes the reference tests/video_422_ref.py
makes of them, and against one that gets the same frames as I444 / I410 through fdh_put_video_planes, the chroma given to every texel by
the reference's own rule -- every level of the atlases, the draw records (the ink boxes shrink the draws) and a rendered frame.  The way
out: the planes against the reference applied to what fdh_read_pixels returns of the same frame, from each plane's pointer to its last
row's end, the padding untouched; the I422 / I210 chroma also against fdh_read_video_planes' I420 / I010 chroma of a frame rendered with
doubled rows, and the packed planes against the I422 call's planes interleaved."""
import ctypes as C

import numpy as np
import pytest

import video_planar_ref as PL
import video_422_cases as VC
import video_422_ref as REF

pytestmark = pytest.mark.gpu

WHITE = [(255, 255, 255, 255)] * 4
OPAQUE, TRANSPARENT = (0.1, 0.2, 0.3, 1.0), (0.0, 0.0, 0.0, 0.0)


class Memory:
    """device memory through the runtime the library runs on"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.blocks, self.pinned = [], []

    def device(self, n):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
        self.blocks.append(p)
        return p.value

    def filled(self, n, align=0):
        """n bytes of VC.FILL in device memory at an address `align` past a 256-byte boundary, in a block that ends with them"""
        base = self.device(n + align)
        assert self.hip.hipMemset(C.c_void_p(base), VC.FILL, C.c_size_t(n + align)) == 0
        return base + align

    def upload(self, data: bytes, align=0):
        """`data` in device memory at an address `align` past a 256-byte boundary, in a block that ends with it"""
        base = self.device(len(data) + align)
        assert self.hip.hipMemcpy(C.c_void_p(base + align), data, C.c_size_t(len(data)), 1) == 0  # host -> device
        return base + align

    def download(self, ptr, n):
        out = np.empty(n, np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(n), 2) == 0  # device -> host
        return out

    def page_locked(self, n, data: bytes = None):
        p = C.c_void_p()
        assert self.hip.hipHostMalloc(C.byref(p), C.c_size_t(n), 0) == 0
        self.pinned.append(p)
        if data is None:
            C.memset(p.value, VC.FILL, n)
        else:
            C.memmove(p.value, data, n)
        return p.value

    def free(self):
        for p in self.blocks:
            self.hip.hipFree(p)
        for p in self.pinned:
            self.hip.hipHostFree(p)
        self.blocks, self.pinned = [], []


@pytest.fixture(scope="module")
def memory():
    m = Memory()
    yield m
    m.free()


def three_of(values):
    """a one-plane format's pointer or pitch as the call takes it: (v, 0, 0)"""
    return list(values) + [0] * (3 - len(values))


# ------------------------------------------------------------------------------------------------------------------ the way in
def put_case(ctx, memory, key, case, update=False, place=None):
    """`place`: how a plane's bytes get an address (memory.upload by default)"""
    w, h = VC.size_of(case)
    place = place or memory.upload
    packed = VC.pack(case)
    ptrs, pitches = three_of([place(data, align) for data, align, _ in packed]), three_of([pitch for _, _, pitch in packed])
    call = ctx.update_video_422 if update else ctx.put_video_422
    return call(key, ptrs, w, h, pitches, format=case[1], matrix=case[2], range=case[3], flags=case[4])


def put_as_444(ctx, memory, key, case, update=False):
    """the same texels through the sibling: fdh_put_video_planes of the I444 / I410 frame whose chroma the reference's rule gave every texel,
    tightly packed"""
    w, h = VC.size_of(case)
    fmt, planes = VC.as_444(case)
    call = ctx.update_video_planes if update else ctx.put_video_planes
    return call(key, [memory.upload(p.tobytes()) for p in planes], w, h, [p.strides[0] for p in planes], format=fmt, matrix=case[2], range=case[3], flags=0)


def levels_of(ctx):
    return [ctx.read_atlas_level(l) for l in range(ctx.atlas_size().bit_length())]


def same_atlases(a, b, what=""):
    """usage and every level, byte for byte"""
    assert a.atlas_usage() == b.atlas_usage(), what
    for l, (x, y) in enumerate(zip(levels_of(a), levels_of(b))):
        assert x.shape == y.shape, (what, l)
        if not np.array_equal(x, y):
            ys, xs = np.nonzero((x != y).any(axis=2))
            raise AssertionError(f"{what}: level {l} differs in {len(xs)} texels, the first at ({xs[0]}, {ys[0]}): {x[ys[0], xs[0]]} != {y[ys[0], xs[0]]}")


@pytest.fixture(scope="module")
def three(memory):
    """every case into one atlas of 2048 on three fresh contexts: the 4:2:2 call; fdh_put_image of the reference's texels; and
    fdh_put_video_planes of the frame as I444 / I410 -> cases, contexts, the rectangles"""
    from figdraw_amd.context import HipContext

    cases = VC.in_cases()
    dev, host, sib = (HipContext(atlas_size=2048, device=0) for _ in range(3))
    rects = []
    for i, case in enumerate(cases):
        texels = VC.texels(case)
        r = put_case(dev, memory, 100 + i, case)
        assert r == host.put_image(100 + i, texels), case[0]
        assert r == put_as_444(sib, memory, 100 + i, case), case[0]
        assert r[2:] == VC.size_of(case) and dev.image_rect(100 + i) == r
        rects.append(r)
    assert dev.atlas_size() == 2048
    yield cases, dev, host, sib, rects
    dev.close(), host.close(), sib.close()


def test_rectangles_usage_and_every_level(three):
    cases, dev, host, sib, rects = three
    assert len(cases) >= 48 and {VC.build_of(c[1], c[4]) for c in cases} == set(VC.BUILDS)
    same_atlases(dev, host, "all cases, against fdh_put_image")
    same_atlases(dev, sib, "all cases, against fdh_put_video_planes of the 4:4:4 frame")
    level0 = dev.read_atlas_level(0)
    for case, (x, y, w, h) in zip(cases, rects):  # and level 0 is the reference's conversion (nothing of a line)
        want = VC.texels(case) if w > 1 and h > 1 else np.zeros((h, w, 4), np.uint8)
        assert np.array_equal(level0[y:y + h, x:x + w], want), case[0]


def _frame(ctx, cases, rects):
    """every image up to 128 x 128 at 1:1 and magnified 2.5 times (the draws shrink to the ink boxes), the larger ones minified"""
    W, H = 2000, 1500
    ctx.begin_frame(W, H, True, (0.1, 0.2, 0.3, 1.0))
    x, y, row, n = 4.0, 4.0, 0.0, 0
    for i, r in enumerate(rects):
        w, h = r[2:]
        for s in ((0.25,) if w > 128 or h > 128 else (1.0, 2.5)):
            if x + w * s > W - 4:
                x, y, row = 4.0, y + row + 3.0, 0.0
            ctx.draw_image(100 + i, (x + 0.25 * (i % 3), y), WHITE, (w * s, h * s), i % 7 == 3)
            x += w * s + 3.0
            row = max(row, h * s)
            n += 1
    assert y + row < H
    ctx.end_frame()
    return n


def test_draw_records_and_frames(three):
    """the ink boxes: the draw records are those of the host path (a draw shrinks to its image's ink box), and so is the rendered frame"""
    cases, dev, host, sib, rects = three
    for ctx in (dev, host, sib):
        n = _frame(ctx, cases, rects)
    assert n > 60
    assert dev.record_digest() == host.record_digest() == sib.record_digest()
    got = dev.read_pixels()
    assert np.array_equal(got, host.read_pixels()) and np.array_equal(got, sib.read_pixels())


def test_updates_of_every_case(three, memory):
    """(behind the tests of the puts: it changes the fixture's atlases) every entry gets the next frame on every path"""
    cases, dev, host, sib, rects = three
    nxt = VC.in_cases(again=True)
    for i, case in enumerate(nxt):
        texels = VC.texels(case)
        assert not np.array_equal(texels, VC.texels(cases[i])), case[0]
        put_case(dev, memory, 100 + i, case, update=True)
        host.update_image(100 + i, texels)
        put_as_444(sib, memory, 100 + i, case, update=True)
    same_atlases(dev, host, "all cases updated, against fdh_update_image")
    same_atlases(dev, sib, "all cases updated, against fdh_update_video_planes of the 4:4:4 frame")
    for ctx in (dev, host):
        _frame(ctx, nxt, rects)
    assert dev.record_digest() == host.record_digest()
    assert np.array_equal(dev.read_pixels(), host.read_pixels())


def small_case(fmt, flags, w, h, seed, layout="padded", matrix=REF.BT601, rng=REF.FULL):
    return (f"{REF.NAMES[fmt]} {w} x {h} seed {seed}", fmt, matrix, rng, flags, VC.noise_stored(np.random.default_rng(seed), fmt, w, h), layout, w)


def test_page_locked_host_memory_is_a_source(memory):
    from figdraw_amd.context import HipContext

    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    for key, (fmt, flags) in enumerate(((REF.I210, REF.CHROMA_LINEAR), (REF.UYVY, 0), (REF.I422, 0)), start=1):
        case = small_case(fmt, flags, 71, 45, 30 + key, layout="tight", matrix=REF.BT2020, rng=REF.LIMITED)
        assert put_case(dev, memory, key, case, place=lambda data, align: memory.page_locked(len(data), data)) == host.put_image(key, VC.texels(case))
    same_atlases(dev, host, "page-locked")
    dev.close(), host.close()


def test_pageable_host_memory_is_refused_for_every_plane(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    host_planes = [np.zeros((9, 16), np.uint8), np.zeros((9, 8), np.uint8), np.zeros((9, 8), np.uint8)]
    good = [memory.upload(p.tobytes()) for p in host_planes]
    packed_host = np.zeros((9, 32), np.uint8)
    assert ctx.put_video_422(1, good, 16, 9, (16, 8, 8))[2:] == (16, 9)
    before = ctx.atlas_usage()
    attempts = []
    for p in range(3):
        ptrs = list(good)
        ptrs[p] = host_planes[p].ctypes.data
        attempts.append((ptrs, (16, 8, 8), REF.I422))
    attempts.append(([packed_host.ctypes.data, 0, 0], (32, 0, 0), REF.YUY2))
    for ptrs, pitches, fmt in attempts:
        for call in (lambda: ctx.put_video_422(2, ptrs, 16, 9, pitches, format=fmt), lambda: ctx.update_video_422(1, ptrs, 16, 9, pitches, format=fmt)):
            with pytest.raises(FigdrawHipError) as e:
                call()
            assert e.value.code == -1 and "neither device memory of the context's device nor page-locked host memory" in str(e.value)
            assert ctx.atlas_usage() == before and not ctx.has_image(2)
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    assert ctx.put_video_422(2, good, 16, 9, (16, 8, 8))[2:] == (16, 9)  # and the context works on
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the way out
def noise(w, h, seed=0):
    """premultiplied noise with every alpha"""
    rng = np.random.default_rng(1000 * w + h + seed)
    img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint16)
    img[..., :3] = img[..., :3] * img[..., 3:] // 255
    return img.astype(np.uint8)


def render(ctx, w, h, clear, seed=0, double=False):
    """a few shapes, then the noise image 1:1 over them: neighbouring pixels differ in every channel.  `double`: the frame is 2 h rows,
    row y of the noise in rows 2 y and 2 y + 1 -- what is drawn under it is covered (the noise is drawn opaque then)"""
    img = noise(w, h, seed)
    if double:
        img[..., 3] = 255
        img = np.repeat(img, 2, axis=0)
        h = 2 * h
    ctx.put_image(1, img)
    ctx.begin_frame(w, h, True, clear)
    ctx.draw_rect((0.0, 0.0, w * 0.6, h * 0.5), (200, 40, 90, 255))
    ctx.draw_rect((w * 0.3, h * 0.25, w * 0.7, h * 0.75), (10, 220, 160, 180))
    ctx.draw_image(1, (0.0, 0.0), WHITE, (float(w), float(h)))
    ctx.end_frame()
    return ctx.read_pixels()


def export(ctx, memory, frame, fmt, m, r, flags, layout, rect=None, alloc=None):
    """one fdh_read_video_422 into fresh blocks of VC.FILL and its comparison with the reference applied to `frame`
    -> the pointers, the layout, the stored planes"""
    h, w = frame.shape[:2]
    case = (f"{w} x {h} rect {rect} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", w, h, rect, fmt, m, r, flags, layout)
    lay = VC.layouts(case)
    alloc = alloc or memory.filled
    sizes = [VC.plane_bytes(pitch, rows, row_bytes) for _, pitch, rows, row_bytes in lay]
    ptrs = [alloc(n, align) for n, (align, _, _, _) in zip(sizes, lay)]
    ctx.read_video_422(three_of(ptrs), three_of([l[1] for l in lay]), format=fmt, matrix=m, range=r, flags=flags, rect=rect)
    want = VC.expected_planes(case, frame)
    got = [memory.download(ptr, n) for ptr, n in zip(ptrs, sizes)]
    for p, (a, b) in enumerate(zip(got, want)):
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{case[0]}: plane {p} differs in {int((a != b).sum())} bytes, the first at {at} (pitch {lay[p][1]}): {a[at]} != {b[at]}")
    return ptrs, lay, VC.stored_of(got, case)


CLEARS = (OPAQUE, TRANSPARENT)


@pytest.mark.parametrize("w,h", VC.OUT_SIZES, ids=[f"{w}x{h}" for w, h in VC.OUT_SIZES])
def test_every_kind_and_layout_against_the_reference(memory, w, h):
    """every format x chroma rule x layout, the rows of the coefficient table dealt out over them; a packed plane is the I422 call's planes
    of the same matrix, range and rule interleaved"""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=512, device=0)
    frame = render(ctx, w, h, CLEARS[(w + h) & 1])
    n, planar = 0, {}
    for li, layout in enumerate(VC.LAYOUTS):
        for ki, (fmt, flags) in enumerate(VC.KINDS):
            m, r = VC.MATRIX_RANGE[(flags + li + w) % 6]  # (the four formats of a rule and a layout share the row)
            _, _, stored = export(ctx, memory, frame, fmt, m, r, flags, layout)
            if fmt == REF.I422:
                planar[(flags, layout)] = stored
            if REF.packed(fmt):
                assert np.array_equal(stored[0], REF.interleave(planar[(flags, layout)], fmt)), (fmt, flags, layout)
            n += 1
    assert n == 24 and np.array_equal(ctx.read_pixels(), frame)  # the frame is untouched
    ctx.close()
    memory.free()


@pytest.mark.parametrize("w,h", [(2, 1), (9, 2), (33, 7), (257, 9)], ids=lambda v: str(v))  # (an image of one column stores nothing)
def test_planar_chroma_is_the_420_chroma_of_a_frame_with_doubled_rows(memory, w, h):
    """a frame of 2 h rows, rows 2 y and 2 y + 1 equal: fdh_read_video_planes' I420 / I010 chroma planes, h rows, are the chroma planes
    fdh_read_video_422 writes for rows 0, 2, .. of that frame -- and every row of its 4:2:2 chroma occurs twice"""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=1024, device=0)
    frame = render(ctx, w, h, OPAQUE, double=True)
    assert frame.shape == (2 * h, w, 4) and np.array_equal(frame[0::2], frame[1::2])
    cw = (w + 1) // 2
    for k, ((fmt, sib), flags) in enumerate(((p, f) for p in ((REF.I422, PL.I420), (REF.I210, PL.I010)) for f in (0, REF.CHROMA_LINEAR))):
        m, r = VC.MATRIX_RANGE[(k + w) % 6]
        _, _, (y2, cb2, cr2) = export(ctx, memory, frame, fmt, m, r, flags, "tight")
        es = 1 if fmt == REF.I422 else 2
        ptrs = [memory.filled(2 * h * w * es), memory.filled(h * cw * es), memory.filled(h * cw * es)]
        ctx.read_video_planes(ptrs, (w * es, cw * es, cw * es), format=sib, matrix=m, range=r, flags=flags)
        dt = REF.dtype_of(fmt)
        y0 = memory.download(ptrs[0], 2 * h * w * es).view(dt).reshape(2 * h, w)
        cb0, cr0 = (memory.download(p, h * cw * es).view(dt).reshape(h, cw) for p in ptrs[1:])
        assert np.array_equal(y0, y2) and np.array_equal(np.repeat(cb0, 2, axis=0), cb2) and np.array_equal(np.repeat(cr0, 2, axis=0), cr2), (fmt, flags)
    ctx.close()
    memory.free()


def test_rectangles_are_the_export_of_the_cropped_frame(memory):
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=256, device=0)
    frame = render(ctx, *VC.RECT_SOURCE, TRANSPARENT)
    for k, rect in enumerate(VC.RECTS):
        assert np.array_equal(ctx.read_pixels(*rect), VC.cropped(frame, rect))
        for ki, (fmt, flags) in enumerate(VC.KINDS):
            m, r = VC.MATRIX_RANGE[(k + ki) % 6]
            export(ctx, memory, frame, fmt, m, r, flags, VC.LAYOUTS[(k + ki) % 3], rect=rect)
    assert np.array_equal(ctx.read_pixels(), frame)
    ctx.close()


def test_a_page_locked_destination(memory):
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=256, device=0)
    frame = render(ctx, 71, 45, OPAQUE)
    pinned = Memory()
    pinned.download = lambda ptr, n: np.ctypeslib.as_array((C.c_uint8 * n).from_address(ptr)).copy()
    try:
        for fmt, flags, layout in ((REF.I422, REF.CHROMA_LINEAR, "tight"), (REF.YUY2, 0, "padded"), (REF.I210, 0, "aligned"), (REF.UYVY, REF.CHROMA_LINEAR, "aligned")):
            export(ctx, pinned, frame, fmt, REF.BT2020, REF.LIMITED, flags, layout, alloc=lambda n, align: pinned.page_locked(n + align) + align)
    finally:
        pinned.free()
    ctx.close()


def test_the_exported_planes_go_back_in_through_put_video_422(memory):
    """closing the loop on the device: context A's planes are context B's source; level 0 of B's atlas holds what the reference makes of A's
    frame there and back, byte for byte"""
    from figdraw_amd.context import HipContext

    a, b = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    frame = render(a, 71, 45, OPAQUE)
    kinds = [(REF.I422, REF.BT709, REF.LIMITED, 0, "tight"), (REF.I210, REF.BT601, REF.FULL, REF.CHROMA_LINEAR, "padded"),
             (REF.YUY2, REF.BT2020, REF.LIMITED, REF.CHROMA_LINEAR, "aligned"), (REF.UYVY, REF.BT709, REF.FULL, 0, "padded")]
    for key, (fmt, m, r, flags, layout) in enumerate(kinds, start=1):
        ptrs, lay, _ = export(a, memory, frame, fmt, m, r, flags, layout)
        x, y, w, h = b.put_video_422(key, three_of(ptrs), 71, 45, three_of([l[1] for l in lay]), format=fmt, matrix=m, range=r, flags=flags)
        want = REF.convert(REF.export(frame, fmt, m, r, flags), fmt, m, r, flags, w=71)
        got = b.read_atlas_level(0)[y:y + h, x:x + w]
        assert np.array_equal(got, want), (fmt, m, r, flags)
        print(f"{REF.NAMES[fmt]} m{m} r{r} f{flags}: max |back - frame| = {int(np.abs(got.astype(int) - frame.astype(int))[..., :3].max())} on rendered noise")
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------------ refusals: each in front of any launch
def test_refusals_on_a_device_context(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    sizes = (16 * 9, 8 * 9, 8 * 9)
    good = [memory.filled(n) for n in sizes]
    pitches = (16, 8, 8)

    def refused(text, ptrs, pitches=pitches, **kw):
        with pytest.raises(FigdrawHipError) as e:
            ctx.read_video_422(ptrs, pitches, **kw)
        assert e.value.code == -1 and str(e.value).split("] ", 1)[1].startswith("read_video_422: ") and text in str(e.value), str(e.value)
        assert all((memory.download(p, n) == VC.FILL).all() for p, n in zip(good, sizes))

    def with_plane(p, ptr):
        ptrs = list(good)
        ptrs[p] = ptr
        return ptrs

    refused("no frame has been submitted", good)
    frame = render(ctx, 16, 9, OPAQUE)
    # pageable host memory, for every plane and for the one packed plane
    pageable = [np.full(n, VC.FILL, np.uint8) for n in sizes]
    for p in range(3):
        refused("neither device memory of the context's device nor page-locked host memory", with_plane(p, pageable[p].ctypes.data))
    packed_host = np.full(32 * 9, VC.FILL, np.uint8)
    refused("neither device memory of the context's device nor page-locked host memory", [packed_host.ctypes.data, 0, 0], (32, 0, 0), format=REF.UYVY)
    assert all((a == VC.FILL).all() for a in pageable) and (packed_host == VC.FILL).all()
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    # a plane inside the context's own surface
    surface = ctx.frame_device_ptr()[0]
    for p in range(3):
        refused("a plane overlaps the context's own frame surface", with_plane(p, surface + 16 * 9 * 4 - 2))
    refused("a plane overlaps the context's own frame surface", [surface + 16, 0, 0], (32, 0, 0), format=REF.YUY2)
    # two planes in one block, one inside the other's bytes
    refused("planes 1 and 2 overlap", with_plane(2, good[1] + 8 * 9 - 1))
    # the rules that need no device hold here too
    refused("the rectangle's x must be even", good, rect=(1, 0, 4, 4))
    refused("rectangle outside the frame", good, rect=(2, 0, 16, 9))
    refused("unknown format", good, format=PL.I420)
    refused("planes[1], planes[2] and their pitches must be 0", good, format=REF.YUY2)
    # under a row stripe
    ctx.set_stripe(0, 4)
    refused("not under fdh_set_stripe", good)
    ctx.set_stripe(0, 0)
    assert np.array_equal(ctx.read_pixels(), frame)
    # and the context works on: an odd y is fine
    ctx.read_video_422(good, pitches, rect=(2, 3, 13, 5))
    want = REF.export(frame[3:8, 2:15], REF.I422, REF.BT709, REF.LIMITED)
    for ptr, pitch, plane in zip(good, pitches, want):
        got = memory.download(ptr, pitch * 5).reshape(5, pitch)
        assert np.array_equal(got[:, :plane.shape[1]], plane) and (got[:, plane.shape[1]:] == VC.FILL).all()
    ctx.close()
