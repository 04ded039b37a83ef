"""Three-plane video in and out on the device (fdh_put_video_planes, fdh_update_video_planes, fdh_read_video_planes;
k_video_planar_import, k_video_planar_export; include_video/figdraw_hip_video_planar.h).  The bar is identity both ways.  The way in: a
context that gets I420, I010, I444 and I410 frames from device memory against one that gets, through fdh_put_image, the bytes the reference
tests/video_planar_ref.py makes of them, and against one that gets the 4:2:0 frames interleaved through fdh_put_video_frame -- every level
of the atlases, the draw records (the ink boxes shrink the draws) and a rendered frame.  The way out: the three planes against the
reference applied to what fdh_read_pixels returns of the same frame, from each plane's pointer to its last sample's end, the padding
untouched; the 4:2:0 planes also against fdh_read_video_frame's NV12 and P010 planes."""
import ctypes as C

import numpy as np
import pytest

import video_frame_ref as SIB_IN
import video_out_cases as OC
import video_out_ref as SIB_OUT
import video_planar_cases as VC
import video_planar_ref as REF

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


# ------------------------------------------------------------------------------------------------------------------ the way in
def put_case(ctx, memory, key, case, update=False, place=None, swap=False):
    """`place`: how a plane's bytes get an address (memory.upload by default); `swap`: the chroma pointers and pitches swapped (YV12)"""
    w, h = VC.size_of(case)
    place = place or memory.upload
    packed = VC.pack(case)
    ptrs, pitches = [place(data, align) for data, align, _ in packed], [pitch for _, _, pitch in packed]
    if swap:
        ptrs, pitches = [ptrs[0], ptrs[2], ptrs[1]], [pitches[0], pitches[2], pitches[1]]
    call = ctx.update_video_planes if update else ctx.put_video_planes
    return call(key, ptrs, w, h, pitches, format=case[1], matrix=case[2], range=case[3], flags=case[4])


def put_interleaved(ctx, memory, key, case, update=False):
    """the same samples through the sibling: fdh_put_video_frame of the NV12 / P010 frame, tightly packed"""
    w, h = VC.size_of(case)
    sib, luma, chroma = VC.interleaved(case)
    call = ctx.update_video_frame if update else ctx.put_video_frame
    return call(key, memory.upload(luma.tobytes()), memory.upload(chroma.tobytes()), w, h, luma.strides[0], chroma.strides[0], format=sib, matrix=case[2], range=case[3], flags=case[4])


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
    """every case into one atlas of 2048 on three fresh contexts: the planar call; fdh_put_image of the reference's texels; and the sibling
    call on the interleaved frame for 4:2:0 (fdh_put_image for 4:4:4, which has no sibling) -> cases, contexts, the rectangles"""
    from figdraw_amd.context import HipContext

    cases = VC.in_cases()
    dev, host, sib = (HipContext(atlas_size=2048, device=0) for _ in range(3))
    rects = []
    for i, case in enumerate(cases):
        texels = VC.texels(case)
        r = put_case(dev, memory, 100 + i, case)
        assert r == host.put_image(100 + i, texels), case[0]
        assert r == (sib.put_image(100 + i, texels) if REF.full_chroma(case[1]) else put_interleaved(sib, memory, 100 + i, case)), case[0]
        assert r[2:] == VC.size_of(case) and dev.image_rect(100 + i) == r
        rects.append(r)
    assert dev.atlas_size() == 2048
    yield cases, dev, host, sib, rects
    dev.close(), host.close(), sib.close()


def test_rectangles_usage_and_every_level(three):
    cases, dev, host, sib, rects = three
    assert len(cases) >= 36
    same_atlases(dev, host, "all cases, against fdh_put_image")
    same_atlases(dev, sib, "all cases, against fdh_put_video_frame")
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
        if REF.full_chroma(case[1]):
            sib.update_image(100 + i, texels)
        else:
            put_interleaved(sib, memory, 100 + i, case, update=True)
    same_atlases(dev, host, "all cases updated, against fdh_update_image")
    same_atlases(dev, sib, "all cases updated, against fdh_update_video_frame")
    for ctx in (dev, host):
        _frame(ctx, nxt, rects)
    assert dev.record_digest() == host.record_digest()
    assert np.array_equal(dev.read_pixels(), host.read_pixels())


def small_case(fmt, flags, w, h, seed, layout="padded", matrix=REF.BT601, rng=REF.FULL):
    return (f"{REF.NAMES[fmt]} {w} x {h} seed {seed}", fmt, matrix, rng, flags, VC.noise_planes(np.random.default_rng(seed), fmt, w, h), layout)


def test_yv12_is_swapped_pointers(memory):
    from figdraw_amd.context import HipContext

    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    case = small_case(REF.I420, REF.CHROMA_LINEAR, 70, 45, 21)
    y, cb, cr = case[5]
    swapped = (case[0] + " swapped",) + case[1:5] + ((y, cr, cb),) + case[6:]
    assert not np.array_equal(VC.texels(case), VC.texels(swapped))
    assert put_case(dev, memory, 1, case, swap=True) == host.put_image(1, VC.texels(swapped))
    same_atlases(dev, host, "YV12")
    dev.close(), host.close()


def test_page_locked_host_memory_is_a_source(memory):
    from figdraw_amd.context import HipContext

    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    for key, (fmt, flags) in enumerate(((REF.I010, REF.CHROMA_LINEAR), (REF.I444, 0)), start=1):
        case = small_case(fmt, flags, 70, 45, 30 + key, layout="tight", matrix=REF.BT2020, rng=REF.LIMITED)
        assert put_case(dev, memory, key, case, place=lambda data, align: memory.page_locked(len(data), data)) == host.put_image(key, VC.texels(case))
    same_atlases(dev, host, "page-locked")
    dev.close(), host.close()


def test_pageable_host_memory_is_refused_for_every_plane(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    host_planes = [np.zeros((9, 16), np.uint8), np.zeros((5, 8), np.uint8), np.zeros((5, 8), np.uint8)]
    good = [memory.upload(p.tobytes()) for p in host_planes]
    assert ctx.put_video_planes(1, good, 16, 9, (16, 8, 8))[2:] == (16, 9)
    before = ctx.atlas_usage()
    for p in range(3):
        ptrs = list(good)
        ptrs[p] = host_planes[p].ctypes.data
        for call in (lambda: ctx.put_video_planes(2, ptrs, 16, 9, (16, 8, 8)), lambda: ctx.update_video_planes(1, ptrs, 16, 9, (16, 8, 8))):
            with pytest.raises(FigdrawHipError) as e:
                call()
            assert e.value.code == -1 and "neither device memory of the context's device nor page-locked host memory" in str(e.value)
            assert ctx.atlas_usage() == before and not ctx.has_image(2)
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    assert ctx.put_video_planes(2, good, 16, 9, (16, 8, 8))[2:] == (16, 9)  # and the context works on
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the way out
def noise(w, h, seed=0):
    """premultiplied noise with every alpha"""
    rng = np.random.default_rng(1000 * w + h + seed)
    img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint16)
    img[..., :3] = img[..., :3] * img[..., 3:] // 255
    return img.astype(np.uint8)


def render(ctx, w, h, clear, seed=0):
    """a few shapes, then the noise image 1:1 over them: neighbouring pixels differ in every channel"""
    ctx.put_image(1, noise(w, h, seed))
    ctx.begin_frame(w, h, True, clear)
    ctx.draw_rect((0.0, 0.0, w * 0.6, h * 0.5), (200, 40, 90, 255))
    ctx.draw_rect((w * 0.3, h * 0.25, w * 0.7, h * 0.75), (10, 220, 160, 180))
    ctx.draw_image(1, (0.0, 0.0), WHITE, (float(w), float(h)))
    ctx.end_frame()
    return ctx.read_pixels()


def export(ctx, memory, frame, fmt, m, r, flags, layout, rect=None, alloc=None):
    """one fdh_read_video_planes into fresh blocks of VC.FILL and its comparison with the reference applied to `frame`
    -> the pointers, the layout, the planes' bytes"""
    h, w = frame.shape[:2]
    case = (f"{w} x {h} rect {rect} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", w, h, rect, fmt, m, r, flags, layout)
    lay = VC.layouts(case)
    alloc = alloc or memory.filled
    sizes = [VC.plane_bytes(pitch, rows, row_bytes) for _, pitch, rows, row_bytes in lay]
    ptrs = [alloc(n, align) for n, (align, _, _, _) in zip(sizes, lay)]
    ctx.read_video_planes(ptrs, [l[1] for l in lay], format=fmt, matrix=m, range=r, flags=flags, rect=rect)
    want = VC.expected_planes(case, frame)
    got = [memory.download(ptr, n) for ptr, n in zip(ptrs, sizes)]
    for p, (a, b) in enumerate(zip(got, want)):
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{case[0]}: plane {p} differs in {int((a != b).sum())} bytes, the first at {at} (pitch {lay[p][1]}): {a[at]} != {b[at]}")
    return ptrs, lay, VC.planes_of(got, case)


def sibling_export(ctx, memory, frame, sib, m, r, flags, rect=None):
    """fdh_read_video_frame of the same frame, tightly packed -> luma (h, w), chroma (ch, cw, 2) as stored"""
    x, y, w, h = rect if rect is not None else (0, 0, frame.shape[1], frame.shape[0])
    cw, ch = (w + 1) // 2, (h + 1) // 2
    es = 1 if sib == SIB_OUT.NV12 else 2
    y_ptr, c_ptr = memory.filled(w * h * es), memory.filled(cw * ch * 2 * es)
    ctx.read_video_frame(y_ptr, c_ptr, w * es, cw * 2 * es, format=sib, matrix=m, range=r, flags=flags, rect=rect)
    dt = np.uint8 if es == 1 else np.uint16
    return memory.download(y_ptr, w * h * es).view(dt).reshape(h, w), memory.download(c_ptr, cw * ch * 2 * es).view(dt).reshape(ch, cw, 2)


def against_the_sibling(ctx, memory, frame, fmt, m, r, flags, planes, rect=None):
    """the I420 planes are the NV12 export de-interleaved, the I010 planes the P010 export >> 6"""
    sib, shift = (SIB_OUT.NV12, 0) if fmt == REF.I420 else (SIB_OUT.P010, 6)
    luma, chroma = sibling_export(ctx, memory, frame, sib, m, r, flags, rect)
    assert np.array_equal(planes[0], luma >> shift) and np.array_equal(planes[1], chroma[..., 0] >> shift) and np.array_equal(planes[2], chroma[..., 1] >> shift), (fmt, m, r, flags, rect)


CLEARS = (OPAQUE, TRANSPARENT)


@pytest.mark.parametrize("w,h", VC.OUT_SIZES, ids=[f"{w}x{h}" for w, h in VC.OUT_SIZES])
def test_every_kind_and_layout_against_the_reference(memory, w, h):
    """every format x chroma rule x layout, the rows of the coefficient table dealt out over them; the 4:2:0 planes also against the sibling"""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=512, device=0)
    frame = render(ctx, w, h, CLEARS[(w + h) & 1])
    n = 0
    for ki, (fmt, flags) in enumerate(VC.KINDS):
        for li, layout in enumerate(VC.LAYOUTS):
            m, r = VC.MATRIX_RANGE[(ki + li + w) % 6]
            _, _, planes = export(ctx, memory, frame, fmt, m, r, flags, layout)
            if not REF.full_chroma(fmt) and layout == "padded":
                against_the_sibling(ctx, memory, frame, fmt, m, r, flags, planes)
            n += 1
    assert n == 18 and np.array_equal(ctx.read_pixels(), frame)  # the frame is untouched
    ctx.close()
    memory.free()


def test_rectangles_are_the_export_of_the_cropped_frame(memory):
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=256, device=0)
    frame = render(ctx, *VC.RECT_SOURCE, TRANSPARENT)
    for k, rect in enumerate(VC.RECTS + VC.ODD_RECTS):
        assert np.array_equal(ctx.read_pixels(*rect), VC.cropped(frame, rect))
        for ki, (fmt, flags) in enumerate(VC.KINDS):
            if rect in VC.ODD_RECTS and not REF.full_chroma(fmt):
                continue
            m, r = VC.MATRIX_RANGE[(k + ki) % 6]
            _, _, planes = export(ctx, memory, frame, fmt, m, r, flags, VC.LAYOUTS[(k + ki) % 3], rect=rect)
            if not REF.full_chroma(fmt):
                against_the_sibling(ctx, memory, frame, fmt, m, r, flags, planes, rect=rect)
    assert np.array_equal(ctx.read_pixels(), frame)
    ctx.close()


def test_a_page_locked_destination(memory):
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=256, device=0)
    frame = render(ctx, 70, 45, OPAQUE)
    pinned = Memory()
    pinned.download = lambda ptr, n: np.ctypeslib.as_array((C.c_uint8 * n).from_address(ptr)).copy()
    try:
        for fmt, flags, layout in ((REF.I420, REF.CHROMA_LINEAR, "tight"), (REF.I410, 0, "padded"), (REF.I010, 0, "aligned")):
            export(ctx, pinned, frame, fmt, REF.BT2020, REF.LIMITED, flags, layout, alloc=lambda n, align: pinned.page_locked(n + align) + align)
    finally:
        pinned.free()
    ctx.close()


def test_the_exported_planes_go_back_in_through_put_video_planes(memory):
    """closing the loop on the device: context A's planes are context B's source; level 0 of B's atlas holds what the reference makes of A's
    frame there and back, byte for byte -- and for 4:4:4 that is within the coding's quantisation of the frame itself"""
    from figdraw_amd.context import HipContext

    a, b = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    frame = render(a, 70, 45, OPAQUE)
    kinds = [(REF.I420, REF.BT709, REF.LIMITED, 0, "tight"), (REF.I010, REF.BT601, REF.FULL, REF.CHROMA_LINEAR, "padded"),
             (REF.I444, REF.BT2020, REF.LIMITED, 0, "aligned"), (REF.I410, REF.BT709, REF.FULL, 0, "padded")]
    for key, (fmt, m, r, flags, layout) in enumerate(kinds, start=1):
        ptrs, lay, _ = export(a, memory, frame, fmt, m, r, flags, layout)
        x, y, w, h = b.put_video_planes(key, ptrs, 70, 45, [l[1] for l in lay], format=fmt, matrix=m, range=r, flags=flags)
        want = REF.convert(REF.export(frame, fmt, m, r, flags), fmt, m, r, flags)
        got = b.read_atlas_level(0)[y:y + h, x:x + w]
        assert np.array_equal(got, want), (fmt, m, r, flags)
        print(f"{REF.NAMES[fmt]} m{m} r{r} f{flags}: max |back - frame| = {int(np.abs(got.astype(int) - frame.astype(int))[..., :3].max())} on rendered noise")
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------------ refusals: each in front of any launch
def test_refusals_on_a_device_context(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    sizes = (16 * 9, 8 * 5, 8 * 5)
    good = [memory.filled(n) for n in sizes]
    pitches = (16, 8, 8)

    def refused(text, ptrs, pitches=pitches, **kw):
        with pytest.raises(FigdrawHipError) as e:
            ctx.read_video_planes(ptrs, pitches, **kw)
        assert e.value.code == -1 and str(e.value).split("] ")[-1].startswith("read_video_planes: ") and text in str(e.value), str(e.value)
        assert all((memory.download(p, n) == VC.FILL).all() for p, n in zip(good, sizes))

    def with_plane(p, ptr):
        ptrs = list(good)
        ptrs[p] = ptr
        return ptrs

    refused("no frame has been submitted", good)
    frame = render(ctx, 16, 9, OPAQUE)
    # pageable host memory, for every plane
    pageable = [np.full(n, VC.FILL, np.uint8) for n in sizes]
    for p in range(3):
        refused("neither device memory of the context's device nor page-locked host memory", with_plane(p, pageable[p].ctypes.data))
    assert all((a == VC.FILL).all() for a in pageable)
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    # a plane inside the context's own surface
    surface = ctx.frame_device_ptr()[0]
    for p in range(3):
        refused("a plane overlaps the context's own frame surface", with_plane(p, surface + 16 * 9 * 4 - 2))
    # two planes in one block, one inside the other's bytes
    refused("planes 1 and 2 overlap", with_plane(2, good[1] + 8 * 5 - 1))
    # the rules that need no device hold here too
    refused("the rectangle's x and y must be even", good, rect=(1, 0, 4, 4))
    refused("rectangle outside the frame", good, rect=(2, 0, 16, 9))
    refused("FDH_VIDEO_CHROMA_LINEAR is for I420 / I010", good, format=REF.I444, flags=REF.CHROMA_LINEAR)
    # under a row stripe
    ctx.set_stripe(0, 4)
    refused("not under fdh_set_stripe", good)
    ctx.set_stripe(0, 0)
    assert np.array_equal(ctx.read_pixels(), frame)
    # and the context works on
    ctx.read_video_planes(good, pitches)
    want = REF.export(frame, REF.I420, REF.BT709, REF.LIMITED)
    for ptr, n, plane in zip(good, sizes, want):
        assert np.array_equal(memory.download(ptr, n), plane.ravel())
    ctx.close()
