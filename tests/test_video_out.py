"""The rendered frame out as NV12, P010 or BGRA8 on the device (fdh_read_video_frame; k_video_export): the planes a context exports
against the reference tests/video_out_ref.py applied to what fdh_read_pixels returns of the same frame.  The bar is identity: every
plane byte for byte from its pointer to its last element's end, the bytes between a row's end and the pitch untouched, the frame
untouched."""
import ctypes as C

import numpy as np
import pytest

import video_frame_ref as IN
import video_out_cases as VC
import video_out_ref as REF

pytestmark = pytest.mark.gpu

WHITE = [(255, 255, 255, 255)] * 4
Z4 = (0.0, 0.0, 0.0, 0.0)
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
        base = self.device(len(data) + align)
        assert self.hip.hipMemcpy(C.c_void_p(base + align), data, C.c_size_t(len(data)), 1) == 0  # host -> device
        return base + align

    def download(self, ptr, n):
        out = np.empty(n, np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(n), 2) == 0  # device -> host
        return out

    def page_locked(self, n):
        p = C.c_void_p()
        assert self.hip.hipHostMalloc(C.byref(p), C.c_size_t(n), 0) == 0
        self.pinned.append(p)
        C.memset(p.value, VC.FILL, n)
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


def noise(w, h, seed=0):
    """premultiplied noise with every alpha"""
    rng = np.random.default_rng(1000 * w + h + seed)
    img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint16)
    img[..., :3] = img[..., :3] * img[..., 3:] // 255
    return img.astype(np.uint8)


def render(ctx, w, h, clear, blur=None, seed=0):
    """a few shapes, then the noise image 1:1 over them: neighbouring pixels differ in every channel (alpha too over a transparent clear)"""
    ctx.put_image(1, noise(w, h, seed))
    ctx.begin_frame(w, h, True, clear)
    ctx.draw_rect((0.0, 0.0, w * 0.6, h * 0.5), (200, 40, 90, 255))
    ctx.draw_rect((w * 0.3, h * 0.25, w * 0.7, h * 0.75), (10, 220, 160, 180))
    ctx.draw_image(1, (0.0, 0.0), WHITE, (float(w), float(h)))
    if blur:
        ctx.draw_backdrop_blur((0.0, 0.0, float(w), float(h)), Z4, Z4, blur)
    ctx.end_frame()
    return ctx.read_pixels()


def export(ctx, memory, frame, fmt, m, r, flags, layout, rect=None, alloc=None):
    """one fdh_read_video_frame into fresh blocks of VC.FILL and its comparison with the reference applied to `frame`"""
    h, w = frame.shape[:2]
    case = (f"{w} x {h} rect {rect} {VC.name_of(fmt)} m{m} r{r} f{flags} {layout}", w, h, rect, fmt, m, r, flags, layout)
    lay = VC.layouts(case)
    alloc = alloc or memory.filled
    sizes = [VC.plane_bytes(pitch, rows, row_bytes) for _, pitch, rows, row_bytes in lay]
    ptrs = [alloc(n, align) for n, (align, _, _, _) in zip(sizes, lay)]
    ctx.read_video_frame(ptrs[0], ptrs[1] if len(ptrs) > 1 else 0, lay[0][1], lay[1][1] if len(lay) > 1 else 0, format=fmt, matrix=m, range=r, flags=flags, rect=rect)
    want = VC.expected_planes(case, frame)
    for p, (ptr, n, b) in enumerate(zip(ptrs, sizes, want)):
        a = memory.download(ptr, n)
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{case[0]}: plane {p} differs in {int((a != b).sum())} bytes, the first at {at} (pitch {lay[p][1]}): {a[at]} != {b[at]}")
    return ptrs, lay


FRAMES = [(1, 1, OPAQUE), (3, 3, TRANSPARENT), (5, 7, OPAQUE), (VC.TILE_W - 1, VC.TILE_H + 1, TRANSPARENT), (VC.TILE_W, VC.TILE_H, OPAQUE),
          (VC.TILE_W + 1, VC.TILE_H - 1, TRANSPARENT)]


@pytest.mark.parametrize("w,h,clear", FRAMES, ids=[f"{w}x{h}" for w, h, _ in FRAMES])
def test_every_kind_and_layout_against_the_reference(memory, w, h, clear):
    """every format x chroma rule (BGRA8: x alpha rule) x layout, the rows of the coefficient table dealt out over them"""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=256, device=0)
    frame = render(ctx, w, h, clear)
    if clear == OPAQUE:
        assert (frame[..., 3] == 255).all()
    elif w > 3:
        assert len(np.unique(frame[..., 3])) > 50  # BGRA8 copies an alpha that varies
    n = 0
    for ki, (fmt, flags) in enumerate(VC.KINDS):
        for li, layout in enumerate(VC.LAYOUTS):
            m, r = (0, 0) if fmt == REF.BGRA8 else VC.MATRIX_RANGE[(ki + li + w) % 6]
            export(ctx, memory, frame, fmt, m, r, flags, layout)
            n += 1
    assert n == 18 and np.array_equal(ctx.read_pixels(), frame)  # the frame is untouched
    ctx.close()


def test_rectangles_are_the_export_of_the_cropped_frame(memory):
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=256, device=0)
    frame = render(ctx, *VC.RECT_SOURCE, TRANSPARENT)
    for k, rect in enumerate(VC.RECTS + VC.ODD_RECTS):
        for fmt, flags in VC.KINDS:
            if rect in VC.ODD_RECTS and fmt != REF.BGRA8:
                continue
            m, r = (0, 0) if fmt == REF.BGRA8 else VC.MATRIX_RANGE[(k + fmt + flags) % 6]
            assert np.array_equal(ctx.read_pixels(*rect), VC.cropped(frame, rect))
            export(ctx, memory, frame, fmt, m, r, flags, VC.LAYOUTS[(k + fmt + flags) % 3], rect=rect)
    assert np.array_equal(ctx.read_pixels(), frame)
    ctx.close()


def test_a_frame_that_ends_in_the_other_surface_and_the_frame_after_it(memory):
    """1024 x 384 with a full-frame backdrop blur on the one-kernel route renders out of place: the frame lies in the second surface.
    Each export matches its own fdh_read_pixels"""
    from figdraw_amd.context import HipContext

    w, h = 1024, 384
    ctx = HipContext(atlas_size=1024, device=0)
    ctx.set_blur_route(1)
    first = render(ctx, w, h, OPAQUE)
    at = ctx.frame_device_ptr()[0]
    blurred = render(ctx, w, h, OPAQUE, blur=16.0, seed=1)
    moved = ctx.frame_device_ptr()[0]
    assert moved != at, "the blurred frame did not end in the other surface"
    assert not np.array_equal(first, blurred)
    export(ctx, memory, blurred, REF.NV12, REF.BT709, REF.LIMITED, REF.CHROMA_LINEAR, "tight")
    export(ctx, memory, blurred, REF.BGRA8, 0, 0, 0, "aligned", rect=(511, 101, 130, 18))
    after = render(ctx, w, h, TRANSPARENT, seed=2)
    export(ctx, memory, after, REF.P010, REF.BT2020, REF.FULL, 0, "padded")
    export(ctx, memory, after, REF.NV12, REF.BT601, REF.FULL, 0, "aligned", rect=(2, 2, 1000, 380))
    assert np.array_equal(ctx.read_pixels(), after)
    ctx.close()


def test_a_page_locked_destination(memory):
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=256, device=0)
    frame = render(ctx, 70, 45, OPAQUE)
    pinned = Memory()
    pinned.download = lambda ptr, n: np.ctypeslib.as_array((C.c_uint8 * n).from_address(ptr)).copy()
    try:
        export(ctx, pinned, frame, REF.NV12, REF.BT2020, REF.LIMITED, REF.CHROMA_LINEAR, "tight", alloc=lambda n, align: pinned.page_locked(n + align) + align)
        export(ctx, pinned, frame, REF.P010, REF.BT709, REF.LIMITED, 0, "padded", alloc=lambda n, align: pinned.page_locked(n + align) + align)
    finally:
        pinned.free()
    ctx.close()


def test_the_exported_planes_go_back_in_through_put_video_frame(memory):
    """closing the loop on the device: context A's planes are context B's decoder surface; level 0 of B's atlas holds what the two references
    make of A's frame, byte for byte"""
    from figdraw_amd.context import HipContext

    a, b = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    frame = render(a, 70, 45, OPAQUE)
    kinds = [(REF.NV12, REF.BT709, REF.LIMITED, 0, "tight"), (REF.NV12, REF.BT601, REF.FULL, REF.CHROMA_LINEAR, "padded"),
             (REF.P010, REF.BT2020, REF.LIMITED, REF.CHROMA_LINEAR, "aligned"), (REF.BGRA8, 0, 0, 0, "padded")]
    for key, (fmt, m, r, flags, layout) in enumerate(kinds, start=1):
        ptrs, lay = export(a, memory, frame, fmt, m, r, flags, layout)
        x, y, w, h = b.put_video_frame(key, ptrs[0], ptrs[1] if len(ptrs) > 1 else 0, 70, 45, lay[0][1], lay[1][1] if len(lay) > 1 else 0, format=fmt, matrix=m, range=r, flags=flags)
        want = IN.convert(*REF.export(frame, fmt, m, r, flags), fmt, m, r, flags)
        got = b.read_atlas_level(0)[y:y + h, x:x + w]
        assert np.array_equal(got, want), (fmt, m, r, flags)
        if fmt == REF.BGRA8:
            assert np.array_equal(got, frame)  # and BGRA8 is lossless
        else:
            print(f"{VC.name_of(fmt)} m{m} r{r} f{flags}: max |back - frame| = {int(np.abs(got.astype(int) - frame.astype(int))[..., :3].max())} on rendered noise")
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------------ refusals: each in front of any launch
def untouched(memory, ptr, n):
    return bool((memory.download(ptr, n) == VC.FILL).all())


def test_refusals_on_a_device_context(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    y_ptr, uv_ptr = memory.filled(16 * 9), memory.filled(16 * 5)

    def refused(text, *args, **kw):
        with pytest.raises(FigdrawHipError) as e:
            ctx.read_video_frame(*args, **kw)
        assert e.value.code == -1 and str(e.value).split("] ")[-1].startswith("read_video_frame: ") and text in str(e.value), str(e.value)
        assert untouched(memory, y_ptr, 16 * 9) and untouched(memory, uv_ptr, 16 * 5)

    refused("no frame has been submitted", y_ptr, uv_ptr, 16, 16)
    frame = render(ctx, 16, 9, OPAQUE)
    # pageable host memory, for either plane
    luma, chroma = np.full((9, 16), VC.FILL, np.uint8), np.full((5, 8, 2), VC.FILL, np.uint8)
    refused("neither device memory of the context's device nor page-locked host memory", luma.ctypes.data, uv_ptr, 16, 16)
    refused("neither device memory of the context's device nor page-locked host memory", y_ptr, chroma.ctypes.data, 16, 16)
    assert (luma == VC.FILL).all() and (chroma == VC.FILL).all()
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    # a plane inside the context's own surface
    surface = ctx.frame_device_ptr()[0]
    refused("a plane overlaps the context's own frame surface", surface, uv_ptr, 16, 16)
    refused("a plane overlaps the context's own frame surface", y_ptr, surface + 16 * 9 * 4 - 2, 16, 16)
    refused("a plane overlaps the context's own frame surface", surface + 64, 0, 64, 0, format=REF.BGRA8, matrix=0, range=0, rect=(0, 0, 16, 8))
    # the rules that need no device hold here too
    refused("the rectangle's x and y must be even", y_ptr, uv_ptr, 16, 16, rect=(1, 0, 4, 4))
    refused("rectangle outside the frame", y_ptr, uv_ptr, 16, 16, rect=(2, 0, 16, 9))
    # under a row stripe
    ctx.set_stripe(0, 4)
    refused("not under fdh_set_stripe", y_ptr, uv_ptr, 16, 16)
    ctx.set_stripe(0, 0)
    assert np.array_equal(ctx.read_pixels(), frame)
    # and the context works on
    ctx.read_video_frame(y_ptr, uv_ptr, 16, 16)
    want = REF.export(frame, REF.NV12, REF.BT709, REF.LIMITED)
    assert np.array_equal(memory.download(y_ptr, 16 * 9).reshape(9, 16), want[0]) and np.array_equal(memory.download(uv_ptr, 16 * 5).reshape(5, 8, 2), want[1])
    ctx.close()


def test_a_plane_on_another_device_is_refused(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    n = C.c_int()
    assert memory.hip.hipGetDeviceCount(C.byref(n)) == 0
    if n.value < 2:
        pytest.skip("one device")
    ctx = HipContext(atlas_size=256, device=0)
    render(ctx, 16, 9, OPAQUE)
    assert memory.hip.hipSetDevice(1) == 0
    other = memory.device(16 * 9)
    assert memory.hip.hipSetDevice(0) == 0
    here = memory.device(16 * 9)
    for y_ptr, uv_ptr in ((other, here), (here, other)):
        with pytest.raises(FigdrawHipError) as e:
            ctx.read_video_frame(y_ptr, uv_ptr, 16, 16)
        assert e.value.code == -1 and "neither device memory of the context's device" in str(e.value)
    ctx.close()


def test_the_order_of_the_refusals_that_need_the_device(memory):
    """the device half of the four calls asks plane by plane, in plane order -- whether the plane can be addressed, then whether it touches
    memory of the context's own -- and the planes' overlap with each other last; a plane a format does not have is not asked.  A refused
    call writes nothing: every block, the pageable array and the frame are as they were"""
    from figdraw_amd.context import VIDEO_A444, VIDEO_UYVA, FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    frame = render(ctx, 16, 9, OPAQUE)
    surface = ctx.frame_device_ptr()[0]
    pageable = np.full(512, VC.FILL, np.uint8)
    block = memory.filled(4 * 512)  # a plane of the 16 x 9 frame has at most 288 bytes
    calls = [  # the call, which planes the format has, the text for planes that overlap each other
        ("read_video_frame", lambda p: ctx.read_video_frame(p[0], p[1], 16, 16), (1, 1), "the two planes overlap"),
        ("read_video_planes", lambda p: ctx.read_video_planes(p, (16, 8, 8)), (1, 1, 1), "planes 0 and 1 overlap"),
        ("read_video_422", lambda p: ctx.read_video_422(p, (16, 8, 8)), (1, 1, 1), "planes 0 and 1 overlap"),
        ("read_video_alpha", lambda p: ctx.read_video_alpha(p, (16, 16, 16, 16), format=VIDEO_A444), (1, 1, 1, 1), "planes 0 and 1 overlap"),
        ("read_video_alpha", lambda p: ctx.read_video_alpha(p, (32, 0, 0, 16), format=VIDEO_UYVA), (1, 0, 0, 1), "planes 0 and 3 overlap"),
    ]
    n = 0
    for name, call, present, overlap in calls:
        valid = [block + 512 * p if there else 0 for p, there in enumerate(present)]
        second = present.index(1, 1)  # the format's next plane after plane 0

        def refused(text, plane_0, plane_second):
            nonlocal n
            ptrs = list(valid)
            ptrs[0], ptrs[second] = plane_0, plane_second
            with pytest.raises(FigdrawHipError) as e:
                call(ptrs)
            assert e.value.code == -1 and str(e.value).endswith(f"{name}: {text}"), str(e.value)
            assert untouched(memory, block, 4 * 512) and (pageable == VC.FILL).all()
            n += 1

        refused("a plane is neither device memory of the context's device nor page-locked host memory", pageable.ctypes.data, surface)
        refused("a plane overlaps the context's own frame surface", surface, pageable.ctypes.data)
        refused(overlap, valid[0], valid[0] + 4)
    assert n == 15 and memory.hip.hipGetLastError() == 0
    assert np.array_equal(ctx.read_pixels(), frame)
    ctx.close()
