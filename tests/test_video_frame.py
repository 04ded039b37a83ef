"""Decoded video frames on the device (fdh_put_video_frame, fdh_update_video_frame; k_video_import, k_image_import_tail): a context that
gets NV12, P010 and BGRA8 frames from device memory against a second one that gets, through fdh_put_image / fdh_update_image, the bytes
the reference tests/video_frame_ref.py makes of the same frames.  The bar is identity: rectangles, usage, every level of both atlases byte
for byte, the draw records; rendered frames also against the oracle within the suite's bar of 1 LSB on at most 0.5 % of the pixels."""
import ctypes as C
import os

import numpy as np
import pytest

import video_frame_cases as VC
import video_frame_ref as REF

pytestmark = pytest.mark.gpu

WHITE = [(255, 255, 255, 255)] * 4


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

    def upload(self, data: bytes, align=0):
        """`data` in device memory at an address `align` past a 256-byte boundary, in a block that ends with it"""
        base = self.device(len(data) + align)
        assert self.hip.hipMemcpy(C.c_void_p(base + align), data, C.c_size_t(len(data)), 1) == 0  # host -> device
        return base + align

    def page_locked(self, data: bytes):
        p = C.c_void_p()
        assert self.hip.hipHostMalloc(C.byref(p), C.c_size_t(len(data)), 0) == 0
        self.pinned.append(p)
        C.memmove(p.value, data, len(data))
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


def put_case(ctx, memory, key, case, update=False, place=None):
    """`place`: how a plane's bytes get an address (memory.upload by default)"""
    w, h = VC.size_of(case)
    (ybuf, yalign, ypitch), c = VC.pack(case)
    place = place or memory.upload
    y_ptr = place(ybuf, yalign)
    uv_ptr, cpitch = (place(c[0], c[1]), c[2]) if c else (0, 0)
    call = ctx.update_video_frame if update else ctx.put_video_frame
    return call(key, y_ptr, uv_ptr, w, h, ypitch, cpitch, format=case[1], matrix=case[2], range=case[3], flags=case[4])


def nv12(rng, w, h, flags=0, layout="tight", name="frame", matrix=REF.BT709, rgn=REF.LIMITED):
    luma, chroma = VC.noise_yuv(rng, REF.NV12, w, h)
    return (f"{name} {w} x {h}", REF.NV12, matrix, rgn, flags, luma, chroma, layout)


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


def against_oracle(got, want, what):
    d = np.abs(got.astype(int) - want.astype(int)).max(axis=2)
    print(f"{what}: max |hip - oracle| = {d.max()} LSB on {int((d > 0).sum())} of {d.size} pixels")
    assert d.max() <= 1 and (d > 0).sum() <= 0.005 * d.size, what


# ------------------------------------------------------------------------------------------------------------------ equality with the host path
@pytest.fixture(scope="module")
def both(memory):
    """every case into one atlas of 2048 on either path, and into the oracle's -> cases, contexts, the rectangles"""
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    cases = VC.cases()
    dev, host, orc = HipContext(atlas_size=2048, device=0), HipContext(atlas_size=2048, device=0), O.Oracle(atlas_size=2048, threads=8)
    rects = []
    for i, case in enumerate(cases):
        texels = VC.texels(case)
        r = put_case(dev, memory, 100 + i, case)
        assert r == host.put_image(100 + i, texels) == tuple(orc.put_image(100 + i, texels)), case[0]
        assert r[2:] == VC.size_of(case)
        rects.append(r)
    assert dev.atlas_size() == 2048
    yield cases, dev, host, orc, rects
    dev.close(), host.close()


def test_rectangles_usage_and_every_level(both):
    cases, dev, host, orc, rects = both
    assert len(cases) >= 36
    same_atlases(dev, host, "all cases")
    level0 = dev.read_atlas_level(0)
    for case, (x, y, w, h) in zip(cases, rects):  # and level 0 is the reference's conversion (nothing of a line)
        want = VC.texels(case) if w > 1 and h > 1 else np.zeros((h, w, 4), np.uint8)
        assert np.array_equal(level0[y:y + h, x:x + w], want), case[0]


def _frame(ctx, cases, rects):
    """every image up to 128 x 128 at 1:1 and magnified 2.5 times (the draws shrink to the ink boxes), the larger ones minified"""
    W, H = 2000, 1500
    ctx.begin_frame(W, H, True, (0.1, 0.2, 0.3, 1.0))
    x, y, row = 4.0, 4.0, 0.0
    n = 0
    for i, (case, r) in enumerate(zip(cases, rects)):
        w, h = r[2:]
        scales = (0.25,) if w > 128 or h > 128 else (1.0, 2.5)
        for s in scales:
            if x + w * s > W - 4:
                x, y, row = 4.0, y + row + 3.0, 0.0
            ctx.draw_image(100 + i, (x + 0.25 * (i % 3), y), WHITE, (w * s, h * s), i % 7 == 3)
            x += w * s + 3.0
            row = max(row, h * s)
            n += 1
    assert y + row < H
    ctx.end_frame()
    return n


def test_draw_records_and_frames(both):
    cases, dev, host, orc, rects = both
    for ctx in (dev, host, orc):
        n = _frame(ctx, cases, rects)
    assert n > 80
    assert dev.record_digest() == host.record_digest()
    got = dev.read_pixels()
    assert np.array_equal(got, host.read_pixels())
    against_oracle(got, orc.read_pixels(), "all cases")


def test_updates_of_every_case(both, memory):
    """(behind the tests of the puts: it changes the fixture's atlases) every entry gets the next frame on either path"""
    from oracle import oracle as O

    cases, dev, host, _, rects = both
    nxt = VC.cases(again=True)
    orc = O.Oracle(atlas_size=2048, threads=8)  # (the oracle has no update: a fresh one takes the new texels into the same rectangles)
    for i, case in enumerate(nxt):
        texels = VC.texels(case)
        assert not np.array_equal(texels, VC.texels(cases[i])), case[0]
        put_case(dev, memory, 100 + i, case, update=True)
        host.update_image(100 + i, texels)
        assert tuple(orc.put_image(100 + i, texels)) == rects[i]
    same_atlases(dev, host, "all cases updated")
    for ctx in (dev, host, orc):
        _frame(ctx, nxt, rects)
    assert dev.record_digest() == host.record_digest()
    got = dev.read_pixels()
    assert np.array_equal(got, host.read_pixels())
    against_oracle(got, orc.read_pixels(), "all cases updated")


def test_ink_boxes_shrink_the_draws(memory):
    """a frame whose ink is one texel (BGRA8, everything else transparent): the draw record is the host path's, and not that of a full one"""
    from figdraw_amd.context import HipContext

    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    corner = np.zeros((100, 100, 4), np.uint8)
    corner[99, 0] = (9, 9, 9, 255)
    full = np.full((100, 100, 4), 255, np.uint8)
    digests = []
    for img in (corner, full):
        for ctx in (dev, host):
            ctx.reset_atlas(0)
        case = ("ink", REF.BGRA8, 0, 0, 0, img, None, "tight")
        assert put_case(dev, memory, 1, case) == host.put_image(1, VC.texels(("ink %d" % len(digests),) + case[1:]))
        for ctx in (dev, host):
            ctx.begin_frame(400, 300, True, (0, 0, 0, 1))
            ctx.draw_image(1, (10.0, 20.0), WHITE, (250.0, 250.0))
            ctx.end_frame()
        assert np.array_equal(dev.read_pixels(), host.read_pixels())
        digests.append((dev.record_digest(), host.record_digest()))
    assert digests[0][0] == digests[0][1] and digests[1][0] == digests[1][1] and digests[0][0] != digests[1][0]
    dev.close(), host.close()


def test_source_beyond_the_tail(memory):
    """2100 x 40 in an atlas of 4096: the level-5 image is 66 texels wide and takes a k_minify2 step before the tail's workgroup holds it"""
    from figdraw_amd.context import HipContext

    case = nv12(np.random.default_rng(4), 2100, 40, flags=REF.CHROMA_LINEAR, name="beyond the tail")
    dev, host = HipContext(atlas_size=4096, device=0), HipContext(atlas_size=4096, device=0)
    assert put_case(dev, memory, 1, case) == host.put_image(1, VC.texels(case))
    same_atlases(dev, host, case[0])
    assert dev.read_atlas_level(5).any()
    dev.close(), host.close()


def test_entries_against_the_right_and_bottom_edges(memory):
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(12)
    dev, host = HipContext(atlas_size=128, device=0), HipContext(atlas_size=128, device=0)
    for key, (w, h) in enumerate(((119, 60), (119, 44)), start=1):
        case = nv12(rng, w, h, flags=key & 1, layout="padded", name=f"edge {key}", matrix=REF.BT601, rgn=REF.FULL)
        r = put_case(dev, memory, key, case)
        assert r == host.put_image(key, VC.texels(case)) and r[0] + r[2] == 123
    assert r[1] + r[3] == 124 and dev.atlas_size() == 128
    same_atlases(dev, host, "edges")
    dev.close(), host.close()


# ------------------------------------------------------------------------------------------------------------------ life cycle
def test_update_of_a_flippy_entry(memory):
    from conftest import GOLDEN
    from figdraw_amd.context import HipContext

    data = open(os.path.join(GOLDEN, "img1.flippy"), "rb").read()
    luma, chroma = VC.noise_yuv(np.random.default_rng(13), REF.P010, 100, 100)
    case = ("update of a flippy", REF.P010, REF.BT2020, REF.LIMITED, REF.CHROMA_LINEAR, luma, chroma, "padded")
    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    assert dev.put_flippy(1, data) == host.put_flippy(1, data) == (4, 4, 100, 100)
    put_case(dev, memory, 1, case, update=True)
    host.update_image(1, VC.texels(case))
    same_atlases(dev, host, "updated")
    assert dev.compact_atlas(512)["rects_moved"] == host.compact_atlas(512)["rects_moved"]  # a chain entry now: the move makes its levels again
    same_atlases(dev, host, "compacted")
    dev.close(), host.close()


@pytest.mark.parametrize("keep", [False, True])
def test_put_that_grows_the_atlas(memory, keep):
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(14)
    small = nv12(rng, 20, 20, name=f"small, keep {keep}")
    case = nv12(rng, 100, 70, flags=REF.CHROMA_LINEAR, layout="padded", name=f"grows, keep {keep}")
    dev, host = HipContext(atlas_size=64, device=0), HipContext(atlas_size=64, device=0)
    for ctx in (dev, host):
        ctx.set_atlas_keep(keep)
    assert put_case(dev, memory, 1, small) == host.put_image(1, VC.texels(small))
    assert put_case(dev, memory, 2, case) == host.put_image(2, VC.texels(case))
    assert dev.atlas_size() == host.atlas_size() > 64
    assert dev.has_image(1) == host.has_image(1) == keep and dev.has_image(2)
    same_atlases(dev, host, f"keep {keep}")
    dev.close(), host.close()


def test_retained_scene_is_recorded_again_after_an_update(memory):
    from figdraw_amd.context import HipContext
    from figdraw_amd.scene import Fig, FigKind, Glyph, Renders, rect, rgba

    rng = np.random.default_rng(16)
    first = ("retained first", REF.BGRA8, 0, 0, 0, VC.noise_bgra(rng, 24, 30), None, "tight")
    img = np.zeros((30, 24, 4), np.uint8)
    img[10:20, 8:12] = (200, 200, 200, 255)  # other ink boxes than the noise has
    second = ("retained second", REF.BGRA8, 0, 0, 0, img, None, "padded")
    frames = []
    for path in ("device", "host"):
        ctx = HipContext(atlas_size=256, device=0)
        if path == "device":
            put_case(ctx, memory, 7, first)
        else:
            ctx.put_image(7, VC.texels(first))
        r = Renders()
        r.addRoot(0, Fig(kind=FigKind.nkRectangle, screenBox=rect(0, 0, 256, 128), fill=rgba(240, 240, 240, 255)))
        r.addRoot(0, Fig(kind=FigKind.nkText, screenBox=rect(20, 30, 200, 40), glyphs=[Glyph(image_id=7, x=10.3 + 29.37 * i, y=2.0, subpixel_shift=-1.0) for i in range(4)]))
        ctx.scene_retain(r, 256, 128)
        ctx.scene_render()
        assert ctx.scene_stats()[0] == 0  # nothing moved: no root is walked again
        before = ctx.read_pixels()
        if path == "device":
            put_case(ctx, memory, 7, second, update=True)
        else:
            ctx.update_image(7, VC.texels(second))
        ctx.scene_render()
        assert ctx.scene_stats()[0] > 0  # the epoch moved: the text root was recorded again
        frames.append((before, ctx.read_pixels(), ctx.record_digest()))
        ctx.close()
    assert not np.array_equal(frames[0][0], frames[0][1])
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1]) and frames[0][2] == frames[1][2]


# ------------------------------------------------------------------------------------------------------------------ sources of other kinds
def test_page_locked_host_memory_is_a_source(memory):
    from figdraw_amd.context import HipContext

    case = nv12(np.random.default_rng(17), 70, 45, flags=REF.CHROMA_LINEAR, name="pinned", matrix=REF.BT2020)
    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    assert put_case(dev, memory, 1, case, place=lambda data, align: memory.page_locked(data)) == host.put_image(1, VC.texels(case))
    same_atlases(dev, host, "page-locked")
    dev.close(), host.close()


def test_a_decoder_surface_in_one_torch_allocation():
    """luma and chroma as two views of one torch tensor on the device, chroma at pitch * height: tests/video_frame_tensor_child.py, in a
    process of its own -- torch brings its own copies of the ROCm libraries, and this process has loaded the system's"""
    import subprocess
    import sys

    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "video_frame_tensor_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "video_frame_tensor_child: OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------------------------ refusals on a device context
def test_pageable_host_memory_is_refused_for_either_plane(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    luma, chroma = np.zeros((9, 16), np.uint8), np.zeros((5, 8, 2), np.uint8)
    good_y, good_uv = memory.upload(luma.tobytes()), memory.upload(chroma.tobytes())
    assert ctx.put_video_frame(1, good_y, good_uv, 16, 9, 16, 16)[2:] == (16, 9)
    before = ctx.atlas_usage()
    for y_ptr, uv_ptr in ((luma.ctypes.data, good_uv), (good_y, chroma.ctypes.data)):
        for call in (lambda: ctx.put_video_frame(2, y_ptr, uv_ptr, 16, 9, 16, 16), lambda: ctx.update_video_frame(1, y_ptr, uv_ptr, 16, 9, 16, 16)):
            with pytest.raises(FigdrawHipError) as e:
                call()
            assert e.value.code == -1 and "neither device memory of the context's device nor page-locked host memory" in str(e.value)
            assert ctx.atlas_usage() == before and not ctx.has_image(2)
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    assert ctx.put_video_frame(2, good_y, good_uv, 16, 9, 16, 16)[2:] == (16, 9)  # and the context works on
    ctx.close()


def test_a_plane_on_another_device_is_refused(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    n = C.c_int()
    assert memory.hip.hipGetDeviceCount(C.byref(n)) == 0
    if n.value < 2:
        pytest.skip("one device")
    ctx = HipContext(atlas_size=256, device=0)
    assert memory.hip.hipSetDevice(1) == 0
    other = memory.device(16 * 9)
    assert memory.hip.hipSetDevice(0) == 0
    here = memory.device(16 * 9)
    before = ctx.atlas_usage()
    for y_ptr, uv_ptr in ((other, here), (here, other)):
        with pytest.raises(FigdrawHipError) as e:
            ctx.put_video_frame(2, y_ptr, uv_ptr, 16, 9, 16, 16)
        assert e.value.code == -1 and "neither device memory of the context's device" in str(e.value) and ctx.atlas_usage() == before
    ctx.close()
