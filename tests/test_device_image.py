"""Images from device memory on the device (fdh_put_image_device, fdh_update_image_device; k_image_import, k_image_import_tail): a context
that gets its images from device memory against a second one that gets, through fdh_put_image / fdh_update_image, the bytes the reference
tests/device_image_ref.py makes of the same sources.  The bar is identity: rectangles, usage, every level of both atlases byte for byte, the
draw records; rendered frames also against the oracle within the suite's bar of 1 LSB on at most 0.5 % of the pixels."""
import ctypes as C
import os

import numpy as np
import pytest

import device_image_cases as DC
import device_image_ref as REF

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


def put_case(ctx, memory, key, case, update=False):
    w, h = DC.size_of(case)
    buf, align, pitch, plane, channels = DC.pack(case)
    ptr = memory.upload(buf, align)
    call = ctx.update_image_device if update else ctx.put_image_device
    return call(key, ptr, w, h, pitch, format=case[1], channels=channels, plane_bytes=plane, straight_alpha=bool(case[2] & 1))


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

    cases = DC.cases(large=True)
    dev, host, orc = HipContext(atlas_size=2048, device=0), HipContext(atlas_size=2048, device=0), O.Oracle(atlas_size=2048, threads=8)
    rects = []
    for i, case in enumerate(cases):
        texels = DC.texels(case)
        r = put_case(dev, memory, 100 + i, case)
        assert r == host.put_image(100 + i, texels) == tuple(orc.put_image(100 + i, texels)), case[0]
        assert r[2:] == DC.size_of(case)
        rects.append(r)
    assert dev.atlas_size() == 2048
    yield cases, dev, host, orc, rects
    dev.close(), host.close()


def test_rectangles_usage_and_every_level(both):
    cases, dev, host, orc, rects = both
    assert len(cases) > 50
    same_atlases(dev, host, "all cases")
    level0 = dev.read_atlas_level(0)
    for case, (x, y, w, h) in zip(cases, rects):  # and level 0 is the reference's conversion (nothing of a line)
        want = DC.texels(case) if w > 1 and h > 1 else np.zeros((h, w, 4), np.uint8)
        assert np.array_equal(level0[y:y + h, x:x + w], want), case[0]


def _frame(ctx, cases, rects):
    """every image up to 128 x 128 at 1:1 and magnified 2.5 times (the draws shrink to the ink boxes), a few larger ones minified"""
    W, H = 2000, 1500
    ctx.begin_frame(W, H, True, (0.1, 0.2, 0.3, 1.0))
    x, y, row = 4.0, 4.0, 0.0
    n = 0
    for i, (case, r) in enumerate(zip(cases, rects)):
        w, h = r[2:]
        if w > 128 or h > 128:
            scales = (0.25,) if w <= 300 else (0.125,)
        else:
            scales = (1.0, 2.5)
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
    assert n > 100
    assert dev.record_digest() == host.record_digest()
    got = dev.read_pixels()
    assert np.array_equal(got, host.read_pixels())
    against_oracle(got, orc.read_pixels(), "all cases")


def test_ink_boxes_shrink_the_draws():
    """an image whose ink is one texel: the draw record is the host path's, and not that of the same image with ink everywhere"""
    from figdraw_amd.context import HipContext

    mem = Memory()
    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    corner = np.zeros((100, 100, 4), np.uint8)
    corner[99, 0] = (9, 9, 9, 255)
    full = np.full((100, 100, 4), 255, np.uint8)
    digests = []
    for img in (corner, full):
        for ctx in (dev, host):
            ctx.reset_atlas(0)
        assert dev.put_image_device(1, mem.upload(img.tobytes()), 100, 100, 400) == host.put_image(1, img)
        for ctx in (dev, host):
            ctx.begin_frame(400, 300, True, (0, 0, 0, 1))
            ctx.draw_image(1, (10.0, 20.0), WHITE, (250.0, 250.0))
            ctx.end_frame()
        assert np.array_equal(dev.read_pixels(), host.read_pixels())
        digests.append((dev.record_digest(), host.record_digest()))
    assert digests[0][0] == digests[0][1] and digests[1][0] == digests[1][1] and digests[0][0] != digests[1][0]
    dev.close(), host.close(), mem.free()


def test_source_beyond_the_tail(memory):
    """2100 x 40 in an atlas of 4096: the level-5 image is 66 texels wide and takes a k_minify2 step before the tail's workgroup holds it"""
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(4)
    case = ("noise 2100 x 40", REF.RGBA8, 1, DC.noise_rgba(rng, 2100, 40), "tight")
    dev, host = HipContext(atlas_size=4096, device=0), HipContext(atlas_size=4096, device=0)
    assert put_case(dev, memory, 1, case) == host.put_image(1, DC.texels(case))
    same_atlases(dev, host, case[0])
    assert dev.read_atlas_level(5).any()
    dev.close(), host.close()


# ------------------------------------------------------------------------------------------------------------------ neighbours
def test_neighbours_share_a_column_of_level_6(memory):
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(11)
    imgs = [("a", REF.RGBA8, 0, DC.noise_rgba(rng, 100, 100), "tight"), ("b", REF.PLANAR_F32, 1, DC.float_planes(rng, np.float32, 4, 100, 100), "pitch 4"),
            ("a again", REF.PLANAR_F16, 0, DC.float_planes(rng, np.float16, 3, 100, 100), "data + 4")]
    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    assert put_case(dev, memory, 1, imgs[0]) == host.put_image(1, DC.texels(imgs[0])) == (4, 4, 100, 100)
    assert put_case(dev, memory, 2, imgs[1]) == host.put_image(2, DC.texels(imgs[1])) == (112, 4, 100, 100)  # level 6: columns 0 .. 1 and 1 .. 3
    same_atlases(dev, host, "two puts")
    put_case(dev, memory, 1, imgs[2], update=True)  # the first after the second: it takes the shared column back
    host.update_image(1, DC.texels(imgs[2]))
    same_atlases(dev, host, "the first updated")
    dev.close(), host.close()


def test_entries_against_the_right_and_bottom_edges(memory):
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(12)
    dev, host = HipContext(atlas_size=128, device=0), HipContext(atlas_size=128, device=0)
    for key, (w, h) in enumerate(((119, 60), (119, 44)), start=1):
        case = (f"edge {key}", REF.RGBA8, 0, DC.noise_rgba(rng, w, h), "pitch 16")
        r = put_case(dev, memory, key, case)
        assert r == host.put_image(key, DC.texels(case)) and r[0] + r[2] == 123
    assert r[1] + r[3] == 124 and dev.atlas_size() == 128
    same_atlases(dev, host, "edges")
    dev.close(), host.close()


# ------------------------------------------------------------------------------------------------------------------ life cycle
def test_update_of_a_flippy_entry(memory):
    from conftest import GOLDEN
    from figdraw_amd.context import HipContext

    data = open(os.path.join(GOLDEN, "img1.flippy"), "rb").read()
    case = ("update", REF.PLANAR_F32, 1, DC.float_planes(np.random.default_rng(13), np.float32, 4, 100, 100), "sub-rectangle")
    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    assert dev.put_flippy(1, data) == host.put_flippy(1, data) == (4, 4, 100, 100)
    put_case(dev, memory, 1, case, update=True)
    host.update_image(1, DC.texels(case))
    same_atlases(dev, host, "updated")
    assert dev.compact_atlas(512)["rects_moved"] == host.compact_atlas(512)["rects_moved"]  # a chain entry now: the move makes its levels again
    same_atlases(dev, host, "compacted")
    dev.close(), host.close()


@pytest.mark.parametrize("keep", [False, True])
def test_put_that_grows_the_atlas(memory, keep):
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(14)
    small = DC.noise_rgba(rng, 20, 20)
    case = ("grows", REF.RGBA8, 1, DC.noise_rgba(rng, 100, 70), "data + 4")
    dev, host = HipContext(atlas_size=64, device=0), HipContext(atlas_size=64, device=0)
    for ctx in (dev, host):
        ctx.set_atlas_keep(keep)
    assert dev.put_image_device(1, memory.upload(small.tobytes()), 20, 20, 80) == host.put_image(1, small)
    assert put_case(dev, memory, 2, case) == host.put_image(2, DC.texels(case))
    assert dev.atlas_size() == host.atlas_size() > 64
    assert dev.has_image(1) == host.has_image(1) == keep and dev.has_image(2)
    same_atlases(dev, host, f"keep {keep}")
    dev.close(), host.close()


def test_compaction_and_distance_field_of_a_device_put_entry(memory):
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(15)
    cases = [("c0", REF.RGBA8, 0, DC.noise_rgba(rng, 40, 30), "tight"), ("c1", REF.PLANAR_F16, 1, DC.float_planes(rng, np.float16, 4, 61, 35), "pitch 16"),
             ("c2", REF.PLANAR_F32, 0, DC.float_planes(rng, np.float32, 1, 90, 33), "tight")]
    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    for key, case in enumerate(cases, start=1):
        assert put_case(dev, memory, key, case) == host.put_image(key, DC.texels(case))
    dev.remove_image(1), host.remove_image(1)
    assert dev.put_image_sdf_of(2, 9, channel=3, pad=3, sdf_range=6) == host.put_image_sdf_of(2, 9, channel=3, pad=3, sdf_range=6)
    same_atlases(dev, host, "a field of a device-put entry")
    a, b = dev.compact_atlas(), host.compact_atlas()
    assert (a["entries"], a["rects_moved"], a["texels"]) == (b["entries"], b["rects_moved"], b["texels"]) and a["entries"] == 3
    assert [dev.image_rect(k) for k in (2, 3, 9)] == [host.image_rect(k) for k in (2, 3, 9)]
    same_atlases(dev, host, "compacted")
    dev.close(), host.close()


def test_retained_scene_is_recorded_again_after_a_device_update(memory):
    from figdraw_amd.context import HipContext
    from figdraw_amd.scene import Fig, FigKind, Glyph, Renders, rect, rgba

    rng = np.random.default_rng(16)
    first = ("first", REF.RGBA8, 0, DC.noise_rgba(rng, 24, 30), "tight")
    second = np.zeros((30, 24, 4), np.uint8)
    second[10:20, 8:12] = (200, 200, 200, 255)  # other ink boxes than the noise has
    frames = []
    for path in ("device", "host"):
        ctx = HipContext(atlas_size=256, device=0)
        if path == "device":
            put_case(ctx, memory, 7, first)
        else:
            ctx.put_image(7, DC.texels(first))
        r = Renders()
        r.addRoot(0, Fig(kind=FigKind.nkRectangle, screenBox=rect(0, 0, 256, 128), fill=rgba(240, 240, 240, 255)))
        r.addRoot(0, Fig(kind=FigKind.nkText, screenBox=rect(20, 30, 200, 40), glyphs=[Glyph(image_id=7, x=10.3 + 29.37 * i, y=2.0, subpixel_shift=-1.0) for i in range(4)]))
        ctx.scene_retain(r, 256, 128)
        ctx.scene_render()
        assert ctx.scene_stats()[0] == 0  # nothing moved: no root is walked again
        before = ctx.read_pixels()
        if path == "device":
            ctx.update_image_device(7, memory.upload(second.tobytes()), 24, 30, 96)
        else:
            ctx.update_image(7, second)
        ctx.scene_render()
        assert ctx.scene_stats()[0] > 0  # the epoch moved: the text root was recorded again
        frames.append((before, ctx.read_pixels(), ctx.record_digest()))
        ctx.close()
    assert not np.array_equal(frames[0][0], frames[0][1])
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1]) and frames[0][2] == frames[1][2]


# ------------------------------------------------------------------------------------------------------------------ sources of other kinds
def test_a_frame_as_a_source():
    """context A's frame surface (fdh_frame_device_ptr), a region of it, goes into context B's atlas; B draws it.  Against B given
    fdh_read_pixels of the same region through fdh_put_image; and a context's own frame into its own atlas."""
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    a, b, host, orc = HipContext(device=0), HipContext(atlas_size=512, device=0), HipContext(atlas_size=512, device=0), O.Oracle(atlas_size=512, threads=4)
    a.begin_frame(320, 200, True, (0.9, 0.5, 0.1, 1.0))
    for i in range(12):
        a.draw_rounded_rect_sdf((10.0 + 24 * i, 12.0 + 9 * i, 60.0, 40.0), [(20 * i, 255 - 20 * i, 90, 255 - 15 * i), (255, 20 * i, 0, 255), (0, 90, 255 - 20 * i, 200), (255, 255, 255, 255)], (8.0,) * 4, (8.0,) * 4, 3)
    a.end_frame()
    ptr, w, h, pitch = a.frame_device_ptr()
    a.sync()
    x0, y0, rw, rh = 37, 21, 151, 90
    region = a.read_pixels(x0, y0, rw, rh)
    assert len(np.unique(region.reshape(-1, 4), axis=0)) > 50
    r = b.put_image_device(5, ptr + y0 * pitch + x0 * 4, rw, rh, pitch)
    assert r == host.put_image(5, region) == tuple(orc.put_image(5, region))
    same_atlases(b, host, "a frame region")
    for ctx in (b, host, orc):
        ctx.begin_frame(400, 260, True, (1.0, 1.0, 1.0, 1.0))
        ctx.draw_image(5, (8.0, 6.0), WHITE)
        ctx.draw_image(5, (170.0, 100.0), [(255, 200, 200, 200)] * 4, (rw * 1.4, rh * 1.4))
        ctx.end_frame()
    got = b.read_pixels()
    assert np.array_equal(got, host.read_pixels()) and b.record_digest() == host.record_digest()
    against_oracle(got, orc.read_pixels(), "a frame as a cached layer")
    # the frame B has just rendered, into B's own atlas
    ptr, w, h, pitch = b.frame_device_ptr()
    b.sync()
    assert b.put_image_device(6, ptr, w, h, pitch) == host.put_image(6, got)
    same_atlases(b, host, "the context's own frame")
    a.close(), b.close(), host.close()


def test_page_locked_host_memory_is_a_source(memory):
    from figdraw_amd.context import HipContext

    case = ("pinned", REF.PLANAR_F16, 1, DC.float_planes(np.random.default_rng(17), np.float16, 4, 70, 45), "tight")
    buf, align, pitch, plane, channels = DC.pack(case)
    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    r = dev.put_image_device(1, memory.page_locked(buf), 70, 45, pitch, format=case[1], channels=channels, plane_bytes=plane, straight_alpha=True)
    assert r == host.put_image(1, DC.texels(case))
    same_atlases(dev, host, "page-locked")
    dev.close(), host.close()


def test_a_tensor():
    """torch tensors on the device through put_image_tensor / update_image_tensor against the host path: tests/device_image_tensor_child.py,
    in a process of its own -- torch brings its own copies of the ROCm libraries, and this process has loaded the system's"""
    import subprocess
    import sys

    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_image_tensor_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device_image_tensor_child: OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------------------------ refusals on a device context
def test_pageable_host_memory_is_refused(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    img = np.zeros((9, 16, 4), np.uint8)
    assert ctx.put_image(1, img)[2:] == (16, 9)
    before = ctx.atlas_usage()
    for call in (lambda: ctx.put_image_device(2, img.ctypes.data, 16, 9, 64), lambda: ctx.update_image_device(1, img.ctypes.data, 16, 9, 64)):
        with pytest.raises(FigdrawHipError) as e:
            call()
        assert e.value.code == -1 and "neither device memory of the context's device nor page-locked host memory" in str(e.value)
        assert ctx.atlas_usage() == before and not ctx.has_image(2)
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    assert ctx.put_image_device(2, memory.upload(img.tobytes()), 16, 9, 64)[2:] == (16, 9)  # and the context works on
    ctx.close()


def test_memory_of_another_device_is_refused(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    n = C.c_int()
    assert memory.hip.hipGetDeviceCount(C.byref(n)) == 0
    if n.value < 2:
        pytest.skip("one device")
    ctx = HipContext(atlas_size=256, device=0)
    assert memory.hip.hipSetDevice(1) == 0
    other = memory.device(16 * 9 * 4)
    assert memory.hip.hipSetDevice(0) == 0
    before = ctx.atlas_usage()
    with pytest.raises(FigdrawHipError) as e:
        ctx.put_image_device(2, other, 16, 9, 64)
    assert e.value.code == -1 and "neither device memory of the context's device" in str(e.value) and ctx.atlas_usage() == before
    ctx.close()
