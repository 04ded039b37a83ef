"""Batches of images from device memory on the device (fdh_put_images_device, fdh_update_images_device; k_image_import_batch,
k_image_import_tail_batch): two contexts per case, one filled by the batch, one by single calls of the same sources in the same order.  The
bar is identity: rectangles, usage, every level of both atlases byte for byte, and the draw records of a frame that draws every image once,
which holds the ink boxes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import device_image_cases as DC
import device_image_ref as REF
from test_device_image import WHITE, Memory, same_atlases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def memory():
    m = Memory()
    yield m
    m.free()


def uploaded(memory, key, case, pinned=False):
    """-> an item of put_images_device: the case's source in device (page-locked) memory"""
    w, h = DC.size_of(case)
    buf, align, pitch, plane, channels = DC.pack(case)
    ptr = memory.page_locked(buf) if pinned else memory.upload(buf, align)
    return (key, ptr, w, h, pitch, case[1], channels, plane, bool(case[2] & 1))


def thin_floats(rng, dtype, channels, w, h):
    """planes of an image 1 texel wide or high (too few elements for DC.float_planes): seeded values with hostile ones among them"""
    v = rng.uniform(-0.2, 1.2, size=(channels, h, w)).astype(dtype)
    hostile = np.array([np.nan, np.inf, -np.inf, -0.0, 0.5, 1.5 / 255.0, 2.0, -1.0], dtype)
    v.reshape(-1)[np.arange(len(hostile)) * 4 + 1] = hostile
    return v


def single_put(ctx, it, update=False):
    key, ptr, w, h, pitch, fmt, channels, plane, straight = it
    call = ctx.update_image_device if update else ctx.put_image_device
    return call(key, ptr, w, h, pitch, format=fmt, channels=channels, plane_bytes=plane, straight_alpha=straight)


def digest_of_a_frame(ctx, items, rects):
    """every image that is still in the atlas drawn once, magnified 1.5 times -> the digest of the draw records"""
    W, H = 2000, 1600
    ctx.begin_frame(W, H, True, (0.1, 0.2, 0.3, 1.0))
    x, y, row = 4.0, 4.0, 0.0
    for i, (it, r) in enumerate(zip(items, rects)):
        if not ctx.has_image(it[0]):
            continue
        s = 1.5 if max(r[2:]) <= 128 else 0.25
        w, h = r[2] * s, r[3] * s
        if x + w > W - 4:
            x, y, row = 4.0, y + row + 3.0, 0.0
        ctx.draw_image(it[0], (x + 0.25 * (i % 3), y), WHITE, (w, h))
        x, row = x + w + 3.0, max(row, h)
    assert y + row < H
    ctx.end_frame()
    return ctx.record_digest()


def both_ways(items, atlas_size=256, keep=False, what=""):
    """the items as one batch and as single calls -> (the batch's context, the single calls' context, the rectangles)"""
    from figdraw_amd.context import HipContext

    batch, single = HipContext(atlas_size=atlas_size, device=0), HipContext(atlas_size=atlas_size, device=0)
    for ctx in (batch, single):
        ctx.set_atlas_keep(keep)
    rects = batch.put_images_device(items)
    if keep and batch.atlas_size() != atlas_size:
        # (include_glyphs/figdraw_hip_atlas.h: a batch in keep mode makes room once, before its first image, and equals single calls from there on)
        single.compact_atlas(batch.atlas_size())
    assert rects == [single_put(single, it) for it in items], what
    same_atlases(batch, single, what)
    assert [batch.has_image(it[0]) for it in items] == [single.has_image(it[0]) for it in items]
    assert digest_of_a_frame(batch, items, rects) == digest_of_a_frame(single, items, rects), what
    assert np.array_equal(batch.read_pixels(), single.read_pixels()), what
    return batch, single, rects


# ------------------------------------------------------------------------------------------------------------------ identity with single calls
@pytest.fixture(scope="module")
def mixed(memory):
    """all of cases(large=False): the three formats, every layout, straight alpha; the sources are uploaded once"""
    cases = DC.cases(large=False)
    return cases, [uploaded(memory, 100 + i, c) for i, c in enumerate(cases)]


@pytest.mark.parametrize("order", ["given", "reversed"])
def test_the_mixed_batch(mixed, order):
    cases, items = mixed
    items = items if order == "given" else items[::-1]
    batch, single, rects = both_ways(items, atlas_size=2048, what=f"the mixed batch, {order}")
    assert len(items) > 50 and batch.atlas_size() == 2048
    st = batch.image_batch_stats()
    assert (st["images"], st["written"], st["dropped_by_growth"], st["launches"]) == (len(items), len(items), 0, 4)
    level0 = batch.read_atlas_level(0)
    for it, (x, y, w, h) in zip(items, rects):  # and level 0 is the reference's conversion (nothing of a line)
        want = DC.texels(cases[it[0] - 100]) if w > 1 and h > 1 else np.zeros((h, w, 4), np.uint8)
        assert np.array_equal(level0[y:y + h, x:x + w], want), cases[it[0] - 100][0]
    batch.close(), single.close()


def test_a_batch_of_one(mixed):
    cases, items = mixed
    it = next(i for i, c in zip(items, cases) if c[0] == "float16 33 x 31 pitch 4")
    batch, single, _ = both_ways([it], what="one")
    assert batch.image_batch_stats()["launches"] == 1
    batch.close(), single.close()


def test_lines_alone_store_nothing_and_launch_nothing(mixed, memory):
    cases, items = mixed
    lines = [i for i, c in zip(items, cases) if c[0] in ("noise 1 x 1", "noise 1 x 40", "noise 40 x 1")]
    assert len(lines) == 3
    rng = np.random.default_rng(25)  # and planar ones: the host converts a line's elements itself
    lines.append(uploaded(memory, 1, ("half line", REF.PLANAR_F16, 1, thin_floats(rng, np.float16, 4, 40, 1), "pitch 16")))
    lines.append(uploaded(memory, 2, ("float column", REF.PLANAR_F32, 0, thin_floats(rng, np.float32, 3, 1, 40), "sub-rectangle")))
    lines.append(uploaded(memory, 3, ("one plane", REF.PLANAR_F32, 1, thin_floats(rng, np.float32, 1, 1, 40), "pitch 4")))
    batch, single, _ = both_ways(lines, what="lines")
    st = batch.image_batch_stats()
    assert (st["written"], st["tiles"], st["launches"]) == (6, 0, 0)
    assert not batch.read_atlas_level(0).any()
    batch.close(), single.close()


def pair(memory):
    rng = np.random.default_rng(11)
    a = ("a", REF.RGBA8, 0, DC.noise_rgba(rng, 100, 100), "tight")
    b = ("b", REF.PLANAR_F32, 1, DC.float_planes(rng, np.float32, 4, 100, 100), "pitch 4")
    return uploaded(memory, 1, a), uploaded(memory, 2, b)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_the_level_6_pair(memory, order):
    two = pair(memory)
    batch, single, rects = both_ways([two[k] for k in order], what=f"the pair {order}")
    assert rects == [(4, 4, 100, 100), (112, 4, 100, 100)]  # level 6: columns 0 .. 1 and 1 .. 2
    assert batch.image_batch_stats()["launches"] == 3  # two formats, and the tails
    batch.close(), single.close()


def test_images_against_the_right_and_bottom_edges(memory):
    rng = np.random.default_rng(12)
    items = [uploaded(memory, k, (f"edge {k}", REF.RGBA8, k & 1, DC.noise_rgba(rng, 247, (120, 112)[k - 1]), "pitch 16")) for k in (1, 2)]
    batch, single, rects = both_ways(items, what="edges")
    assert batch.atlas_size() == 256 and rects[1][0] + rects[1][2] == 251 and rects[1][1] + rects[1][3] == 252
    batch.close(), single.close()


@pytest.mark.parametrize("keep", [False, True])
def test_growth_in_the_middle_of_a_batch(memory, keep):
    rng = np.random.default_rng(14)
    sizes = [(100, 100), (100, 100), (60, 60), (120, 120), (90, 40), (33, 31)]
    items = [uploaded(memory, k, (f"g{k}", (REF.RGBA8, REF.PLANAR_F16)[k & 1], 1, DC.noise_rgba(rng, w, h) if not k & 1 else DC.float_planes(rng, np.float16, 4, w, h), "tight"))
             for k, (w, h) in enumerate(sizes, start=1)]
    batch, single, _ = both_ways(items, keep=keep, what=f"growth, keep {keep}")
    assert batch.atlas_size() == 512
    st = batch.image_batch_stats()
    alive = [batch.has_image(k) for k in range(1, 7)]
    assert st["dropped_by_growth"] == alive.count(False) and st["written"] == alive.count(True)
    assert (st["dropped_by_growth"] == 0) == keep
    batch.close(), single.close()


def test_sources_in_page_locked_host_memory(memory):
    rng = np.random.default_rng(17)
    cases = [("pinned half", REF.PLANAR_F16, 1, DC.float_planes(rng, np.float16, 4, 70, 45), "tight"), ("pinned bytes", REF.RGBA8, 0, DC.noise_rgba(rng, 33, 31), "pitch 4"),
             ("pinned line", REF.PLANAR_F32, 1, thin_floats(rng, np.float32, 4, 1, 40), "pitch 16")]
    items = [uploaded(memory, k, c, pinned=True) for k, c in enumerate(cases, start=1)]
    batch, single, _ = both_ways(items, what="page-locked")
    batch.close(), single.close()


def test_a_rendered_frame_as_one_of_the_sources(memory):
    from figdraw_amd.context import HipContext

    a = HipContext(device=0)
    a.begin_frame(320, 200, True, (0.9, 0.5, 0.1, 1.0))
    for i in range(12):
        a.draw_rounded_rect_sdf((10.0 + 24 * i, 12.0 + 9 * i, 60.0, 40.0), [(20 * i, 255 - 20 * i, 90, 255 - 15 * i), (255, 20 * i, 0, 255), (0, 90, 255 - 20 * i, 200), (255, 255, 255, 255)], (8.0,) * 4, (8.0,) * 4, 3)
    a.end_frame()
    ptr, w, h, pitch = a.frame_device_ptr()
    a.sync()
    x0, y0, rw, rh = 37, 21, 151, 90
    rng = np.random.default_rng(18)
    items = [uploaded(memory, 1, ("before", REF.PLANAR_F32, 0, DC.float_planes(rng, np.float32, 1, 40, 40), "tight")), (5, ptr + y0 * pitch + x0 * 4, rw, rh, pitch, REF.RGBA8, 4, 0, False),
             uploaded(memory, 2, ("after", REF.RGBA8, 1, DC.noise_rgba(rng, 50, 20), "tight"))]
    batch, single, rects = both_ways(items, atlas_size=512, what="a frame region")
    x, y = rects[1][:2]
    assert np.array_equal(batch.read_atlas_level(0)[y:y + rh, x:x + rw], a.read_pixels(x0, y0, rw, rh))
    a.close(), batch.close(), single.close()


# ------------------------------------------------------------------------------------------------------------------ updates
def test_an_update_batch_of_a_permuted_subset(memory):
    """put everything, then new texels in another format for a permuted subset that holds both images of the level-6 pair; a retained scene
    is recorded again afterwards, as after a single update"""
    from figdraw_amd.context import HipContext
    from figdraw_amd.scene import Fig, FigKind, Glyph, Renders, rect, rgba

    rng = np.random.default_rng(21)
    two = pair(memory)
    sizes = [(24, 30), (65, 65), (33, 31), (1, 40), (129, 127)]
    first = list(two) + [uploaded(memory, 3 + k, (f"p{k}", REF.RGBA8, k & 1, DC.noise_rgba(rng, w, h), "tight")) for k, (w, h) in enumerate(sizes)]
    new_sizes = {1: (100, 100), 2: (100, 100), 3: (24, 30), 5: (33, 31), 6: (1, 40), 7: (129, 127)}
    planes = lambda k, w, h: (thin_floats if w == 1 else DC.float_planes)(rng, np.float16 if k & 1 else np.float32, (4, 3, 1)[k % 3], w, h)  # noqa: E731
    fresh = {k: uploaded(memory, k, (f"u{k}", REF.PLANAR_F16 if k & 1 else REF.PLANAR_F32, ~k & 1, planes(k, w, h), DC.LAYOUTS[k % 5])) for k, (w, h) in new_sizes.items()}
    order = [5, 2, 7, 1, 6, 3]
    batch, single = HipContext(atlas_size=512, device=0), HipContext(atlas_size=512, device=0)
    rects = batch.put_images_device(first)
    assert rects == [single_put(single, it) for it in first] and rects[:2] == [(4, 4, 100, 100), (112, 4, 100, 100)]
    scenes = []
    for ctx in (batch, single):
        r = Renders()
        r.addRoot(0, Fig(kind=FigKind.nkRectangle, screenBox=rect(0, 0, 256, 128), fill=rgba(240, 240, 240, 255)))
        r.addRoot(0, Fig(kind=FigKind.nkText, screenBox=rect(20, 30, 200, 40), glyphs=[Glyph(image_id=3, x=10.3 + 29.37 * i, y=2.0, subpixel_shift=-1.0) for i in range(4)]))
        ctx.scene_retain(r, 256, 128)
        ctx.scene_render()
        assert ctx.scene_stats()[0] == 0  # nothing moved: no root is walked again
        scenes.append(ctx.read_pixels())
    epoch = batch.atlas_usage()["epoch"]
    batch.update_images_device([fresh[k] for k in order])
    for k in order:
        single_put(single, fresh[k], update=True)
    assert batch.atlas_usage()["epoch"] == epoch + len(order)
    same_atlases(batch, single, "updated")
    st = batch.image_batch_stats()
    assert (st["images"], st["written"], st["launches"]) == (6, 6, 3)
    for ctx in (batch, single):
        ctx.scene_render()
        assert ctx.scene_stats()[0] > 0  # the epoch moved: the text root was recorded again
    assert batch.record_digest() == single.record_digest() and np.array_equal(batch.read_pixels(), single.read_pixels())
    assert not np.array_equal(batch.read_pixels(), scenes[0])
    assert digest_of_a_frame(batch, first, rects) == digest_of_a_frame(single, first, rects)
    batch.close(), single.close()


# ------------------------------------------------------------------------------------------------------------------ launch counts
def test_launches_do_not_depend_on_the_number_of_images(memory):
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(22)
    kinds = [lambda w, h: ("b", REF.RGBA8, 0, DC.noise_rgba(rng, w, h), "tight"), lambda w, h: ("f", REF.PLANAR_F32, 1, DC.float_planes(rng, np.float32, 3, w, h), "tight"),
             lambda w, h: ("h", REF.PLANAR_F16, 0, DC.float_planes(rng, np.float16, 1, w, h), "tight")]
    sources = [uploaded(memory, 0, kinds[k](70 + k, 65)) for k in range(3)]  # (three sources: an image's key is its item's alone)
    ctx = HipContext(atlas_size=2048, device=0)
    counts = []
    for n in (3, 60):
        ctx.reset_atlas(0)
        ctx.put_images_device([(k + 1,) + sources[k % 3][1:] for k in range(n)])
        st = ctx.image_batch_stats()
        assert st["written"] == n
        counts.append(st["launches"])
    assert counts[0] == counts[1] == 4
    ctx.reset_atlas(0)
    small = uploaded(memory, 0, kinds[2](32, 32))
    ctx.put_images_device([(k + 1,) + small[1:] for k in range(20)])
    assert ctx.image_batch_stats()["launches"] == 1 and ctx.image_batch_stats()["tiles"] == 20
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ refusals on the device
def test_a_refused_batch_changes_nothing(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext
    from test_device_image import levels_of

    rng = np.random.default_rng(23)
    items = [uploaded(memory, k, (f"r{k}", REF.RGBA8, 0, DC.noise_rgba(rng, 40, 30), "tight")) for k in (1, 2, 3)]
    ctx = HipContext(atlas_size=256, device=0)
    rects = ctx.put_images_device(items)
    before = (ctx.atlas_usage(), levels_of(ctx), digest_of_a_frame(ctx, items, rects), ctx.image_batch_stats())
    pageable = np.zeros((30, 40, 4), np.uint8)
    hostile = [
        ([(7,) + items[0][1:], (8,) + items[1][1:], (9, pageable.ctypes.data, 40, 30, 160)], "neither device memory of the context's device nor page-locked host memory"),
        ([(7,) + items[0][1:], (8,) + items[1][1:], (7,) + items[2][1:]], "a key occurs twice"),
    ]
    for update in (False, True):
        for bad, text in hostile:
            if update:
                bad = [(k,) + it[1:] for k, it in zip((1, 2, 1 if "twice" in text else 3), bad)]
            with pytest.raises(FigdrawHipError) as e:
                (ctx.update_images_device if update else ctx.put_images_device)(bad)
            assert e.value.code == -1 and text in str(e.value)
            after = (ctx.atlas_usage(), levels_of(ctx), digest_of_a_frame(ctx, items, rects), ctx.image_batch_stats())
            assert after[0] == before[0] and after[2:] == before[2:] and all(np.array_equal(x, y) for x, y in zip(after[1], before[1])), (update, text)
            assert not any(ctx.has_image(k) for k in (7, 8, 9))
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    assert ctx.put_images_device([(7,) + items[0][1:]])[0][2:] == (40, 30)  # and the context works on
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ other users of the atlas
def test_other_users_of_the_atlas(memory):
    rng = np.random.default_rng(24)
    cases = [("c0", REF.RGBA8, 0, DC.noise_rgba(rng, 40, 30), "tight"), ("c1", REF.PLANAR_F16, 1, DC.float_planes(rng, np.float16, 4, 61, 35), "pitch 16"),
             ("c2", REF.PLANAR_F32, 0, DC.float_planes(rng, np.float32, 1, 90, 33), "tight")]
    items = [uploaded(memory, k, c) for k, c in enumerate(cases, start=1)]
    from figdraw_amd.context import HipContext

    batch, single = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    old = DC.noise_rgba(rng, 50, 50)
    frames = []
    for ctx in (batch, single):
        ctx.put_image(40, old)
        ctx.begin_frame(200, 120, True, (0.2, 0.2, 0.2, 1.0))
        ctx.draw_image(40, (10.0, 8.0), WHITE, (125.0, 100.0))
        ctx.end_frame()
        frames.append(ctx.read_pixels())
    assert batch.put_images_device(items) == [single_put(single, it) for it in items]
    for ctx, frame in zip((batch, single), frames):  # a frame rendered before the batch and again after it
        ctx.begin_frame(200, 120, True, (0.2, 0.2, 0.2, 1.0))
        ctx.draw_image(40, (10.0, 8.0), WHITE, (125.0, 100.0))
        ctx.end_frame()
        assert np.array_equal(ctx.read_pixels(), frame)
    batch.remove_image(1), single.remove_image(1)
    assert batch.put_image_sdf_of(2, 9, channel=3, pad=3, sdf_range=6) == single.put_image_sdf_of(2, 9, channel=3, pad=3, sdf_range=6)
    same_atlases(batch, single, "a field of a batch-put entry")
    a, b = batch.compact_atlas(), single.compact_atlas()
    assert (a["entries"], a["rects_moved"], a["texels"]) == (b["entries"], b["rects_moved"], b["texels"]) and a["entries"] == 4
    assert [batch.image_rect(k) for k in (2, 3, 9, 40)] == [single.image_rect(k) for k in (2, 3, 9, 40)]
    same_atlases(batch, single, "compacted")
    batch.close(), single.close()


# ------------------------------------------------------------------------------------------------------------------ the binding
def test_tensors():
    """an N x C x H x W float16 tensor through put_image_tensors against N put_image_tensor calls: tests/device_images_tensor_child.py, in a
    process of its own -- torch brings its own copies of the ROCm libraries, and this process has loaded the system's"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_images_tensor_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device_images_tensor_child: OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
