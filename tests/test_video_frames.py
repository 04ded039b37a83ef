"""Batches of decoded video frames on the device (fdh_put_video_frames, fdh_update_video_frames; k_video_import_batch,
k_image_import_tail_batch): two contexts per case, one filled by the batch, one by single calls of the same planes in the same order.  The
bar is identity: rectangles, has_image, usage, every level of both atlases byte for byte, the draw records of a frame that draws every
entry once, which holds the ink boxes, and its pixels.  Level 0 is also held to the reference's conversion (tests/video_frame_ref.py)."""
import numpy as np
import pytest

import coverage_cases as CC
import video_frame_cases as VC
import video_frame_ref as REF
from test_video_frame import WHITE, Memory, levels_of, nv12, same_atlases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def memory():
    m = Memory()
    yield m
    m.free()


def uploaded(memory, key, case, pinned=False):
    """-> an item of put_video_frames: the case's planes in device (page-locked) memory"""
    w, h = VC.size_of(case)
    (ybuf, yalign, ypitch), c = VC.pack(case)
    place = (lambda data, align: memory.page_locked(data)) if pinned else memory.upload
    y_ptr = place(ybuf, yalign)
    uv_ptr, cpitch = (place(c[0], c[1]), c[2]) if c else (0, 0)
    return (key, y_ptr, uv_ptr, w, h, ypitch, cpitch, case[1], case[2], case[3], case[4])


def single_put(ctx, it, update=False):
    return (ctx.update_video_frame if update else ctx.put_video_frame)(*it[:7], format=it[7], matrix=it[8], range=it[9], flags=it[10])


def digest_of_a_frame(ctx, items, rects):
    """every frame that is still in the atlas drawn once, magnified 1.5 times -> the digest of the draw records"""
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


def same_contexts(batch, single, items, rects, what):
    same_atlases(batch, single, what)
    assert [batch.has_image(it[0]) for it in items] == [single.has_image(it[0]) for it in items], what
    assert digest_of_a_frame(batch, items, rects) == digest_of_a_frame(single, items, rects), what
    assert np.array_equal(batch.read_pixels(), single.read_pixels()), what


def both_ways(items, atlas_size=256, keep=False, what=""):
    """the items as one batch and as single calls -> (the batch's context, the single calls' context, the rectangles)"""
    from figdraw_amd.context import HipContext

    batch, single = HipContext(atlas_size=atlas_size, device=0), HipContext(atlas_size=atlas_size, device=0)
    for ctx in (batch, single):
        ctx.set_atlas_keep(keep)
    rects = batch.put_video_frames(items)
    if keep and batch.atlas_size() != atlas_size:
        # (include_glyphs/figdraw_hip_atlas.h: a batch in keep mode makes room once, before its first frame, and equals single calls from there on)
        single.compact_atlas(batch.atlas_size())
    assert rects == [single_put(single, it) for it in items], what
    same_contexts(batch, single, items, rects, what)
    return batch, single, rects


def batch_cases(**kw):
    """VC.cases under names of their own: VC.texels keeps its results by name, and cases(largest=False) draws other noise for the cases
    behind the sizes than the cases() of the single calls' tests do"""
    return [("batch " + c[0],) + c[1:] for c in VC.cases(**kw)]


def level0_is_the_reference(ctx, cases, rects):
    level0 = ctx.read_atlas_level(0)
    for case, (x, y, w, h) in zip(cases, rects):  # (nothing of a line)
        want = VC.texels(case) if w > 1 and h > 1 else np.zeros((h, w, 4), np.uint8)
        assert np.array_equal(level0[y:y + h, x:x + w], want), case[0]


# ------------------------------------------------------------------------------------------------------------------ identity with single calls
@pytest.fixture(scope="module")
def mixed(memory):
    """all of cases(largest=False): the five groups, every layout, matrix, range and flag; the planes are uploaded once"""
    cases = batch_cases(largest=False)
    return cases, [uploaded(memory, 100 + i, c) for i, c in enumerate(cases)]


@pytest.mark.parametrize("order", ["given", "reversed"])
def test_the_mixed_batch(mixed, order):
    cases, items = mixed
    if order == "reversed":
        cases, items = cases[::-1], items[::-1]
    batch, single, rects = both_ways(items, atlas_size=1024, what=f"the mixed batch, {order}")
    assert len(items) >= 40 and batch.atlas_size() == 1024
    st = batch.video_batch_stats()
    assert (st["frames"], st["written"], st["dropped_by_growth"], st["launches"]) == (len(items), len(items), 0, 6)  # five groups and the tails
    assert st["tiles"] == sum(-(-it[3] // 32) * -(-it[4] // 32) for it in items) and st["bytes_copied"] > 0
    level0_is_the_reference(batch, cases, rects)
    batch.close(), single.close()


def test_a_batch_of_one(mixed):
    cases, items = mixed
    k = next(i for i, c in enumerate(cases) if VC.size_of(c) == (33, 31) and c[1] == REF.P010)
    batch, single, rects = both_ways([items[k]], what="one")
    assert batch.video_batch_stats()["launches"] == 1
    level0_is_the_reference(batch, [cases[k]], rects)
    batch.close(), single.close()


def test_lines_alone_store_nothing_but_are_measured(mixed):
    cases, items = mixed
    lines = [it for it, c in zip(items, cases) if VC.size_of(c) in ((1, 1), (1, 9))]
    assert len(lines) == 4
    batch, single, _ = both_ways(lines, what="lines")
    st = batch.video_batch_stats()
    assert (st["written"], st["tiles"]) == (4, 4) and 1 <= st["launches"] <= 4  # a tile each, whose ink blocks the device makes; no tail
    assert not any(level.any() for level in levels_of(batch))
    batch.close(), single.close()


def pair(memory):
    rng = np.random.default_rng(11)
    luma, chroma = VC.noise_yuv(rng, REF.P010, 100, 100)
    a = ("batch pair a", REF.BGRA8, 0, 0, REF.STRAIGHT_ALPHA, VC.noise_bgra(rng, 100, 100), None, "tight")
    b = ("batch pair b", REF.P010, REF.BT2020, REF.FULL, REF.CHROMA_LINEAR, luma, chroma, "padded")
    return (a, b), (uploaded(memory, 1, a), uploaded(memory, 2, b))


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_the_level_6_pair(memory, order):
    cases, two = pair(memory)
    batch, single, rects = both_ways([two[k] for k in order], what=f"the pair {order}")
    assert rects == [(4, 4, 100, 100), (112, 4, 100, 100)]  # level 6: columns 0 .. 1 and 1 .. 2
    assert batch.video_batch_stats()["launches"] == 3  # two groups, and the tails
    level0_is_the_reference(batch, [cases[k] for k in order], rects)
    batch.close(), single.close()


def test_frames_against_the_right_and_bottom_edges(memory):
    rng = np.random.default_rng(12)
    items = [uploaded(memory, k, nv12(rng, 247, (120, 112)[k - 1], flags=k & 1, layout="padded", name=f"batch edge {k}", matrix=REF.BT601, rgn=REF.FULL)) for k in (1, 2)]
    batch, single, rects = both_ways(items, what="edges")
    assert batch.atlas_size() == 256 and rects[1][0] + rects[1][2] == 251 and rects[1][1] + rects[1][3] == 252
    batch.close(), single.close()


@pytest.mark.parametrize("keep", [False, True])
def test_growth_in_the_middle_of_a_batch(memory, keep):
    rng = np.random.default_rng(14)
    sizes = [(100, 100), (100, 100), (60, 60), (120, 120), (90, 40), (33, 31)]
    items = [uploaded(memory, k, nv12(rng, w, h, flags=k & 1, layout=("tight", "padded")[k & 1], name=f"batch growth {k} keep {keep}")) for k, (w, h) in enumerate(sizes, start=1)]
    batch, single, _ = both_ways(items, keep=keep, what=f"growth, keep {keep}")
    assert batch.atlas_size() == 512
    st = batch.video_batch_stats()
    alive = [batch.has_image(k) for k in range(1, 7)]
    assert st["dropped_by_growth"] == alive.count(False) and st["written"] == alive.count(True)
    assert (st["dropped_by_growth"] == 0) == keep
    batch.close(), single.close()


def test_planes_in_page_locked_host_memory(memory):
    rng = np.random.default_rng(17)
    luma, chroma = VC.noise_yuv(rng, REF.P010, 33, 31)
    cases = [nv12(rng, 70, 45, flags=REF.CHROMA_LINEAR, name="batch pinned", matrix=REF.BT2020), ("batch pinned words", REF.P010, REF.BT601, REF.LIMITED, 0, luma, chroma, "tight"),
             ("batch pinned bytes", REF.BGRA8, 0, 0, REF.IGNORE_ALPHA, VC.noise_bgra(rng, 1, 9), None, "tight")]
    items = [uploaded(memory, k, c, pinned=True) for k, c in enumerate(cases, start=1)]
    batch, single, rects = both_ways(items, what="page-locked")
    level0_is_the_reference(batch, cases, rects)
    batch.close(), single.close()


def test_the_largest_case_has_a_real_tail(memory):
    """514 x 258: a level-5 image of 17 x 9 that the tail's workgroup takes through four more levels"""
    cases = [c for c in batch_cases() if VC.size_of(c) == VC.LARGEST]
    assert len(cases) == 2
    items = [uploaded(memory, k, c) for k, c in enumerate(cases, start=1)]
    batch, single, rects = both_ways(items, atlas_size=1024, what="the largest")
    assert batch.atlas_size() == 1024 and batch.read_atlas_level(8).any()
    level0_is_the_reference(batch, cases, rects)
    batch.close(), single.close()


# ------------------------------------------------------------------------------------------------------------------ updates
def test_an_update_batch_of_a_permuted_subset(mixed, memory):
    """put everything, then the next frames -- cases(again=True): other noise, other flags or matrices where the sizes allow -- for a
    permuted subset, in one batch against single updates"""
    from figdraw_amd.context import HipContext

    cases, items = mixed
    nxt = batch_cases(largest=False, again=True)
    batch, single = HipContext(atlas_size=1024, device=0), HipContext(atlas_size=1024, device=0)
    rects = batch.put_video_frames(items)
    assert rects == [single_put(single, it) for it in items]
    order = [k for k in np.random.default_rng(21).permutation(len(cases)) if k % 3 != 1]
    assert 20 < len(order) < len(cases) and {VC.size_of(cases[k]) for k in order} >= {(1, 9), (127, 129), (128, 128)}
    fresh = [uploaded(memory, 100 + int(k), nxt[k]) for k in order]
    epoch = batch.atlas_usage()["epoch"]
    batch.update_video_frames(fresh)
    for it in fresh:
        single_put(single, it, update=True)
    assert batch.atlas_usage()["epoch"] == epoch + len(order)
    st = batch.video_batch_stats()
    assert (st["frames"], st["written"], st["dropped_by_growth"]) == (len(order), len(order), 0) and st["launches"] <= 6
    same_contexts(batch, single, items, rects, "updated")
    level0 = batch.read_atlas_level(0)
    for k, (x, y, w, h) in enumerate(rects):
        if w > 1 and h > 1:
            assert np.array_equal(level0[y:y + h, x:x + w], VC.texels(nxt[k] if k in order else cases[k])), cases[k][0]
    batch.close(), single.close()


# ------------------------------------------------------------------------------------------------------------------ launch counts
def test_launches_do_not_depend_on_the_number_of_frames(memory):
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(22)
    luma, chroma = VC.noise_yuv(rng, REF.P010, 71, 65)
    kinds = [nv12(rng, 70, 65, name="batch count a"), ("batch count b", REF.P010, REF.BT709, REF.FULL, REF.CHROMA_LINEAR, luma, chroma, "tight"),
             ("batch count c", REF.BGRA8, 0, 0, 0, VC.noise_bgra(rng, 72, 65), None, "tight")]
    sources = [uploaded(memory, 0, c) for c in kinds]  # (three sources: a frame's key is its item's alone)
    ctx = HipContext(atlas_size=2048, device=0)
    counts = []
    for n in (3, 30):
        ctx.reset_atlas(0)
        ctx.put_video_frames([(k + 1,) + sources[k % 3][1:] for k in range(n)])
        st = ctx.video_batch_stats()
        assert st["written"] == n and st["tiles"] == 9 * n
        counts.append(st["launches"])
    assert counts[0] == counts[1] == 4  # three groups and the tails
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ refusals on the device
def test_a_refused_batch_changes_nothing(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    rng = np.random.default_rng(23)
    items = [uploaded(memory, k, nv12(rng, 40, 30, name=f"batch refused {k}")) for k in (1, 2, 3)]
    ctx = HipContext(atlas_size=256, device=0)
    rects = ctx.put_video_frames(items)
    before = (ctx.atlas_usage(), levels_of(ctx), digest_of_a_frame(ctx, items, rects), ctx.video_batch_stats())
    luma, chroma = np.zeros((30, 40), np.uint8), np.zeros((15, 20, 2), np.uint8)
    hostile = [
        ([(7,) + items[0][1:], (8,) + items[1][1:], (9, luma.ctypes.data, items[2][2], 40, 30, 40, 40)], "neither device memory of the context's device nor page-locked host memory"),
        ([(7,) + items[0][1:], (8, items[1][1], chroma.ctypes.data, 40, 30, 40, 40), (9,) + items[2][1:]], "neither device memory of the context's device nor page-locked host memory"),
        ([(7,) + items[0][1:], (8,) + items[1][1:], (7,) + items[2][1:]], "a key occurs twice"),
    ]
    for update in (False, True):
        for bad, text in hostile:
            if update:
                bad = [(k,) + it[1:] for k, it in zip((1, 2, 1 if "twice" in text else 3), bad)]
            with pytest.raises(FigdrawHipError) as e:
                (ctx.update_video_frames if update else ctx.put_video_frames)(bad)
            assert e.value.code == -1 and text in str(e.value)
            after = (ctx.atlas_usage(), levels_of(ctx), digest_of_a_frame(ctx, items, rects), ctx.video_batch_stats())
            assert after[0] == before[0] and after[2:] == before[2:] and all(np.array_equal(x, y) for x, y in zip(after[1], before[1])), (update, text)
            assert not any(ctx.has_image(k) for k in (7, 8, 9))
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    assert ctx.put_video_frames([(7,) + items[0][1:]])[0][2:] == (40, 30)  # and the context works on
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ other users of the atlas
def test_other_users_of_the_atlas(memory):
    """a glyph batch before and after the frames (the batches share their table buffer), a distance field of a batch-put entry, a compaction"""
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(24)
    luma, chroma = VC.noise_yuv(rng, REF.P010, 61, 35)
    cases = [nv12(rng, 40, 30, name="batch users 0"), ("batch users 1", REF.P010, REF.BT601, REF.LIMITED, 0, luma, chroma, "padded"),
             ("batch users 2", REF.BGRA8, 0, 0, 0, VC.noise_bgra(rng, 90, 33), None, "tight")]
    items = [uploaded(memory, k, c) for k, c in enumerate(cases, start=1)]
    batch, single = HipContext(atlas_size=512, device=0), HipContext(atlas_size=512, device=0)
    square, triangle = CC.poly([(2, 2), (10, 2), (10, 9), (2, 9)]), CC.poly([(2, 2), (10, 2), (6, 9)])
    old = VC.noise_bgra(rng, 50, 50)
    frames = []
    for ctx in (batch, single):
        ctx.put_image(40, old)
        assert ctx.put_glyph_coverage_batch([(50, square, 12, 11), (51, triangle, 12, 11)])
        ctx.begin_frame(200, 120, True, (0.2, 0.2, 0.2, 1.0))
        ctx.draw_image(40, (10.0, 8.0), WHITE, (125.0, 100.0))
        ctx.draw_image(51, (150.0, 8.0), WHITE, (24.0, 22.0))
        ctx.end_frame()
        frames.append(ctx.read_pixels())
    assert batch.put_video_frames(items) == [single_put(single, it) for it in items]
    for ctx, frame in zip((batch, single), frames):  # a frame rendered before the batch and again after it
        ctx.begin_frame(200, 120, True, (0.2, 0.2, 0.2, 1.0))
        ctx.draw_image(40, (10.0, 8.0), WHITE, (125.0, 100.0))
        ctx.draw_image(51, (150.0, 8.0), WHITE, (24.0, 22.0))
        ctx.end_frame()
        assert np.array_equal(ctx.read_pixels(), frame)
    for ctx in (batch, single):
        assert ctx.put_glyph_coverage_batch([(52, triangle, 12, 11), (53, square, 12, 11)])
    same_atlases(batch, single, "a glyph batch behind the frames")
    batch.remove_image(1), single.remove_image(1)
    assert batch.put_image_sdf_of(3, 9, channel=3, pad=3, sdf_range=6) == single.put_image_sdf_of(3, 9, channel=3, pad=3, sdf_range=6)
    same_atlases(batch, single, "a field of a batch-put entry")
    a, b = batch.compact_atlas(), single.compact_atlas()
    assert (a["entries"], a["rects_moved"], a["texels"]) == (b["entries"], b["rects_moved"], b["texels"]) and a["entries"] == 8
    keys = (2, 3, 9, 40, 50, 51, 52, 53)
    assert [batch.image_rect(k) for k in keys] == [single.image_rect(k) for k in keys]
    same_atlases(batch, single, "compacted")
    batch.close(), single.close()
