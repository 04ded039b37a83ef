"""A batch of distance-field glyphs in one call on the device (fdh_put_glyph_outlines, include_glyphs/figdraw_hip_glyphs.h: k_msdf_generate_batch,
k_msdf_generate_union_batch, k_msdf_correct_batch, k_msdf_correct_union_batch, k_atlas_blit_batch, k_minify2_batch).  The yardstick is the
single call, which test_msdf.py, test_msdf_correct.py and test_msdf_overlap.py hold to the float64 references: every comparison here is
equality of bytes between a context filled by one batch and a context filled by single calls in the same order."""
import numpy as np
import pytest

import msdf_cases as MC
from test_msdf_batch_host import SQUARE, small_shapes, square

pytestmark = pytest.mark.gpu
WHITE = [(255, 255, 255, 255)] * 4
FLAGS = [dict(correct=c, overlap=o) for c in (False, True) for o in (False, True)]


def contexts(atlas_size=2048):
    from figdraw_amd.context import HipContext

    return HipContext(atlas_size=atlas_size, device=0), HipContext(atlas_size=atlas_size, device=0)


def fill_both(glyphs, atlas_size=2048, first_key=5000, **kw):
    """glyphs: [(name, segs, w, h, R)] -> the context filled by one batch, the one filled by single calls, the keys; rectangles checked"""
    a, b = contexts(atlas_size)
    keys = [first_key + i for i in range(len(glyphs))]
    rects = a.put_glyph_outlines([(k, segs, w, h, R) for k, (_, segs, w, h, R) in zip(keys, glyphs)], **kw)
    singles = [b.put_glyph_outline(k, segs, w, h, mtsdf=True, sdf_range=R, **kw) for k, (_, segs, w, h, R) in zip(keys, glyphs)]
    assert rects == singles
    assert a.atlas_size() == b.atlas_size()
    return a, b, keys


def same_level0(a, b, what=""):
    la, lb = a.debug_read_surface(4), b.debug_read_surface(4)
    assert la.shape == lb.shape
    assert np.array_equal(la, lb), f"{what}: {int((la != lb).any(axis=2).sum())} texels of level 0 differ"
    return la


@pytest.fixture(scope="module")
def font():
    """the 106 font inputs into a 2048 atlas, once as one batch and once as 106 single calls -> (batch context, singles context, keys, inputs)"""
    inputs = MC.inputs()
    a, b, keys = fill_both(inputs)
    yield a, b, keys, inputs
    a.close()
    b.close()


def test_font_set_level_0_is_the_single_calls(font):
    a, b, keys, inputs = font
    assert len(inputs) == 106 and a.atlas_size() == 2048
    atlas = same_level0(a, b, "the font set")  # whole arrays: the margins and everything outside the rectangles too
    assert atlas.any()
    st = a.glyph_batch_stats()
    assert st["glyphs"] == st["written"] == 106 and st["dropped_by_growth"] == 0
    assert st["tiles"] == sum(((w + 7) // 8) * ((h + 7) // 8) for _, _, w, h, _ in inputs) and st["edges"] > 0 and st["bytes_copied"] > st["edges"] * 96


@pytest.mark.parametrize("kw", FLAGS, ids=lambda kw: "+".join(k for k, v in kw.items() if v) or "plain")
def test_hostile_set(kw):
    """the 71 hostile outlines, 16 383 squares in one glyph and a glyph without segments, each with its own range"""
    from test_msdf import DEVICE_ONLY

    glyphs = [c[:5] for c in MC.hostile_inputs()] + DEVICE_ONLY
    assert len(glyphs) == 73 and len({g[4] for g in glyphs}) > 1
    a, b, _ = fill_both(glyphs, **kw)
    same_level0(a, b, f"hostile set, {kw}")
    a.close()
    b.close()


@pytest.mark.parametrize("order", ["given", "reversed"])
def test_small_shapes(order):
    """1 x 1, 9 x 1, 1 x 9, 8 x 8, 7 x 9 and 17 x 23 with a 0-segment glyph between them: the tile table's boundaries, partial tiles, the level-0
    rule for fields 1 texel wide or high"""
    glyphs = small_shapes() if order == "given" else small_shapes()[::-1]
    for kw in (FLAGS[0], FLAGS[3]):
        a, b, keys = fill_both(glyphs, atlas_size=256, **kw)
        same_level0(a, b, f"small shapes {order}, {kw}")
        a.close()
        b.close()


def test_small_shapes_are_written():
    """what the comparison above cannot show if both sides wrote nothing: a field 1 texel wide or high has its texels in level 0"""
    glyphs = small_shapes()
    a, b, keys = fill_both(glyphs, atlas_size=256)
    b.close()
    b = a  # a second batch, into a context that holds the first: new rectangles, whose texels nothing has written before
    rects = b.put_glyph_outlines([(9000 + i, segs, w, h, R) for i, (_, segs, w, h, R) in enumerate(glyphs)])
    atlas = b.debug_read_surface(4)
    for (name, segs, w, h, R), (x, y, rw, rh) in zip(glyphs, rects):
        if len(segs):
            assert atlas[y:y + rh, x:x + rw, 3].any(), name  # a texel inside the square or within the range of it: its true distance is not stored as 0
    assert all(a.has_image(k) for k in keys)
    a.close()


def test_a_batch_of_one_is_the_single_call():
    name, segs, w, h, R = MC.inputs()[40]
    for kw in FLAGS:
        a, b, _ = fill_both([(name, segs, w, h, R)], atlas_size=256, **kw)
        same_level0(a, b, f"{name}, {kw}")
        assert a.glyph_batch_stats()["glyphs"] == 1
        a.close()
        b.close()


def _minified_frame(ctx, keys, sizes, scales):
    W = H = 256
    ctx.begin_frame(W, H, True, (0.1, 0.2, 0.3, 1.0))
    y = 4.0
    row = max(h for _, h in sizes)
    for s in scales:
        x = 4.0
        for k, (w, h) in zip(keys, sizes):
            if x + w * s > W - 4.0:  # the next row
                x, y = 4.0, y + row * s + 3.0
            ctx.draw_image(k, (x, y), WHITE, size=(w * s, h * s))
            x += w * s + 3.0
        y += row * s + 3.0
    assert y < H
    ctx.end_frame()
    return ctx.read_pixels()


def test_the_level_chain(font):
    """twelve font glyphs drawn at 1/2, 1/4 and 1/8 size (and, for the levels in which rectangles can meet, at 1/16 and 1/32) sample the deeper
    levels: the same bytes from the batch-filled and the singles-filled context, and not those of level-0-only images"""
    from figdraw_amd.context import HipContext

    a, b, keys, inputs = font
    pick = list(range(0, 96, 8))
    assert len(pick) == 12
    ks, sizes = [keys[i] for i in pick], [inputs[i][2:4] for i in pick]
    every = [c[2:4] for c in inputs]
    for scales, kk, ss in (((0.5, 0.25, 0.125), ks, sizes), ((1 / 16.0, 1 / 32.0), keys, every)):  # the deep levels: all 106, neighbours' rectangles meet there
        fa, fb = _minified_frame(a, kk, ss, scales), _minified_frame(b, kk, ss, scales)
        assert np.array_equal(fa, fb), f"scales {scales}: {int((fa != fb).any(axis=2).sum())} pixels differ"
    fa = _minified_frame(a, ks, sizes, (0.5, 0.25, 0.125))
    level0 = b.debug_read_surface(4)
    flat = HipContext(atlas_size=2048, device=0)
    rects = {}
    probe = HipContext(atlas_size=2048, record_only=True)  # where the glyphs lie: the same puts on a record-only context
    for k, (_, segs, w, h, R) in zip(keys, inputs):
        rects[k] = probe.put_glyph_outline(k, segs, w, h, mtsdf=True, sdf_range=R)
    probe.close()
    for k in ks:
        x, y, w, h = rects[k]
        flat.put_image_mips(k, [level0[y:y + h, x:x + w]])  # level 0 alone
    ff = _minified_frame(flat, ks, sizes, (0.5, 0.25, 0.125))
    flat.close()
    assert not np.array_equal(fa, ff), "the minified draws do not sample the deeper levels"


def test_growth_on_the_device():
    """atlas size 64 and twelve 40 x 40 outlines: the atlas grows more than once inside the batch"""
    glyphs = [(f"square {i}", square(40, 40), 40, 40, 4) for i in range(12)]
    a, b, keys = fill_both(glyphs, atlas_size=64, correct=True)
    assert a.atlas_size() > 64
    assert [a.has_image(k) for k in keys] == [b.has_image(k) for k in keys] and not all(b.has_image(k) for k in keys) and b.has_image(keys[-1])
    same_level0(a, b, "growth")
    st = a.glyph_batch_stats()
    assert st["dropped_by_growth"] == sum(not b.has_image(k) for k in keys) and st["written"] == 12 - st["dropped_by_growth"]
    a.close()
    b.close()


def test_launch_count_does_not_depend_on_the_number_of_glyphs(font):
    from figdraw_amd.context import HipContext

    a, _, _, inputs = font
    levels = 12  # a 2048 atlas: 2048, 1024, .. 1
    many = a.glyph_batch_stats()["launches"]
    assert 0 < many <= 2 + 2 * levels
    for kw in FLAGS:
        one, all_ = HipContext(atlas_size=2048, device=0), HipContext(atlas_size=2048, device=0)
        one.put_glyph_outlines([(1, SQUARE, 12, 11)], **kw)
        all_.put_glyph_outlines([(5000 + i, segs, w, h, R) for i, (_, segs, w, h, R) in enumerate(inputs)], **kw)
        n1, n106 = one.glyph_batch_stats()["launches"], all_.glyph_batch_stats()["launches"]
        assert n1 == n106 and 0 < n1 <= 2 + 2 * levels, kw
        assert n1 == many + (1 if kw["correct"] else 0)
        one.close()
        all_.close()


def test_a_refused_batch_leaves_the_device_untouched():
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    ctx.put_glyph_outlines([(1, square(40, 40), 40, 40), (2, SQUARE, 12, 11)])
    before = ctx.debug_read_surface(4)
    with pytest.raises(FigdrawHipError) as e:
        ctx.put_glyph_outlines([(10, SQUARE, 12, 11), (11, SQUARE[:3], 12, 11), (12, SQUARE, 12, 11)])
    assert e.value.code == -1
    assert [ctx.has_image(k) for k in (1, 2, 10, 11, 12)] == [True, True, False, False, False]
    assert np.array_equal(ctx.debug_read_surface(4), before) and before.any()
    ctx.close()


def test_other_work_is_undisturbed():
    """a batch issued while a frame of coverage glyphs is in flight: that frame, and the one before it, are those of a context that got no batch"""
    import os

    from conftest import GOLDEN
    from figdraw_amd.context import HipContext
    from figdraw_amd.scene import Fig, FigKind, RenderList, Renders, rect, rgba
    from figdraw_amd.scenes import load_glyph_fixture

    imgs = load_glyph_fixture(os.path.join(GOLDEN, "glyphs_ubuntu20.npz"))
    gk = sorted(k for k in imgs if 1000 <= k < 1100)[:24]
    w, h = 640, 400

    def scene(shift):
        lst = RenderList()
        lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(0, 0, w, h), fill=rgba(20, 24, 40, 255)))
        for i, k in enumerate(gk):
            gh, gw = imgs[k].shape[:2]
            for row, scale in enumerate((1.0, 2.5, 0.45)):
                f = Fig(kind=FigKind.nkImage, screenBox=rect(12 + 26 * i + shift, 20 + 110 * row + (i % 3) * 0.5, gw * scale, gh * scale), fill=rgba(255, 255, 255, 255))
                f.image_id = k
                lst.addRoot(f)
        sc = Renders()
        sc.setLayer(0, lst)
        return sc

    frames = {}
    for batch in (True, False):
        a = HipContext(atlas_size=512, device=0)
        for k in gk:
            a.put_glyph_image(k, imgs[k], lcd_filter=True)
        a.render_frame(scene(0.0), w, h)
        first = a.read_pixels()
        a.render_frame(scene(3.25), w, h)  # in flight ...
        if batch:  # ... while the batch is put
            a.put_glyph_outlines([(5000 + i, segs, gw, gh, R) for i, (_, segs, gw, gh, R) in enumerate(MC.inputs()[:20])], correct=True)
            assert a.atlas_size() == 512
        frames[batch] = (first, a.read_pixels())
        a.close()
    assert np.array_equal(frames[True][0], frames[False][0]) and np.array_equal(frames[True][1], frames[False][1])
    assert not np.array_equal(frames[True][0], frames[True][1])
