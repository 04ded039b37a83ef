"""A batch of coverage glyphs in one call on the device (fdh_put_glyph_coverage_batch, include_glyphs/figdraw_hip_coverage.h: k_coverage_cells_batch,
k_coverage_sum_batch, k_lcd_filter_batch, k_atlas_blit_batch, k_minify2_batch).  Two yardsticks: a context filled by single calls in the same
order, byte for byte, and the oracle's rasteriser and LCD filter pasted at the returned rectangles, which owe nothing to the code under test."""
import numpy as np
import pytest

import coverage_cases as CC
from test_coverage_batch_host import ATLAS_FULL, FULL_BATCH, INVALID, SQUARE, TRIANGLE, full_atlas

pytestmark = pytest.mark.gpu
WHITE = [(255, 255, 255, 255)] * 4
MODES = {"plain": (False, None, False), "lcd": (True, None, True), "context on": ("context", True, True), "context off": ("context", False, False)}


def fill_both(glyphs, atlas_size=1024, first_key=5000, mode="plain"):
    """glyphs: [(name, segs, w, h)] -> the context filled by one batch, the one filled by single calls, the keys, the rectangles (checked equal)"""
    from figdraw_amd.context import HipContext

    flag, switch, filtered = MODES[mode]
    a, b = HipContext(atlas_size=atlas_size, device=0), HipContext(atlas_size=atlas_size, device=0)
    if switch is not None:
        a.set_text_lcd_filtering(switch)
    keys = [first_key + i for i in range(len(glyphs))]
    rects = a.put_glyph_coverage_batch([(k, segs, w, h) for k, (_, segs, w, h) in zip(keys, glyphs)], lcd_filter=flag)
    singles = [b.put_glyph_outline(k, segs, w, h, lcd_filter=filtered) for k, (_, segs, w, h) in zip(keys, glyphs)]
    assert rects == singles
    assert a.atlas_size() == b.atlas_size()
    return a, b, keys, rects


def same_level0(a, b, what=""):
    la, lb = a.debug_read_surface(4), b.debug_read_surface(4)
    assert la.shape == lb.shape
    assert np.array_equal(la, lb), f"{what}: {int((la != lb).any(axis=2).sum())} texels of level 0 differ"
    return la


def oracle_level0(size, glyphs, rects, lcd, present=None):
    """zeros plus the oracle's image of every glyph at its rectangle; nothing for a glyph 1 texel wide or high, nor for one not `present`"""
    from oracle import oracle as O

    want = np.zeros((size, size, 4), np.uint8)
    for i, ((_, segs, w, h), (x, y, rw, rh)) in enumerate(zip(glyphs, rects)):
        assert (rw, rh) == (w, h)
        if w > 1 and h > 1 and (present is None or present[i]):
            want[y:y + h, x:x + w] = CC.oracle_image(O, segs, w, h, lcd)
    return want


@pytest.fixture(scope="module")
def font():
    """the 94 font outlines into a 1024 atlas per mode, once as one batch and once as single calls -> {mode: (batch context, singles context, keys, rects)}"""
    glyphs = CC.font()
    assert len(glyphs) == 94 and sum(w * h for _, _, w, h in glyphs) == 19820
    filled = {mode: fill_both(glyphs, mode=mode) for mode in MODES}
    yield glyphs, filled
    for a, b, _, _ in filled.values():
        a.close()
        b.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_font_set_level_0(font, mode):
    glyphs, filled = font
    a, b, keys, rects = filled[mode]
    assert a.atlas_size() == 1024
    atlas = same_level0(a, b, f"the font set, {mode}")  # whole arrays: the margins and everything outside the rectangles too
    want = oracle_level0(1024, glyphs, rects, MODES[mode][2])
    assert want.any() and np.array_equal(atlas, want), f"{mode}: {int((atlas != want).any(axis=2).sum())} texels differ from the oracle's"
    st = a.glyph_coverage_batch_stats()
    assert st["glyphs"] == st["written"] == 94 and st["dropped_by_growth"] == 0
    assert st["tiles"] == sum(((w + 7) // 8) * ((h + 7) // 8) for _, _, w, h in glyphs)
    assert st["edges"] == 4108 and st["bytes_copied"] >= st["edges"] * 16 + 94 * 64 + st["tiles"] * 4  # the font's flattened lines (fo_flatten_outline)
    assert a.glyph_batch_stats()["glyphs"] == 0  # fdh_glyph_batch_stats is fdh_put_glyph_outlines'


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


@pytest.mark.parametrize("mode", ["plain", "lcd"])
def test_the_level_chain(font, mode):
    """the font glyphs drawn at 1/2, 1/4 and 1/8 size, and at 1/16 and 1/32 (the levels in which neighbours' rectangles meet), sample levels 1 to 5:
    the same bytes from the batch-filled and the singles-filled context, within the suite's tolerance of the oracle, and not those of level 0 alone"""
    from conftest import diff_stats
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    glyphs, filled = font
    a, b, keys, rects = filled[mode]
    sizes = [g[2:4] for g in glyphs]
    orc = O.Oracle(atlas_size=1024, threads=8)
    for k, (_, segs, w, h), r in zip(keys, glyphs, rects):
        assert orc.put_glyph_outline(k, segs, w, h, lcd_filter=MODES[mode][2]) == r
    for scales in ((0.5, 0.25, 0.125), (1 / 16.0, 1 / 32.0)):
        fa, fb, fo = (_minified_frame(c, keys, sizes, scales) for c in (a, b, orc))
        assert np.array_equal(fa, fb), f"scales {scales}: {int((fa != fb).any(axis=2).sum())} pixels differ"
        mx, n0, n1 = diff_stats(fa, fo)
        print(f"{mode}, scales {scales}: against the oracle max {mx} LSB, {n0} pixels differ, {n1} by more than 1")
        assert mx <= 1 and n0 <= 0.005 * 256 * 256, (scales, mx, n0, n1)
    orc.close()
    fa = _minified_frame(a, keys, sizes, (0.5, 0.25, 0.125))
    level0 = b.debug_read_surface(4)
    flat = HipContext(atlas_size=1024, device=0)
    for k, (x, y, w, h) in zip(keys, rects):
        flat.put_image_mips(k, [level0[y:y + h, x:x + w]])  # level 0 alone
    ff = _minified_frame(flat, keys, sizes, (0.5, 0.25, 0.125))
    flat.close()
    assert not np.array_equal(fa, ff), "the minified draws do not sample the deeper levels"


@pytest.mark.parametrize("mode", ["plain", "lcd"])
@pytest.mark.parametrize("order", ["given", "reversed"])
def test_shapes(order, mode):
    """the smallest shapes at which the batch can go wrong, between one another and with a 0-segment glyph among them"""
    glyphs = CC.shapes() if order == "given" else CC.shapes()[::-1]
    a, b, keys, rects = fill_both(glyphs, atlas_size=512, mode=mode)
    assert a.atlas_size() == 512
    atlas = same_level0(a, b, f"shapes {order}, {mode}")
    want = oracle_level0(512, glyphs, rects, MODES[mode][2])
    for (name, segs, w, h), (x, y, _, _) in zip(glyphs, rects):
        assert np.array_equal(atlas[y:y + h, x:x + w], want[y:y + h, x:x + w]), name
        if w == 1 or h == 1:
            assert not atlas[y:y + h, x:x + w].any(), f"{name}: a single put writes no texel of it"
        elif len(segs):
            assert atlas[y:y + h, x:x + w].any(), name
    assert np.array_equal(atlas, want)
    assert all(a.has_image(k) for k in keys)
    a.close()
    b.close()


def test_a_batch_of_one_and_the_leaving_set():
    """one glyph alone; and the 94 outlines scaled 3.7 x, which leave their images on all sides"""
    for glyphs in ([CC.font()[70]], CC.scaled()):
        a, b, keys, rects = fill_both(glyphs, mode="lcd")
        atlas = same_level0(a, b, glyphs[0][0])
        assert np.array_equal(atlas, oracle_level0(1024, glyphs, rects, True))
        assert a.glyph_coverage_batch_stats()["glyphs"] == len(glyphs)
        a.close()
        b.close()


def test_growth_on_the_device():
    """atlas size 64 and twelve 40 x 40 outlines: the atlas grows more than once inside the batch"""
    glyphs = [(f"square {i}", CC.shifted(CC.square(40, 40), 0.25 * i), 40, 40) for i in range(12)]
    a, b, keys, rects = fill_both(glyphs, atlas_size=64, mode="lcd")
    assert a.atlas_size() > 64
    present = [b.has_image(k) for k in keys]
    assert [a.has_image(k) for k in keys] == present and not all(present) and present[-1]
    atlas = same_level0(a, b, "growth")
    assert np.array_equal(atlas, oracle_level0(a.atlas_size(), glyphs, rects, True, present))
    st = a.glyph_coverage_batch_stats()
    assert st["dropped_by_growth"] == sum(not p for p in present) and st["written"] == 12 - st["dropped_by_growth"]
    a.close()
    b.close()


def test_a_refused_batch_leaves_the_device_untouched():
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    ctx.put_glyph_coverage_batch([(1, CC.square(40, 40), 40, 40), (2, SQUARE, 12, 11)])
    before, stats = ctx.debug_read_surface(4), ctx.glyph_coverage_batch_stats()
    with pytest.raises(FigdrawHipError) as e:
        ctx.put_glyph_coverage_batch([(10, SQUARE, 12, 11), (11, SQUARE, 12, 4097), (12, SQUARE, 12, 11)])
    assert e.value.code == INVALID
    assert [ctx.has_image(k) for k in (1, 2, 10, 11, 12)] == [True, True, False, False, False]
    assert np.array_equal(ctx.debug_read_surface(4), before) and before.any() and ctx.glyph_coverage_batch_stats() == stats and stats["launches"] > 0
    ctx.close()


def test_atlas_full_part_way_through():
    """the largest atlas with nine 4096 x 4096 rectangles in it: the batch's third glyph finds no place; the two before it are in the atlas with
    their texels (drawn 1:1 at integer positions on black, the frame is the atlas content), the one behind it is not"""
    from figdraw_amd.context import FigdrawHipError
    from oracle import oracle as O

    ctx = full_atlas(device=0)
    with pytest.raises(FigdrawHipError) as e:
        ctx.put_glyph_coverage_batch(FULL_BATCH, lcd_filter=True)
    assert e.value.code == ATLAS_FULL and ctx.atlas_size() == 16384
    assert [ctx.has_image(g[0]) for g in FULL_BATCH] == [True, True, False, False]
    st = ctx.glyph_coverage_batch_stats()
    assert st["glyphs"] == 4 and st["written"] == 2 and st["dropped_by_growth"] == 0 and st["launches"] > 0
    orc = O.Oracle(atlas_size=64, threads=4)
    for k, segs, w, h in FULL_BATCH[:2]:
        orc.put_glyph_outline(k, segs, w, h, lcd_filter=True)
    for c in (ctx, orc):
        c.begin_frame(64, 32, True, (0, 0, 0, 1))
        c.draw_image(10, (2, 3), WHITE)
        c.draw_image(11, (30, 5), WHITE)
        c.end_frame()
    got, want = ctx.read_pixels(), orc.read_pixels()
    assert got[..., :3].max() > 200 and np.array_equal(got, want)
    orc.close()
    ctx.close()


def test_coverage_and_distance_field_batches_on_one_context():
    """either order: each keeps the other's texels and figures"""
    from figdraw_amd.context import HipContext

    cov = [(100 + i, segs, w, h) for i, (_, segs, w, h) in enumerate(CC.font()[:20])]
    sdf = [(200, SQUARE, 12, 11, 4), (201, TRIANGLE, 12, 11, 2), (202, CC.square(17, 23), 17, 23, 8)]
    for first in ("coverage", "fields"):
        a, b = HipContext(atlas_size=512, device=0), HipContext(atlas_size=512, device=0)
        for which in ((0, 1) if first == "coverage" else (1, 0)):
            if which == 0:
                assert a.put_glyph_coverage_batch(cov, lcd_filter=True) == [b.put_glyph_outline(k, segs, w, h, lcd_filter=True) for k, segs, w, h in cov]
            else:
                assert a.put_glyph_outlines(sdf, correct=True) == [b.put_glyph_outline(k, segs, w, h, mtsdf=True, sdf_range=R, correct=True) for k, segs, w, h, R in sdf]
        assert same_level0(a, b, f"{first} first").any()
        c, f = a.glyph_coverage_batch_stats(), a.glyph_batch_stats()
        assert c["glyphs"] == c["written"] == 20 and c["edges"] > 20 and f["glyphs"] == f["written"] == 3 and f["edges"] > 0
        a.close()
        b.close()


def test_launch_count_does_not_depend_on_the_number_of_glyphs(font):
    from figdraw_amd.context import HipContext

    glyphs, filled = font
    levels = 11  # a 1024 atlas: 1024, 512, .. 1
    for mode, extra in (("plain", 0), ("lcd", 1)):
        many = filled[mode][0].glyph_coverage_batch_stats()["launches"]
        one = HipContext(atlas_size=1024, device=0)
        one.put_glyph_coverage_batch([(1, SQUARE, 12, 11)], lcd_filter=MODES[mode][0])
        n1 = one.glyph_coverage_batch_stats()["launches"]
        one.close()
        assert n1 == many == 2 + extra + 2 * levels - 1, mode


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
            a.put_glyph_coverage_batch([(5000 + i, segs, gw, gh) for i, (_, segs, gw, gh) in enumerate(CC.font()[:40])], lcd_filter=True)
            assert a.atlas_size() == 512
        frames[batch] = (first, a.read_pixels())
        a.close()
    assert np.array_equal(frames[True][0], frames[False][0]) and np.array_equal(frames[True][1], frames[False][1])
    assert not np.array_equal(frames[True][0], frames[True][1])
