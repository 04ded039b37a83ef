"""A batch of distance-field glyphs with cubic segments in one call on the device (fdh_put_glyph_outlines_cubic,
include_glyphs/figdraw_hip_cubic_batch.h: k_msdf_generate_cubic_batch, k_msdf_correct_cubic_batch, then the level chain's batched kernels).  The
yardstick is the single call fdh_put_glyph_outline_cubic, which test_msdf_cubic.py holds to the float64 reference: every comparison here
but the analytic circle's is equality of bytes between a context filled by one batch and a context filled by single calls in the same order."""
import numpy as np
import pytest

import msdf_cases as MC
import msdf_cubic_cases as CC
import msdf_ref as M
from test_msdf_batch import WHITE, _minified_frame, same_level0
from test_msdf_cubic_batch_host import ATLAS_FULL, BOX, DEVICE_ONLY, FULL_BATCH, INVALID, SQUARE, cubic_square, full_atlas

pytestmark = pytest.mark.gpu
LEVELS_2048 = 12  # a 2048 atlas: 2048, 1024, .. 1


def contexts(atlas_size=2048):
    from figdraw_amd.context import HipContext

    return HipContext(atlas_size=atlas_size, device=0), HipContext(atlas_size=atlas_size, device=0)


def fill_both(glyphs, atlas_size=2048, first_key=5000, correct=False):
    """glyphs: [(name, segs8, w, h, R)] -> the context filled by one batch, the one filled by single calls, the keys, the rectangles (checked equal)"""
    a, b = contexts(atlas_size)
    keys = [first_key + i for i in range(len(glyphs))]
    rects = a.put_glyph_outlines_cubic([(k, segs, w, h, R) for k, (_, segs, w, h, R) in zip(keys, glyphs)], correct=correct)
    singles = [b.put_glyph_outline_cubic(k, segs, w, h, mtsdf=True, sdf_range=R, correct=correct) for k, (_, segs, w, h, R) in zip(keys, glyphs)]
    assert rects == singles
    assert a.atlas_size() == b.atlas_size()
    return a, b, keys, rects


@pytest.fixture(scope="module")
def font():
    """the 106 skewed font outlines into a 2048 atlas, once as one batch and once as 106 single calls -> (batch context, singles context, keys, inputs)"""
    inputs = CC.skewed()
    a, b, keys, _ = fill_both(inputs)
    yield a, b, keys, inputs
    a.close()
    b.close()


def test_font_set_level_0_is_the_single_calls(font):
    a, b, keys, inputs = font
    assert len(inputs) == 106 and a.atlas_size() == 2048
    atlas = same_level0(a, b, "the skewed font set")  # whole arrays: the margins and everything outside the rectangles too
    assert atlas.any()
    st = a.glyph_batch_stats()
    assert st["glyphs"] == st["written"] == 106 and st["dropped_by_growth"] == 0
    assert st["tiles"] == sum(((w + 7) // 8) * ((h + 7) // 8) for _, _, w, h, _ in inputs) and st["edges"] > 1000 and st["bytes_copied"] > st["edges"] * 144


def test_font_set_with_the_correction():
    a, b, _, _ = fill_both(CC.skewed(), correct=True)
    corrected = same_level0(a, b, "the skewed font set, corrected")
    a.close()
    b.close()
    a, b, _, _ = fill_both(CC.skewed())
    assert not np.array_equal(corrected, same_level0(a, b, "the skewed font set"))  # the correction changed texels, the same ones on both sides
    a.close()
    b.close()


@pytest.mark.parametrize("overlap", [False, True], ids=["plain", "overlap"])
def test_a_batch_without_a_cubic(overlap):
    """no cubic in any glyph: the call is fdh_put_glyph_outlines on six-float copies, FDH_GLYPH_MTSDF_OVERLAP included -- rectangles and
    level 0 equal single fdh_put_glyph_outline_cubic calls, which take that flag on a cubic-free outline"""
    import ctypes as C

    glyphs = [(name, CC.lift(segs), w, h, (1, 2, 4, 64)[i % 4]) for i, (name, segs, w, h, _) in enumerate(MC.inputs()[2::8])]
    a, b = contexts(1024)
    keys = [600 + i for i in range(len(glyphs))]
    rects = a.put_glyph_outlines_cubic([(k, segs, w, h, R) for k, (_, segs, w, h, R) in zip(keys, glyphs)], correct=True, overlap=overlap)
    singles = []
    for k, (_, segs, w, h, R) in zip(keys, glyphs):
        out = (C.c_int * 4)()
        assert b.L.fdh_put_glyph_outline_cubic(b.h, k, w, h, segs.ctypes.data, len(segs), 4 | 8 | (32 if overlap else 0) | R << 8, out) == 0
        singles.append(tuple(out))
    assert rects == singles and len(rects) == 13 and a.atlas_size() == b.atlas_size() == 1024
    assert same_level0(a, b, "a batch without a cubic").any()
    a.close()
    b.close()


def small_shapes():
    """partial tiles, thin fields, an empty edge list, a glyph whose first tile is not tile 0, neighbours of different width, kinds mixed in one
    contour and two glyphs without a cubic -> [(name, segs8, w, h, R)], ranges 2, 4, 64, 1 in turn (1 x 9 lies half a texel outside its outline: range 1 would store 0 there)"""
    hostile = {c[0]: c for c in CC.hostile()}
    named = [hostile[n][:4] for n in ("9 x 9 image", "cusp", "cubic, quadratic and lines in one contour")]
    lifted = [(name + " lifted", CC.lift(segs), w, h) for name, segs, w, h, _ in (MC.inputs()[ord("g") - 33], MC.inputs()[ord("i") - 33])]
    shapes = [c[:4] for c in DEVICE_ONLY[:3]] + [lifted[0]] + [DEVICE_ONLY[3][:4]] + named + [lifted[1]]
    return [c + ((2, 4, 64, 1)[i % 4],) for i, c in enumerate(shapes)]


@pytest.mark.parametrize("correct", [False, True], ids=["plain", "correct"])
@pytest.mark.parametrize("order", ["given", "reversed"])
def test_small_shapes(order, correct):
    glyphs = small_shapes() if order == "given" else small_shapes()[::-1]
    assert len(glyphs) == 9 and {g[4] for g in glyphs} == {1, 2, 4, 64}
    a, b, keys, rects = fill_both(glyphs, atlas_size=256, correct=correct)
    atlas = same_level0(a, b, f"small shapes {order}")
    # the 4-texel margin around each rectangle -- and everything else outside the rectangles -- is unwritten
    written = np.zeros(atlas.shape[:2], bool)
    for (name, segs, w, h, R), (x, y, rw, rh) in zip(glyphs, rects):
        assert (rw, rh) == (w, h)
        ring = atlas[max(y - 4, 0):y + h + 4, max(x - 4, 0):x + w + 4].copy()
        ring[y - max(y - 4, 0):y - max(y - 4, 0) + h, x - max(x - 4, 0):x - max(x - 4, 0) + w] = 0
        assert not ring.any(), f"{name}: the margin was written"
        written[y:y + h, x:x + w] = True
        assert atlas[y:y + h, x:x + w, 3].any() == (len(segs) > 0), name  # a field 1 texel wide or high has its level 0; no edges: all zero
    assert not atlas[~written].any()
    a.close()
    b.close()


def test_the_analytic_circle_from_a_batch():
    """the existing bound of test_msdf_cubic.py::test_the_analytic_circle: alpha within one quantisation step plus 0.003 texel of r - |p - c|"""
    from figdraw_amd.context import HipContext

    name, segs, w, h, Rr, exact = CC.analytic()[0]
    ctx = HipContext(atlas_size=256, device=0)
    rects = ctx.put_glyph_outlines_cubic([(1, BOX, 12, 11), (2, segs, w, h, Rr), (3, SQUARE, 12, 11)])
    x, y, _, _ = rects[1]
    got = ctx.debug_read_surface(4)[y:y + h, x:x + w]
    ctx.close()
    ys, xs = np.mgrid[0:h, 0:w]
    want = np.clip(exact(xs + 0.5, ys + 0.5), -Rr / 2, Rr / 2)
    err = np.abs(M.decode(got[..., 3], Rr) - want).max()
    print(f"{name}: max |alpha - (r - |p - c|)| = {err:.5f} texels")
    assert err <= Rr / 255.0 + 0.003


def test_a_batch_of_one_is_the_single_call_on_every_level():
    name, segs, w, h, R = CC.skewed()[40]
    for correct in (False, True):
        a, b, keys, _ = fill_both([(name, segs, w, h, R)], atlas_size=256, correct=correct)
        same_level0(a, b, name)
        assert a.glyph_batch_stats()["glyphs"] == 1
        scales = (1.0, 0.25, 1 / 16.0, 1 / 32.0)
        fa, fb = _minified_frame(a, keys, [(w, h)], scales), _minified_frame(b, keys, [(w, h)], scales)
        assert np.array_equal(fa, fb) and len(np.unique(fa.reshape(-1, 4), axis=0)) > 8
        a.close()
        b.close()


def test_the_level_chain(font):
    """the font-set batch drawn at 1/2, 1/4 and 1/8 size and, for the levels in which neighbours' rectangles meet (the owner bits), at 1/16 and 1/32"""
    a, b, keys, inputs = font
    every = [c[2:4] for c in inputs]
    for scales, n in (((0.5, 0.25, 0.125), 12), ((1 / 16.0, 1 / 32.0), 106)):
        step = 106 // n
        fa, fb = _minified_frame(a, keys[::step][:n], every[::step][:n], scales), _minified_frame(b, keys[::step][:n], every[::step][:n], scales)
        assert np.array_equal(fa, fb), f"scales {scales}: {int((fa != fb).any(axis=2).sum())} pixels differ"
        assert len(np.unique(fa.reshape(-1, 4), axis=0)) > 8


def test_growth_on_the_device():
    """atlas size 64 and twelve 40 x 40 outlines, cubic and cubic-free in turn: the atlas grows more than once inside the batch"""
    plain = CC.lift(MC.poly([(10, 10), (30, 10), (30, 30), (10, 30)]))
    glyphs = [(f"glyph {i}", cubic_square(40, 40) if i % 2 == 0 else plain, 40, 40, 4) for i in range(12)]
    a, b, keys, _ = fill_both(glyphs, atlas_size=64, correct=True)
    assert a.atlas_size() > 64
    assert [a.has_image(k) for k in keys] == [b.has_image(k) for k in keys] and not all(b.has_image(k) for k in keys) and b.has_image(keys[-1])
    assert same_level0(a, b, "growth").any()
    st = a.glyph_batch_stats()
    assert st["dropped_by_growth"] == sum(not b.has_image(k) for k in keys) > 0 and st["written"] == 12 - st["dropped_by_growth"]
    a.close()
    b.close()


def test_a_refused_batch_leaves_the_device_untouched():
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    ctx.put_glyph_outlines_cubic([(1, cubic_square(40, 40), 40, 40), (2, BOX, 12, 11)])
    before = ctx.debug_read_surface(4)
    with pytest.raises(FigdrawHipError) as e:
        ctx.put_glyph_outlines_cubic([(10, BOX, 12, 11), (11, SQUARE, 12, 11), (12, BOX[:3], 12, 11)])  # a bad last glyph
    assert e.value.code == INVALID
    assert [ctx.has_image(k) for k in (1, 2, 10, 11, 12)] == [True, True, False, False, False]
    assert np.array_equal(ctx.debug_read_surface(4), before) and before.any()
    assert ctx.glyph_batch_stats()["glyphs"] == 2
    ctx.close()


def test_atlas_full_part_way_through():
    """the largest atlas with nine 4096 x 4096 rectangles in it: the batch's third glyph finds no place; the two before it are in the atlas with
    their texels (drawn 1:1 at integer positions on black the frame shows level 0 itself: compared with single calls into a small atlas),
    the one behind it is not"""
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = full_atlas(device=0)
    with pytest.raises(FigdrawHipError) as e:
        ctx.put_glyph_outlines_cubic(FULL_BATCH, correct=True)
    assert e.value.code == ATLAS_FULL and ctx.atlas_size() == 16384
    assert [ctx.has_image(g[0]) for g in FULL_BATCH] == [True, True, False, False]
    st = ctx.glyph_batch_stats()
    assert st["glyphs"] == 4 and st["written"] == 2 and st["dropped_by_growth"] == 0 and st["launches"] > 0
    small = HipContext(atlas_size=64, device=0)
    for k, segs, w, h in FULL_BATCH[:2]:
        small.put_glyph_outline_cubic(k, segs, w, h, mtsdf=True, correct=True)
    frames = []
    for c in (ctx, small):
        c.begin_frame(64, 32, True, (0, 0, 0, 1))
        c.draw_image(10, (2, 3), WHITE)
        c.draw_image(11, (30, 5), WHITE)
        c.end_frame()
        frames.append(c.read_pixels())
    assert frames[0][..., :3].max() > 200 and np.array_equal(frames[0], frames[1])
    small.close()
    ctx.close()


@pytest.mark.parametrize("correct", [False, True], ids=["plain", "correct"])
def test_launch_count_does_not_depend_on_the_number_of_glyphs(correct):
    from figdraw_amd.context import HipContext

    inputs = CC.skewed()
    three, all_ = HipContext(atlas_size=2048, device=0), HipContext(atlas_size=2048, device=0)
    three.put_glyph_outlines_cubic([(1, BOX, 12, 11), (2, SQUARE, 12, 11), (3, cubic_square(40, 40), 40, 40)], correct=correct)
    all_.put_glyph_outlines_cubic([(5000 + i, segs, w, h, R) for i, (_, segs, w, h, R) in enumerate(inputs)], correct=correct)
    n3, n106 = three.glyph_batch_stats()["launches"], all_.glyph_batch_stats()["launches"]
    assert n3 == n106 == 1 + (1 if correct else 0) + 2 * LEVELS_2048 - 1
    three.close()
    all_.close()


def test_a_batch_put_while_a_frame_is_in_flight():
    """the call synchronises like every atlas put: the frame in flight keeps its pixels, whether the put was a cubic batch or a plain image"""
    import os

    from conftest import GOLDEN
    from figdraw_amd.context import HipContext

    z = np.load(os.path.join(GOLDEN, "outlines_ubuntu20.npz"))
    W, H = 640, 96
    codes = list(range(65, 85))
    frames = []
    for batch in (True, False):
        ctx = HipContext(atlas_size=512, device=0)
        for code in codes:
            ctx.put_glyph_outline(7000 + code, z[f"segs_{code}"], *(int(v) for v in z[f"size_{code}"]))
        ctx.begin_frame(W, H, True, (0.0, 0.0, 0.0, 1.0))
        x = 3
        for code in codes:
            ctx.draw_image(7000 + code, (float(x), 5.0), [(255, 255, 255, 255)] * 4)
            x += int(z[f"size_{code}"][0]) + 2
        ctx.end_frame()  # in flight: nothing has waited for it yet
        if batch:
            ctx.put_glyph_outlines_cubic([(9000 + i, segs, w, h, R) for i, (_, segs, w, h, R) in enumerate(CC.skewed()[60:72])], correct=True)
            assert ctx.atlas_size() == 512
        else:
            ctx.put_image(9000, np.full((40, 30, 4), 77, np.uint8))
        frames.append(ctx.read_pixels())
        ctx.close()
    assert frames[0].max() == 255 and np.array_equal(frames[0], frames[1])


def test_the_four_batch_calls_on_one_context():
    """both new calls and both old batch calls in turn: level 0 is what the single calls in the same order leave, and each stats call
    reports the last batch of its kind in either segment format"""
    a, b = contexts(1024)
    cubic = [(100 + i, segs, w, h) for i, (_, segs, w, h, _) in enumerate(CC.skewed()[10:22])]
    six = [(200 + i, segs, w, h) for i, (_, segs, w, h, _) in enumerate(MC.inputs()[30:40])]
    re_key = lambda items, d: [(g[0] + d,) + tuple(g[1:]) for g in items]  # noqa: E731
    ra = [a.put_glyph_outlines_cubic(cubic, correct=True), a.put_glyph_coverage_batch(re_key(six, 1000), lcd_filter=True),
          a.put_glyph_coverage_batch_cubic(re_key(cubic, 2000)), a.put_glyph_outlines(re_key(six, 3000), sdf_range=2)]
    assert a.glyph_batch_stats()["glyphs"] == len(six) and a.glyph_coverage_batch_stats()["glyphs"] == len(cubic)
    assert a.glyph_batch_stats()["launches"] == 1 + 2 * 11 - 1 and a.glyph_coverage_batch_stats()["launches"] == 2 + 2 * 11 - 1  # a 1024 atlas: 11 levels
    rb = [[b.put_glyph_outline_cubic(k, s, w, h, mtsdf=True, correct=True) for k, s, w, h in cubic],
          [b.put_glyph_outline(k, s, w, h, lcd_filter=True) for k, s, w, h in re_key(six, 1000)],
          [b.put_glyph_outline_cubic(k, s, w, h) for k, s, w, h in re_key(cubic, 2000)],
          [b.put_glyph_outline(k, s, w, h, mtsdf=True, sdf_range=2) for k, s, w, h in re_key(six, 3000)]]
    assert ra == rb and a.atlas_size() == b.atlas_size() == 1024
    assert same_level0(a, b, "four batch calls in turn").any()
    # and the cubic batches after the six-float ones
    assert a.put_glyph_coverage_batch_cubic(re_key(cubic, 4000), lcd_filter=True) == [b.put_glyph_outline_cubic(k, s, w, h, lcd_filter=True) for k, s, w, h in re_key(cubic, 4000)]
    assert a.put_glyph_outlines_cubic(re_key(cubic, 5000), sdf_range=8) == [b.put_glyph_outline_cubic(k, s, w, h, mtsdf=True, sdf_range=8) for k, s, w, h in re_key(cubic, 5000)]
    assert a.glyph_batch_stats()["glyphs"] == len(cubic) and a.glyph_coverage_batch_stats()["glyphs"] == len(cubic) and a.atlas_size() == b.atlas_size()
    same_level0(a, b, "and the cubic batches again")
    a.close()
    b.close()
