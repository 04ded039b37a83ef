"""Glyph outlines with cubic segments on the device (fdh_put_glyph_outline_cubic; k_msdf_generate_cubic, k_msdf_correct_cubic): the texels
against the float64 reference tests/msdf_cubic_ref.py -- the skewed font set, the hostile outlines and the analytic shapes of
msdf_cubic_cases.py --, the coverage path against the oracle, rendering with the generated texels, and the atlas's other users undisturbed."""
import numpy as np
import pytest

import msdf_cases as MC
import msdf_cubic_cases as CC
import msdf_cubic_ref as R
import msdf_ref as M

pytestmark = pytest.mark.gpu
CORRECT_CAP = 1  # test_msdf_correct.py's: a verdict may flip where |d(q)| is within rounding of R / 255

SMALL = CC.cpath((1, 1), (5, -2, 10, 4, 8, 8), (1, 8), (1, 1))
DEVICE_ONLY = [("1 x 9", SMALL, 1, 9, 2), ("9 x 1", SMALL, 9, 1, 2), ("17 x 9", SMALL, 17, 9, 2), ("0 segments", np.zeros((0, 8), np.float32), 12, 11, 4)]


def all_inputs():
    return CC.skewed() + [c[:5] for c in CC.hostile()] + [c[:5] for c in CC.analytic()] + DEVICE_ONLY


def _cut(atlas, r):
    return atlas[r[1]:r[1] + r[3], r[0]:r[0] + r[2]].copy()


@pytest.fixture(scope="module")
def generated():
    """every input through the call, plain into one 2048 atlas and with FDH_GLYPH_MTSDF_CORRECT into another ->
    {name: (rect, texels, corrected texels)}, and level 0 of the first atlas"""
    from figdraw_amd.context import HipContext

    atlases, rects = [], []
    for correct in (False, True):
        ctx = HipContext(atlas_size=2048, device=0)
        rs = {}
        for i, (name, segs, w, h, Rr) in enumerate(all_inputs()):
            rs[name] = ctx.put_glyph_outline_cubic(5000 + i, segs, w, h, mtsdf=True, sdf_range=Rr, correct=correct)
            assert rs[name][2:] == (w, h)
        assert ctx.atlas_size() == 2048
        atlases.append(ctx.debug_read_surface(4))
        rects.append(rs)
        ctx.close()
    assert rects[0] == rects[1]
    return {name: (r, _cut(atlases[0], r), _cut(atlases[1], r)) for name, r in rects[0].items()}, atlases[0]


@pytest.fixture(scope="module")
def reference():
    """the float64 reference, once per input -> {name: (true distances, texels)}"""
    out = {}
    for name, segs, w, h, Rr in all_inputs():
        d = R.distances(R.build_shape(segs), w, h)
        out[name] = (d[..., 3], M.encode(d, Rr))
    return out


def test_texels_against_the_reference(generated, reference):
    texels, atlas = generated
    over = {}
    written = np.zeros(atlas.shape[:2], bool)
    for name, segs, w, h, Rr in all_inputs():
        (x, y, _, _), got, _ = texels[name]
        n = MC.over_tolerance(got, reference[name][1])
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels are more than 1 LSB from the reference"
        written[y:y + h, x:x + w] = True
    print(f"texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}")
    # the 4-texel margin around each rectangle -- and everything else outside the rectangles -- is unwritten
    for name, ((x, y, w, h), _, _) in texels.items():
        ring = atlas[max(y - 4, 0):y + h + 4, max(x - 4, 0):x + w + 4].copy()
        ring[y - max(y - 4, 0):y - max(y - 4, 0) + h, x - max(x - 4, 0):x - max(x - 4, 0) + w] = 0
        assert not ring.any(), f"{name}: the margin was written"
    assert not atlas[~written].any()
    assert not texels["0 segments"][1].any() and not texels["0 segments"][2].any()  # an outline without edges: an all-zero image
    assert texels["1 x 9"][1].any() and texels["9 x 1"][1].any()                    # a field 1 texel wide or high gets level 0


def test_corrected_texels_against_the_reference(generated):
    """FDH_GLYPH_MTSDF_CORRECT: the reference's step 5 of the device's own uncorrected field, and step 5's invariants exactly"""
    texels, _ = generated
    over, changed = {}, 0
    for name, segs, w, h, Rr in all_inputs():
        _, F, G = texels[name]
        want, _, _ = R.correct(F, segs, Rr)
        n = int((G != want).any(axis=2).sum())
        if n:
            over[name] = n
        assert n <= CORRECT_CAP, f"{name}: {n} texels differ from the reference's correction of the same field"
        assert np.array_equal(G[..., 3], F[..., 3]) and np.array_equal(MC.median3(G), MC.median3(F)), f"{name}: alpha or a median moved"
        changed += int((G != F).any(axis=2).sum())
    print(f"texels that differ from correct(F_device) per image (cap {CORRECT_CAP}): {over or 'none in any image'}; {changed} texels corrected")
    assert changed > 0


def test_sign_of_the_device_texels(generated, reference):
    texels, _ = generated
    simple = {c[0]: c[5] for c in CC.hostile()}
    checked = 0
    for name, segs, w, h, Rr in all_inputs():
        if simple.get(name, True) and len(segs):
            checked += MC.check_sign(name, texels[name][1], None, w, h, Rr, reference[name][0], MC.winding(R.flatten(segs), w, h) != 0)
    assert checked > 100000


def test_the_analytic_circle(generated):
    name, segs, w, h, Rr, exact = CC.analytic()[0]
    ys, xs = np.mgrid[0:h, 0:w]
    want = np.clip(exact(xs + 0.5, ys + 0.5), -Rr / 2, Rr / 2)
    err = np.abs(M.decode(generated[0][name][1][..., 3], Rr) - want).max()
    print(f"{name}: max |alpha - (r - |p - c|)| = {err:.5f} texels")
    assert err <= Rr / 255.0 + 0.003


def test_a_cubic_free_outline_is_the_old_call():
    """byte-equal level 0, distance fields (plain, corrected, overlapping contours) and coverage (plain and filtered)"""
    from figdraw_amd.context import HipContext

    cases = [c for c in MC.inputs()[5::12]]
    two = np.concatenate([MC.poly([(4, 4), (16, 4), (16, 16), (4, 16)]), MC.poly([(10, 10), (24, 10), (24, 22), (10, 22)])])
    levels = []
    for cubic in (False, True):
        ctx = HipContext(atlas_size=1024, device=0)
        put = (lambda k, s, *a, **kw: ctx.put_glyph_outline_cubic(k, CC.lift(s), *a, **kw)) if cubic else ctx.put_glyph_outline
        rects = []
        for i, (name, segs, w, h, Rr) in enumerate(cases):
            rects.append(put(100 + i, segs, w, h, mtsdf=True, sdf_range=Rr, correct=bool(i & 1)))
            rects.append(put(200 + i, segs, w, h, lcd_filter=bool(i & 1)))
        if cubic:  # (the Python wrapper of the new call has no overlap argument: the flag goes through the C call)
            import ctypes as C
            out, s8 = (C.c_int * 4)(), CC.lift(two)
            assert ctx.L.fdh_put_glyph_outline_cubic(ctx.h, 300, 28, 26, s8.ctypes.data, len(s8), 4 | 32, out) == 0
            rects.append(tuple(out))
        else:
            rects.append(ctx.put_glyph_outline(300, two, 28, 26, mtsdf=True, overlap=True))
        levels.append((rects, ctx.debug_read_surface(4)))
        ctx.close()
    assert levels[0][0] == levels[1][0] and levels[0][1].any()
    assert np.array_equal(levels[0][1], levels[1][1])


@pytest.mark.parametrize("lcd", [False, True, "context"])
def test_coverage_of_a_skewed_glyph_matches_the_oracle(lcd):
    """the coverage path: the host's lines (msdf_cubic_cases.flatten_lines restates them; test_msdf_cubic_host.py holds the two together)
    through the oracle's rasteriser and filter, pasted at the rectangle"""
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    ctx = HipContext(atlas_size=256, device=0)
    ctx.set_text_lcd_filtering(True)
    want = np.zeros((256, 256, 4), np.uint8)
    for i, ch in enumerate("g&R"):
        name, segs, w, h, _ = CC.skewed()[ord(ch) - 33]
        x, y, rw, rh = ctx.put_glyph_outline_cubic(10 + i, segs, w, h, lcd_filter=lcd)
        assert (rw, rh) == (w, h)
        img = O.rasterize_outline(CC.lines_as_outline(CC.flatten_lines(segs)), w, h)
        want[y:y + h, x:x + w] = O.lcd_filter(img) if lcd else img
    got = ctx.debug_read_surface(4)
    ctx.close()
    assert want[..., 3].max() == 255 and np.array_equal(got, want)


def test_drawing_a_skewed_glyph(generated):
    """fdh_draw_msdf at 3 : 1 of a field made from cubics, against the oracle drawing the device's texels: within 1 LSB"""
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    name, segs, w, h, Rr = CC.skewed()[ord("g") - 33]
    ctx, orc = HipContext(atlas_size=256, device=0), O.Oracle(atlas_size=256, threads=4)
    assert ctx.put_glyph_outline_cubic(1, segs, w, h, mtsdf=True, sdf_range=Rr) == orc.put_image(1, generated[0][name][1])
    frames = []
    for c in (ctx, orc):
        c.begin_frame(3 * w + 8, 3 * h + 8, True, (0.92, 0.94, 0.98, 1.0))
        c.draw_msdf(1, (4.0, 4.0), (20, 40, 200, 255), (3.0 * w, 3.0 * h), 4.0, 0.5, 0.0, True, False)
        c.end_frame()
        frames.append(c.read_pixels())
    ctx.close()
    d = np.abs(frames[0].astype(int) - frames[1].astype(int))
    assert (frames[1] != frames[1][0, 0]).any(axis=2).sum() > 500  # something was drawn
    print(f"max |hip - oracle| = {d.max()} LSB")
    assert d.max() <= 1


def test_a_put_while_a_frame_is_in_flight():
    """the call synchronises like every atlas put: the frame in flight keeps its pixels, whether the put made a cubic field or a plain image"""
    import os

    from conftest import GOLDEN
    from figdraw_amd.context import HipContext

    z = np.load(os.path.join(GOLDEN, "outlines_ubuntu20.npz"))
    name, fsegs, fw, fh, Rr = CC.skewed()[ord("g") - 33]
    W, H = 640, 96
    codes = list(range(65, 85))
    frames = []
    for cubic in (True, False):
        ctx = HipContext(atlas_size=512, device=0)
        for code in codes:
            ctx.put_glyph_outline(7000 + code, z[f"segs_{code}"], *(int(v) for v in z[f"size_{code}"]))
        ctx.begin_frame(W, H, True, (0.0, 0.0, 0.0, 1.0))
        x = 3
        for code in codes:
            ctx.draw_image(7000 + code, (float(x), 5.0), [(255, 255, 255, 255)] * 4)
            x += int(z[f"size_{code}"][0]) + 2
        ctx.end_frame()  # in flight: nothing has waited for it yet
        if cubic:
            ctx.put_glyph_outline_cubic(9000, fsegs, fw, fh, mtsdf=True, sdf_range=Rr, correct=True)
        else:
            ctx.put_image(9000, np.full((fh, fw, 4), 77, np.uint8))
        frames.append(ctx.read_pixels())
        ctx.close()
    assert frames[0].max() == 255 and np.array_equal(frames[0], frames[1])
