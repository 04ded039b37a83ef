"""Distance-field generation on the device (fdh_put_glyph_outline with FDH_GLYPH_MTSDF, k_msdf_generate): the texels against the float64
reference tests/msdf_ref.py -- the font set and the hostile outlines of msdf_cases.hostile_inputs() --, rendering with those texels against
the oracle, and the atlas's other users undisturbed."""
import math

import numpy as np
import pytest

import msdf_cases as MC
import msdf_ref as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def generated():
    """every input through the flagged call into a 2048 atlas -> {name: (rect, texels)}, and level 0 itself"""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=2048, device=0)
    rects = {}
    for i, (name, segs, w, h, R) in enumerate(MC.inputs()):
        rects[name] = ctx.put_glyph_outline(5000 + i, segs, w, h, mtsdf=True, sdf_range=R)
        assert rects[name][2:] == (w, h)
    assert ctx.atlas_size() == 2048
    atlas = ctx.debug_read_surface(4)
    ctx.close()
    assert atlas.shape == (2048, 2048, 4)
    return {name: (r, atlas[r[1]:r[1] + r[3], r[0]:r[0] + r[2]].copy()) for name, r in rects.items()}, atlas


def test_texels_against_the_reference(generated):
    texels, atlas = generated
    over = {}
    written = np.zeros(atlas.shape[:2], bool)
    for name, segs, w, h, R in MC.inputs():
        (x, y, _, _), got = texels[name]
        n = MC.over_tolerance(got, M.generate(segs, w, h, R))
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels are more than 1 LSB from the reference"
        written[y:y + h, x:x + w] = True
    print(f"texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}")
    # the 4-texel margin around each rectangle -- and everything else outside the rectangles -- is unwritten
    for name, ((x, y, w, h), _) in texels.items():
        ring = atlas[max(y - 4, 0):y + h + 4, max(x - 4, 0):x + w + 4].copy()
        ring[y - max(y - 4, 0):y - max(y - 4, 0) + h, x - max(x - 4, 0):x - max(x - 4, 0) + w] = 0
        assert not ring.any(), f"{name}: the margin was written"
    assert not atlas[~written].any()


def test_sign_of_the_device_texels(generated):
    texels, _ = generated
    for name, segs, w, h, R in MC.inputs():
        MC.check_sign(name, texels[name][1], segs, w, h, R)


SQUARE = MC.poly([(2, 2), (10, 2), (10, 9), (2, 9)])  # in 12 x 11, as on the record-only context (test_msdf_host.py)
DEVICE_ONLY = [("16383 copies of one square", np.tile(SQUARE, (16383, 1)), 12, 11, 4),  # 65532 segments: the most whole squares the call accepts
               ("0 segments", np.zeros((0, 6), np.float32), 12, 11, 4)]


@pytest.fixture(scope="module")
def hostile():
    """every hostile input and the two device-only ones through the flagged call into one 2048 atlas ->
    {name: (rect, texels, the reference's texels, its true distances or None)}, and level 0 itself.  The reference runs once per input, here."""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=2048, device=0)
    rects = {}
    for i, (name, segs, w, h, R) in enumerate([c[:5] for c in MC.hostile_inputs()] + DEVICE_ONLY):
        rects[name] = ctx.put_glyph_outline(8000 + i, segs, w, h, mtsdf=True, sdf_range=R)
        assert rects[name][2:] == (w, h)
    assert ctx.atlas_size() == 2048
    atlas = ctx.debug_read_surface(4)
    ctx.close()
    assert atlas.shape == (2048, 2048, 4)
    want = {}
    for name, segs, w, h, R, _ in MC.hostile_inputs():
        d = M.distances(M.build_shape(segs), w, h)
        want[name] = (M.encode(d, R), d[..., 3])
    # duplicates change no texel ("a square twice" among the hostile inputs shows it): 65532 edges are not fed to numpy
    want[DEVICE_ONLY[0][0]] = (M.generate(SQUARE, 12, 11, 4), None)
    want[DEVICE_ONLY[1][0]] = (M.generate(DEVICE_ONLY[1][1], 12, 11, 4), None)
    return {name: (r, atlas[r[1]:r[1] + r[3], r[0]:r[0] + r[2]].copy()) + want[name] for name, r in rects.items()}, atlas


def test_hostile_texels_against_the_reference(hostile):
    texels, atlas = hostile
    over = {}
    written = np.zeros(atlas.shape[:2], bool)
    assert len(texels) == len(MC.hostile_inputs()) + 2
    for name, ((x, y, w, h), got, want, _) in texels.items():
        n = MC.over_tolerance(got, want)
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels are more than 1 LSB from the reference"
        written[y:y + h, x:x + w] = True
    print(f"texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}")
    assert not texels["0 segments"][1].any() and not texels["0 segments"][2].any()  # what the header promises for an outline without edges
    assert not texels["one edge doubling back on itself"][1].any()
    for name, ((x, y, w, h), _, _, _) in texels.items():
        ring = atlas[max(y - 4, 0):y + h + 4, max(x - 4, 0):x + w + 4].copy()
        ring[y - max(y - 4, 0):y - max(y - 4, 0) + h, x - max(x - 4, 0):x - max(x - 4, 0) + w] = 0
        assert not ring.any(), f"{name}: the margin was written"
    assert not atlas[~written].any()


def test_hostile_sign_of_the_device_texels(hostile):
    texels, _ = hostile
    for name, segs, w, h, R, simple in MC.hostile_inputs():
        if simple:
            assert MC.check_sign(name, texels[name][1], segs, w, h, R, texels[name][3]) > 0
    name, _, w, h, R = DEVICE_ONLY[0]
    MC.check_sign(name, texels[name][1], SQUARE, w, h, R)


def _scene(ctx, keys, sizes):
    """a few dozen fields at scales 0.75, 1, 2.5 and under a 7 degree rotation, the four modes, flip_y"""
    W, H = 1280, 900
    ctx.begin_frame(W, H, True, (0.92, 0.94, 0.98, 1.0))
    y = 6.0
    i = 0
    for scale in (0.75, 1.0, 2.5):
        x, row_h = 6.0, 0.0
        for k in range(9 if scale > 2 else 14):
            key = keys[i % len(keys)]
            w, h = sizes[key]
            mtsdf, stroke, flip = bool(i & 1), 1.5 if i & 2 else 0.0, i % 5 == 4
            ctx.draw_msdf(key, (x + 0.25 * (k % 3), y + 0.5 * (k % 2)), (20 + 15 * k, 40, 200 - 12 * k, 255 - 9 * (k % 4)), (w * scale, h * scale), 4.0, 0.5, stroke, mtsdf, flip)
            x += w * scale + 5.0
            row_h = max(row_h, h * scale)
            i += 1
        y += row_h + 6.0
    ctx.save_transform()
    ctx.translate(40.0, y + 20.0)
    ctx.rotate(math.radians(7.0))
    x = 0.0
    for k in range(12):
        key = keys[i % len(keys)]
        w, h = sizes[key]
        ctx.draw_msdf(key, (x, 0.0), (200, 30 + 15 * k, 40, 255), (w * 1.6, h * 1.6), 4.0, 0.5, 1.5 if k & 2 else 0.0, bool(k & 1), k % 4 == 3)
        x += w * 1.6 + 6.0
        i += 1
    ctx.restore_transform()
    ctx.end_frame()
    return ctx.read_pixels()


def test_rendering_with_the_generated_texels(generated):
    """the first fields with sharp corners and disagreeing channels to reach the compositor's median path: HIP and oracle, both holding the
    texels the device generated, agree within the suite's bar of 1 LSB"""
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    texels, _ = generated
    cases = [c for c in MC.inputs() if c[4] == 4][3::3][:30]
    ctx, orc = HipContext(atlas_size=2048, device=0), O.Oracle(atlas_size=2048, threads=8)
    keys, sizes = [], {}
    for i, (name, segs, w, h, R) in enumerate(cases):
        assert ctx.put_glyph_outline(6000 + i, segs, w, h, mtsdf=True, sdf_range=R) == orc.put_image(6000 + i, texels[name][1])
        keys.append(6000 + i)
        sizes[6000 + i] = (w, h)
    got, want = _scene(ctx, keys, sizes), _scene(orc, keys, sizes)
    ctx.close()
    d = np.abs(got.astype(int) - want.astype(int))
    assert (want != want[0, 0]).any(axis=2).sum() > 20000  # something was drawn
    print(f"max |hip - oracle| = {d.max()} LSB on {int((d > 0).any(axis=2).sum())} pixels")
    assert d.max() <= 1


def test_the_atlas_other_users_are_undisturbed():
    """Coverage glyphs put before and after a distance-field put render bit-identically to a context that never saw the flag (it puts a
    plain image of the same size instead, so that both atlases pack alike), and a frame in flight while the field is generated is
    unharmed: the call synchronises, like every atlas put."""
    import os

    from conftest import GOLDEN
    from figdraw_amd.context import HipContext

    z = np.load(os.path.join(GOLDEN, "outlines_ubuntu20.npz"))
    name, fsegs, fw, fh, R = MC.inputs()[ord("g") - 33]
    W, H = 640, 96

    def frame(ctx, codes):
        ctx.begin_frame(W, H, True, (0.0, 0.0, 0.0, 1.0))
        x = 3
        for code in codes:
            gw, gh = (int(v) for v in z[f"size_{code}"])
            ctx.draw_image(7000 + code, (float(x), 5.0), [(255, 255, 255, 255)] * 4)
            x += gw + 2
        ctx.end_frame()

    before, after = list(range(65, 85)), list(range(97, 117))
    frames = []
    for flagged in (True, False):
        ctx = HipContext(atlas_size=512, device=0)
        for code in before:
            ctx.put_glyph_outline(7000 + code, z[f"segs_{code}"], *(int(v) for v in z[f"size_{code}"]))
        frame(ctx, before)  # in flight: nothing has waited for it yet
        if flagged:
            ctx.put_glyph_outline(9000, fsegs, fw, fh, mtsdf=True, sdf_range=R)
        else:
            ctx.put_image(9000, np.full((fh, fw, 4), 77, np.uint8))
        first = ctx.read_pixels()
        for code in after:
            ctx.put_glyph_outline(7000 + code, z[f"segs_{code}"], *(int(v) for v in z[f"size_{code}"]))
        frame(ctx, before[::2] + after)
        frames.append((first, ctx.read_pixels()))
        ctx.close()
    assert frames[0][0].max() == 255 and frames[0][1].max() == 255
    assert np.array_equal(frames[0][0], frames[1][0]), "the frame in flight"
    assert np.array_equal(frames[0][1], frames[1][1]), "coverage glyphs before and after"
