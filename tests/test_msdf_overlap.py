"""Overlapping contours on the device (fdh_put_glyph_outline with FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_OVERLAP: k_msdf_generate_union,
k_msdf_correct_union): the texels, read back through fdh_debug_read_surface(ctx, 4), against the float64 reference
tests/msdf_overlap_ref.py; what the flag leaves alone; and the hole that a composite glyph no longer has when it is drawn."""
import numpy as np
import pytest

import msdf_cases as MC
import msdf_overlap_cases as OC
import msdf_overlap_ref as OR
import msdf_ref as M

pytestmark = pytest.mark.gpu

SQUARE = MC.poly([(2, 2), (10, 2), (10, 9), (2, 9)])  # in 12 x 11, as in test_msdf.py
LENS = np.array([[4, 12, 14, 0, 24, 12], [24, 12, 14, 24, 4, 12]], np.float32)
SINGLE = [("a square", SQUARE, 12, 11), ("the lens", LENS, 28, 24), ("circle16", MC.circle16(), 28, 24)]
ROW = OC.join(MC.poly([(1, -3), (8, 0.5), (2, 4)]), OC.rect(0.25, -1, 4.25, 2))  # two overlapping contours across a 9 x 1 image
RING_BAR = "ring plus horizontal bar through the hole"
GLYPH = MC.inputs()[ord("g") - 33]  # a plain-mode put before and after the others


@pytest.fixture(scope="module")
def device():
    """every put of this file into one 512 atlas -> {key: (rect, texels)}, and level 0 itself"""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=512, device=0)
    rects = {}

    def put(key, segs, w, h, R=4, **kw):
        rects[key] = ctx.put_glyph_outline(100 + len(rects), segs, w, h, mtsdf=True, sdf_range=R, **kw)
        assert rects[key][2:] == (w, h)

    put("plain before", GLYPH[1], GLYPH[2], GLYPH[3], GLYPH[4])
    for name, segs, w, h in OC.inputs() + OC.tie_inputs():
        put(name, segs, w, h, overlap=True)
    for name, segs, w, h in SINGLE:
        put(name + ", plain", segs, w, h)
        put(name + ", overlap", segs, w, h, overlap=True)
    put("9 x 1", ROW, 9, 1, 2, overlap=True)
    put("0 segments", np.zeros((0, 6), np.float32), 12, 11, overlap=True)
    put("16383 squares", np.tile(SQUARE, (16383, 1)), 16, 16, overlap=True)
    put("one square", SQUARE, 16, 16)
    put("corrected", [c for c in OC.inputs() if c[0] == RING_BAR][0][1], 32, 32, correct=True, overlap=True)
    put("plain after", GLYPH[1], GLYPH[2], GLYPH[3], GLYPH[4])
    assert ctx.atlas_size() == 512
    atlas = ctx.debug_read_surface(4)
    ctx.close()
    assert atlas.shape == (512, 512, 4)
    return {key: (r, atlas[r[1]:r[1] + r[3], r[0]:r[0] + r[2]].copy()) for key, r in rects.items()}, atlas


@pytest.fixture(scope="module")
def reference():
    """the 16 outlines through the float64 reference, once -> {name: (distances, winding != 0)}"""
    return {name: (OR.distances(segs, w, h), MC.winding(segs, w, h) != 0) for name, segs, w, h in OC.inputs()}


def test_texels_against_the_reference(device, reference):
    """the 16 outlines at R = 4 (a 28 x 26 image and five nested squares with a hole among them), the two outlines with ties below the first
    rank under a hole (msdf_overlap_cases.tie_inputs), and two overlapping contours in 9 x 1"""
    texels, _ = device
    over = {}
    for name, segs, w, h in OC.inputs() + OC.tie_inputs() + [("9 x 1", ROW, 9, 1)]:
        want = M.encode(reference[name][0], 4) if name in reference else OR.generate(segs, w, h, 2 if name == "9 x 1" else 4)
        n = MC.over_tolerance(texels[name][1], want)
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels are more than 1 LSB from the reference"
    print(f"texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}")
    assert (28, 26) in [(w, h) for _, _, w, h in OC.inputs()] and "five nested squares plus one hole" in reference


def test_sign_of_the_device_texels(device, reference):
    texels, _ = device
    for name, segs, w, h in OC.inputs():
        d, inside = reference[name]
        assert OC.check_sign(name, texels[name][1], segs, w, h, 4, d[..., 3], inside) > 0.6 * w * h


def test_single_contours_are_byte_identical_with_and_without_the_flag(device):
    texels, _ = device
    for name, segs, w, h in SINGLE:
        assert np.array_equal(texels[name + ", overlap"][1], texels[name + ", plain"][1]), name
        assert MC.over_tolerance(texels[name + ", overlap"][1], M.generate(segs, w, h, 4)) <= MC.CAP


def test_no_segments_and_16383_contours(device):
    texels, _ = device
    assert not texels["0 segments"][1].any()
    assert np.array_equal(texels["16383 squares"][1], texels["one square"][1])  # as many filled contours with equal A: the first one's texels
    assert MC.over_tolerance(texels["16383 squares"][1], M.generate(SQUARE, 16, 16, 4)) <= MC.CAP


def test_the_correction_with_both_flags(device, reference):
    """MTSDF | CORRECT | OVERLAP on ring plus bar: step 5 on the device's own uncorrected field, verdict distance of step 6; its invariants exactly"""
    texels, _ = device
    name, segs, w, h = [c for c in OC.inputs() if c[0] == RING_BAR][0]
    F, G = texels[name][1], texels["corrected"][1]
    want, marked, _ = OR.correct(F, segs, 4)
    assert int((G != want).any(axis=2).sum()) <= 1  # step 5's cap: a verdict within rounding of R / 255
    assert np.array_equal(G[..., 3], F[..., 3]) and np.array_equal(MC.median3(G), MC.median3(F))
    changed = (G != F).any(axis=2)
    assert int((changed != marked).sum()) <= 1
    gm = G[changed]
    assert (gm[:, 0] == gm[:, 1]).all() and (gm[:, 1] == gm[:, 2]).all()
    print(f"{int(changed.sum())} texels corrected, {int(marked.sum())} marked by the reference")


def test_margins_and_the_plain_mode_around(device):
    texels, atlas = device
    written = np.zeros(atlas.shape[:2], bool)
    for name, ((x, y, w, h), _) in texels.items():
        ring = atlas[max(y - 4, 0):y + h + 4, max(x - 4, 0):x + w + 4].copy()
        ring[y - max(y - 4, 0):y - max(y - 4, 0) + h, x - max(x - 4, 0):x - max(x - 4, 0) + w] = 0
        assert not ring.any(), f"{name}: the margin was written"
        written[y:y + h, x:x + w] = True
    assert not atlas[~written].any()
    # a plain-mode glyph put before and after every flagged put: the same bytes, and the reference's
    assert np.array_equal(texels["plain before"][1], texels["plain after"][1])
    assert MC.over_tolerance(texels["plain before"][1], M.generate(*GLYPH[1:])) <= MC.CAP


def seam(segs, W, H, scale):
    """the pixels of a W x H frame showing the field at `scale` that lie where the ring and the bar of "round ring plus diagonal bar" meet:
    within 1.5 texels of the bar and of the ring's band, and at least half a texel inside the union by step 6's true distance"""
    ys, xs = np.mgrid[0:H, 0:W]
    qx, qy = ((xs + 0.5) / scale).ravel(), ((ys + 0.5) / scale).ravel()
    r = np.hypot(qx - 16.0, qy - 16.0)
    ux, uy = (27.8 - 4.2) / np.hypot(27.8 - 4.2, 5.1 - 26.9), (5.1 - 26.9) / np.hypot(27.8 - 4.2, 5.1 - 26.9)
    off = np.abs((qx - 4.2) * uy - (qy - 26.9) * ux)
    near = (r > 6.3 - 1.5) & (r < 11.2 + 1.5) & (off < 1.6 + 1.5)
    d = OR.true_distance(segs, qx.astype(np.float32), qy.astype(np.float32))
    return (near & (d >= 0.5)).reshape(H, W)


def test_the_composite_glyph_drawn_has_no_hole():
    """"ø" -- round ring plus diagonal bar -- drawn through fdh_draw_msdf at 3 : 1, white on black: with the flag no pixel where bar and ring
    meet is below half alpha; without it there are such pixels (the hole the flag is for)"""
    from figdraw_amd.context import HipContext

    name, segs, w, h = [c for c in OC.inputs() if c[0] == "round ring plus diagonal bar"][0]
    W, H = 3 * w, 3 * h
    where = seam(segs, W, H, 3.0)
    assert where.sum() > 500
    below = {}
    for overlap in (True, False):
        ctx = HipContext(atlas_size=256, device=0)
        ctx.put_glyph_outline(1, segs, w, h, mtsdf=True, sdf_range=4, overlap=overlap)
        ctx.begin_frame(W, H, True, (0.0, 0.0, 0.0, 1.0))
        ctx.draw_msdf(1, (0.0, 0.0), (255, 255, 255, 255), (float(W), float(H)), 4.0, 0.5, 0.0, False, False)
        ctx.end_frame()
        alpha = ctx.read_pixels()[..., 0]
        ctx.close()
        below[overlap] = int((alpha[where] < 128).sum())
    print(f"pixels below half alpha where bar and ring meet ({int(where.sum())} pixels): {below[True]} with the flag, {below[False]} without")
    assert below[True] == 0
    assert below[False] > 0
