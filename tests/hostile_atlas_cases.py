"""Hostile atlas draws for the compositor, as data (no GPU): the frames of tests/test_hostile_atlas.py, tests/test_hostile_atlas_host.py
and `tools/make_goldens.py hostile_atlas`.  The companion of tests/hostile_cases.py, which holds no atlas draw: this is modes 0 and 13 - 16
(draw_image, draw_image_adj, draw_msdf, text glyphs), where generated glyph fields, image distance fields and compacted atlases end up.

The atlas path is as full of geometric arguments as the SDF path: "the strip's texels lie between those of its first and last pixel",
"a window of 64 x 12 texels is inside the level", "this pixel IS its texel", "below this byte the draw has no ink", "this level is the
last one".  The frames put the arguments where they are tightest.

Every frame is 250 x 190 (hostile_cases.W, H) over an atlas of 256 (ref_scenes.ATLAS_GOLDEN_SIZE, the reason is written there).  The
images are put in sorted-key order on every backend (put_images); the rectangles must come out equal and some sit against the atlas'
edges (EDGE_RECTS).  Frames come in the two forms of hostile_cases.calls: direct, and `lists`, shifted copies until a phase passes 64
records.  Two families have no golden and are held, quad by quad, to tests/atlas_sample_ref.py instead (ORACLE_ONLY): `steep`, whose alpha
slope per texel is far beyond the 16-bit coordinate grid of the reference shaders' sampler, and `minified_msdf`, which the reference's
desktop and GLES shaders sample differently."""
import math
import os

import numpy as np

import hostile_cases as HC
from hostile_cases import GLASS, H, SHIFT, W, WHITE, _sdf

ATLAS = 256
SEED = 0x61746C73

# ------------------------------------------------------------------------------------------------ the images
K_NOISE, K_CHECK, K_ZERO, K_FULL, K_HALF, K_ONE, K_COL, K_ROW, K_THIN, K_MIPS = 100, 110, 120, 130, 140, 150, 160, 170, 180, 190
K_TALL, K_DISC = 4000, 4010
K_PHOTO = 3000
COVERAGE = tuple(1000 + ord(c) for c in "Rg&a")
MSDF = tuple(2000 + ord(c) for c in "Rg&")
K_R, K_G, K_AMP = MSDF
MIP_COLOURS = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255))  # level 0 .. 5 of K_MIPS: 32, 16, .. 1 texels

# where the packer puts them (asserted on every backend by put_images): x, y, w, h.  K_NOISE has x = 4 and y = 4, K_TALL y + h = S - 4,
# K_DISC x + w = S - 5 -- the packer's right limit: findEmptyRect asks for i + w + 2 margin < S, one texel more than at the bottom.
EDGE_RECTS = {K_NOISE: (4, 4, 80, 28), K_TALL: (24, 96, 30, 156), K_DISC: (201, 108, 50, 24), K_ROW: (210, 4, 40, 1)}

_IMAGES = None


def images():
    """key -> h x w x 4 uint8 (a list of those: a mip chain given level by level).  The fixture's coverage glyphs, MSDF glyphs and
    photograph, and a seeded recipe: RGBA white noise (every channel its own, so the median of three is no single channel), a 0 / 255
    checkerboard of 1-texel cells, all-0 and all-255, a field with every byte on the threshold (128), a 1 x 1 image, a 1 x 40 and a 40 x 1
    sliver, an image 4 texels wide, flat levels of distinct colours, a tall noise strip and a smooth disc field (the last two fill the
    atlas to its bottom and right edge)."""
    global _IMAGES
    if _IMAGES is None:
        from figdraw_amd.scenes import load_glyph_fixture

        fx = load_glyph_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glyphs_ubuntu20.npz"))
        rng = np.random.default_rng(SEED)
        out = {k: fx[k] for k in COVERAGE + MSDF + (K_PHOTO,)}
        out[K_NOISE] = rng.integers(0, 256, size=(28, 80, 4), dtype=np.uint8)
        yy, xx = np.mgrid[0:24, 0:24]
        out[K_CHECK] = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 4, axis=2)
        out[K_ZERO] = np.zeros((12, 12, 4), np.uint8)
        out[K_FULL] = np.full((12, 12, 4), 255, np.uint8)
        out[K_HALF] = np.full((20, 20, 4), 128, np.uint8)
        out[K_ONE] = np.array([[[200, 100, 50, 255]]], np.uint8)
        out[K_COL] = rng.integers(0, 256, size=(40, 1, 4), dtype=np.uint8)
        out[K_ROW] = rng.integers(0, 256, size=(1, 40, 4), dtype=np.uint8)
        out[K_THIN] = rng.integers(0, 256, size=(12, 4, 4), dtype=np.uint8)
        out[K_MIPS] = [np.tile(np.array(c + (255,), np.uint8), (32 >> l, 32 >> l, 1)) for l, c in enumerate(MIP_COLOURS)]
        out[K_TALL] = rng.integers(0, 256, size=(156, 30, 4), dtype=np.uint8)
        yy, xx = np.mgrid[0:24, 0:50]
        d = 9.0 - np.hypot(xx + 0.5 - 25.0, (yy + 0.5 - 12.0) * 1.6)  # texels inside an ellipse, range 4: byte = 128 + 32 d
        out[K_DISC] = np.repeat(np.clip(np.round(128.0 + 32.0 * d), 0, 255).astype(np.uint8)[..., None], 4, axis=2)
        for v in out.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
        _IMAGES = out
    return _IMAGES


def put_images(backend, imgs=None, order=None):
    """the images in sorted-key order (or `order`) on an Oracle, a HipContext or a RefGL -> key: rectangle"""
    imgs = images() if imgs is None else imgs
    rects = {}
    for k in (sorted(imgs) if order is None else order):
        rects[k] = tuple(backend.put_image_mips(k, imgs[k]) if isinstance(imgs[k], list) else backend.put_image(k, imgs[k]))
    if order is None and imgs is _IMAGES:
        for k, r in EDGE_RECTS.items():
            assert rects[k] == r, (k, rects[k], r)
    return rects


# ------------------------------------------------------------------------------------------------ the calls
INK = (20, 20, 30, 255)
SOLID = [INK] * 4
VERTICAL = [(200, 30, 30, 255), (200, 30, 30, 255), (30, 60, 220, 200), (30, 60, 220, 200)]  # BL, BR, TR, TL: one colour per row
FOUR = [(255, 255, 0, 255), (0, 255, 255, 230), (255, 0, 255, 255), (255, 255, 255, 120)]
PLAIN = [(255, 255, 255, 255)] * 4


def _img(key, x, y, w=0.0, h=0.0, cols=PLAIN, flip=0):
    return ["draw_image", int(key), [float(x), float(y)], [list(c) for c in cols], [float(w), float(h)], int(flip)]


def _adj(key, x, y, w, h, col=(255, 255, 255, 255)):
    return ["draw_image_adj", int(key), [float(x), float(y)], list(col), [float(w), float(h)]]


def _msdf(key, x, y, w, h, px_range=4.0, thr=0.5, sw=0.0, mtsdf=0, flip=0, col=INK):
    return ["draw_msdf", int(key), [float(x), float(y)], list(col), [float(w), float(h)], float(px_range), float(thr), float(sw), int(mtsdf), int(flip)]


def _under(ops, body):
    return [["save_transform"]] + ops + body + [["restore_transform"]]


def window():
    """The 4-wide atlas path (k_composite_strip.inc) takes a strip's texel window from three of its pixels, stages it in LDS while it is
    small and inside the level, and clamps the taps of lanes outside the quad into it; neighbouring strips of one quad take different
    routes as soon as one of them has a lane whose extrapolated tap leaves the level -- which is what entries against the atlas' edges
    are for (K_NOISE at x = 4, y = 4, K_TALL at the bottom, K_DISC and K_ROW at the right).  Magnified draws in modes 0, 13 - 16: both
    flips, quads mirrored through the transform, anisotropic quads, quads over the frame's edges.  (The size limits of the window,
    kWinCols and kWinRows, are only reached by MINIFIED distance fields, which the reference's desktop and GLES shaders sample
    differently -- textureLod 0 against texture2D: those draws are `minified_msdf`, without a golden.)"""
    out = [_img(K_NOISE, 3.4, 2.3, 96, 33.6, PLAIN, 0), _img(K_NOISE, 3.6, 38.4, 120, 42, VERTICAL, 1), _msdf(K_R, 128.3, 2.6, 96, 96, 4.0, 0.5, 0.0, 0, 1, col=(20, 20, 160, 255))]
    out += _under([["translate", 246.6, 84.4], ["scale", -1.0, 1.0]], [_msdf(K_G, 0.0, 0.0, 70, 70, 4.0, 0.45, 0.0, 1, 0, col=(120, 20, 160, 230))])
    out += _under([["translate", 4.3, 188.7], ["scale", 1.0, -1.0]], [_msdf(K_AMP, 0.0, 0.0, 64, 80, 4.0, 0.45, 2.5, 1, 0, col=(0, 0, 0, 200))])
    out.append(_img(K_CHECK, 108.4, 120.7, 60, 48, FOUR, 1))
    out += _under([["translate", 240.2, 160.4], ["scale", -1.0, 1.0]], [_img(K_NOISE, 0.0, 0.0, 96, 33.6, VERTICAL, 0)])
    out.append(_img(K_DISC, 168.3, 150.2, 80, 38.4, PLAIN, 0))
    out.append(_msdf(K_DISC, 70.3, 84.2, 100, 48, 4.0, 0.5, 0.0, 0, 0, col=(238, 140, 30, 230)))
    out.append(_msdf(K_DISC, 60.7, 130.6, 75, 60, 4.0, 0.45, 3.0, 1, 1, col=(20, 120, 60, 255)))
    out.append(_img(K_ROW, 120.5, 172.3, 80, 6, PLAIN, 0))
    out.append(_img(K_TALL, 226.3, -40.4, 45, 234, SOLID, 0))  # over the top and the bottom edge
    out.append(_img(K_TALL, -12.6, 80.3, 36, 187.2, FOUR, 1))   # over the left and the bottom edge
    out.append(_img(COVERAGE[0], 100.3, 40.6, 39, 42, SOLID, 0))
    return out


# ------------------------------------------------------------------------------------------------ the families without a golden
def _q(call, xf=None):
    """a quad of an oracle-only family: the call, and the (sx, sy, tx, ty) it is drawn under"""
    return (call, xf)


def _minified_msdf_quads():
    out = []
    for i, wpx in enumerate((39, 40, 41)):  # the column limit, on noise (rows magnified)
        out.append(_q(_msdf(K_NOISE, 3.3 + 43.4 * i, 2.3, wpx, 42, (0.5, 4.0, 0.5)[i], (0.5, 0.45, 0.4)[i], (0.0, 0.0, 2.5)[i], i == 1)))
    for i, (wpx, hpx) in enumerate(((49, 70), (50, 69), (51, 71))):  # both limits, on the photograph's colours
        out.append(_q(_msdf(K_PHOTO, 3.6 + 53.2 * i, 46.4 + 0.3 * i, wpx, hpx, 0.5, 0.4, 0.0, 0, i == 2, col=(200, 30, 60, 220))))
    for i, hpx in enumerate((109, 110, 104)):  # the row limit, on the tall strip (columns magnified; the last one hangs over the frame's right edge)
        out.append(_q(_msdf(K_TALL, 162.4 + 33.3 * i, 2.6 + 1.7 * i, 45, hpx, 0.5, 0.5, 0.0, i == 1, 0, col=(20, 120, 60, 255))))
    for i, hpx in enumerate((18, 19, 20, 21)):
        out.append(_q(_msdf(K_NOISE, 3.4, 118.3 + 17.6 * i, 100, hpx, 0.5, 0.5, 0.0, 0, i % 2, col=(30, 30, 200, 255))))
    out.append(_q(_msdf(K_NOISE, 0.0, 0.0, 40, 42, 0.5, 0.5, 0.0, 0, 0, col=(120, 20, 160, 255)), (-1.0, 1.0, 246.6, 118.4)))
    out.append(_q(_msdf(K_NOISE, 0.0, 0.0, 90, 19, 0.5, 0.45, 0.0, 1, 0, col=(0, 0, 0, 200)), (1.0, -1.0, 110.3, 188.7)))
    tiny = [(K_R, 0.3, 0.3, 4.0, 0.5, 0.0, 0), (K_R, 0.3, 28, 4.0, 0.5, 0.0, 0), (K_R, 28, 0.3, 4.0, 0.5, 0.0, 0), (K_G, 1.0, 1.0, 4.0, 0.5, 0.0, 0), (K_G, 2.49, 2.49, 4.0, 0.5, 3.0, 1),
            (K_G, 7.0, 7.0, 4.0, 0.5, 0.0, 0), (K_R, 3.2, 3.2, 4.0, 0.5, 0.0, 0), (K_PHOTO, 10, 10, 4.0, 0.4, 0.0, 0), (K_NOISE, 8, 3, 4.0, 0.5, 0.0, 1), (K_NOISE, 40, 14, 0.5, 0.5, 0.0, 0),
            (K_NOISE, 40, 14, 0.01, 0.45, 3.0, 0), (K_R, 28, 28, 4.0, 0.5, 0.0, 0), (K_DISC, 28, 14, 4.0, 0.5, 0.05, 1)]
    for i, (key, w, h, rng, thr, sw, mt) in enumerate(tiny):  # 0.1x and below: spr clamps at 1, sampling stays at level 0
        out.append(_q(_msdf(key, 112.4 + 30.6 * (i % 2) + 0.1 * i, 118.6 + 10.3 * (i // 2), w, h, rng, thr, sw, mt, 0, col=(200, 30, 60, 255))))
    return out


def _steep_quads():
    out = [_q(_img(K_CHECK, 200.5, 60.5, 4000, 4000, PLAIN, 1))]
    steep = [(K_R, 3.3, 2.6, 70, 70, 64.0, 0.5, 0.0, 0, 0), (K_G, 80.4, 3.7, 70, 70, 1e4, 0.5, 0.0, 1, 0), (K_AMP, 160.6, 2.3, 70, 70, 64.0, 0.45, 3.0, 0, 1),
             (K_DISC, 3.6, 80.4, 100, 48, 64.0, 0.5, 3.0, 1, 0), (K_R, -200.3, -230.6, 640, 640, 4.0, 0.5, 0.0, 0, 0), (K_NOISE, 3.4, 132.3, 100, 35, 64.0, 0.5, 0.0, 0, 0),
             (K_CHECK, 40.7, 150.2, 60, 36, 1e4, 0.5, 3.0, 1, 0), (K_FULL, 110.6, 150.4, 28, 28, 1e4, 0.98, 0.0, 1, 0)]
    for i, q in enumerate(steep):  # px_range 64 and 1e4 on fields of range 4, a glyph at 20x
        out.append(_q(_msdf(*q, col=[(20, 20, 160, 255), (200, 30, 60, 200)][i % 2])))
    # draw_image where the colour says which levels were mixed, and how: flat levels at fractional levels of detail, the photograph far down its chain
    for i, s in enumerate((31, 15, 5, 3)):
        out.append(_q(_img(K_MIPS, 150.3 + 33.4 * (i > 0) + 17.3 * (i > 1), 152.6 + 8.3 * (i > 2), s, s)))
    out += [_q(_img(K_MIPS, 238.4, 176.2, 11, 11, PLAIN, 1)), _q(_img(K_PHOTO, 172.4, 134.6, 12, 12)), _q(_img(K_PHOTO, 193.3, 130.7, 6, 25, VERTICAL)),
            _q(_img(K_PHOTO, 187.6, 134.3, 1, 1)), _q(_img(K_NOISE, 2.2, 104.6, 79, 27, FOUR))]
    return out


ORACLE_ONLY = {"minified_msdf": _minified_msdf_quads, "steep": _steep_quads}


def quads(name):
    return ORACLE_ONLY[name]()


def quad_calls(call, xf):
    return _under([["translate", xf[2], xf[3]], ["scale", xf[0], xf[1]]], [call]) if xf else [call]


def minified_msdf():
    """Minified distance fields (always sampled at level 0).  The window of the 4-wide path spans fewer than kWinCols = 64 columns and
    kWinRows = 12 rows: along a strip's 32 pixels the first and last tap are 31 s texels apart at s texels per pixel and the window is
    that floor-difference + 2 columns, so it fits while the difference is <= 62 -- always below s = 2, never above 2 + 1/31, for some
    strips but not their neighbours in between; along its 8 rows the difference may be 10: s = 10 / 7 = 1.43.  So: 80 texels on 41, 40
    and 39 pixels (s = 1.95, 2, 2.05), 100 on 51, 50, 49, with the rows magnified, so that only the column limit is crossed; 28 rows on 21,
    20, 19, 18 pixels (s = 1.33, 1.4, 1.47, 1.56), 156 on 110, 109, 104, with the columns magnified; 100 rows on 70 (exactly 10 / 7), 69, 71;
    flipped and mirrored.  And 0.1x and below, where spr clamps at 1.  No golden (the GLES shaders the goldens come from sample a minified
    field from its mip chain, the desktop shaders at level 0): each quad, drawn alone, is held to tests/atlas_sample_ref.py."""
    return [c for call, xf in quads("minified_msdf") for c in quad_calls(call, xf)]


def steep():
    """alpha slopes per texel far beyond what the reference shaders' sampler resolves (its coordinates have 16 bits: 256 steps per texel
    on this atlas; its level of detail a few bits of fraction): px_range 64 and 1e4 on fields of range 4, a glyph at 20x, a checkerboard
    at 166x, flat mip levels of distinct colours and noise at fractional levels.  No golden: each quad, drawn alone, is held to
    tests/atlas_sample_ref.py."""
    return [c for call, xf in quads("steep") for c in quad_calls(call, xf)]


def one_to_one():
    """Recorder::draw_image declares a pixel to be its texel when the quad is upright, unflipped, its ceil-snapped corners as far apart
    as the image is large and the sub-pixel shift 0; the kernel then reads the lane's four texels as one unaligned 16-byte run that begins
    up to 3 texels left of the entry (the packer's margin is what keeps it inside the level).  For each condition a case that holds
    and one that narrowly fails: position x.0 / x.0001 / x.9999, size +- 0.4, shift 0 / 1e-3 / 0.999, flip_y, scale 1 / 1.0001 -- with a
    solid, a vertical and a four-colour tint, at every x phase of the 4-pixel lanes, hanging over all four frame edges, and on the
    entries against the atlas' edges.  (The context's sub-pixel switch is on for the whole frame: tests/hostile_atlas_cases.calls.)"""
    imgs = images()
    keys = COVERAGE + (K_CHECK, K_THIN, K_COL)
    tints = (SOLID, VERTICAL, FOUR)
    variants = [(0.0, 0.0, 0.0, 0, 1.0), (0.0001, 0.0, 0.0, 0, 1.0), (0.9999, 0.0, 0.0, 0, 1.0), (0.0, 0.4, 0.0, 0, 1.0), (0.0, -0.4, 0.0, 0, 1.0),
                (0.5, 0.4, 0.0, 0, 1.0), (0.0, 0.0, 1e-3, 0, 1.0), (0.0, 0.0, 0.999, 0, 1.0), (0.0, 0.0, 0.0, 1, 1.0), (0.0, 0.0, 0.0, 0, 1.0001),
                (0.0, 0.0, 0.5, 0, 1.0), (0.3, 0.0, 0.0, 0, 1.0)]
    out, n = [], 0
    for row in range(4):
        for i, (fx, dsz, shift, flip, sc) in enumerate(variants):
            key = keys[(n + row) % len(keys)]
            h, w = imgs[key].shape[:2]
            x, y = 5.0 + 19.0 * i + row + fx, 6.0 + 19.0 * row + (fx if row % 2 else 0.0)
            call = _img(key, x, y, w + dsz if dsz else 0.0, h + dsz if dsz else 0.0, tints[(n + row) % 3], flip)
            out.append(["set_text_subpixel_shift", shift])
            out += _under([["scale", sc, sc]], [call]) if sc != 1.0 else [call]
            n += 1
    out.append(["set_text_subpixel_shift", 0.0])
    out += [_img(K_NOISE, -5.0, 84.0, 0, 0, FOUR), _img(K_NOISE, 177.0, 90.0, 0, 0, VERTICAL), _img(K_NOISE, 80.0, -9.0 + 190.0 - 10.0, 0, 0, SOLID),
            _img(K_DISC, 83.0, 88.0, 0, 0, PLAIN), _img(K_TALL, 139.0, -3.0, 0, 0, SOLID), _img(K_TALL, 171.0, 40.0, 0, 0, FOUR), _img(K_ROW, 86.0, 116.0, 0, 0, PLAIN),
            _img(K_ROW, 230.0, 120.0, 0, 0, PLAIN), _img(K_PHOTO, 2.0, 118.0, 0, 0, VERTICAL), _img(COVERAGE[0], -6.0, -7.0, 0, 0, SOLID),
            _img(COVERAGE[1], 243.0, 181.0, 0, 0, SOLID), _img(K_ONE, 120.0, 130.0, 0, 0, PLAIN), _img(K_MIPS, 106.0, 126.0, 0, 0, PLAIN)]
    out += _under([["translate", 0.25, 0.75]], [_img(K_CHECK, 205.75, 150.25, 0, 0, FOUR)])  # a fractional translate that lands on integers
    return out


# (key, w, h, px_range, sd_threshold, stroke_weight, mtsdf, alpha): every value of every parameter; cut = threshold - 0.5 / spr - 0.008 on
# both sides of 0 (5, 7, 8: below; 0, 10, 29: above) and of 1 (13: spr 1, cut 0.992; 12, 27: above 1).  The ranges 64 and 1e4 stand where the
# reference shaders' sampler cannot see them: alpha 1 / 255, flat fields, thresholds that saturate (their steep use is `steep`); the sizes
# below the field's own are in `minified_msdf`.  33 pixels for 32 texels: just magnified.
_RANGES = [
    (K_R, 33, 33, 4.0, 0.5, 0.0, 0, 255), (K_G, 33, 33, 4.0, 0.45, 3.0, 0, 255), (K_AMP, 33, 33, 4.0, 0.5, 0.0, 1, 255), (K_R, 33, 33, 4.0, 0.45, 3.0, 1, 255),
    (K_R, 33, 33, 0.5, 0.5, 0.0, 0, 255), (K_G, 33, 33, 0.01, 0.5, 0.0, 0, 255), (K_AMP, 33, 33, 0.5, 0.45, 0.05, 0, 255), (K_R, 33, 33, 4.0, 0.02, 0.0, 0, 255),
    (K_G, 33, 33, 4.0, 0.0, 0.0, 1, 255), (K_AMP, 33, 33, 4.0, -0.5, 0.0, 0, 255), (K_R, 33, 33, 4.0, 0.98, 0.0, 1, 255), (K_G, 33, 33, 4.0, 1.0, 0.0, 0, 255),
    (K_AMP, 33, 33, 4.0, 1.5, 0.0, 0, 255), (K_R, 33, 33, 0.5, 1.5, 0.0, 1, 255), (K_G, 33, 33, 4.0, 0.5, 1000.0, 0, 255), (K_AMP, 33, 33, 4.0, 0.5, 1000.0, 1, 255),
    (K_R, 33, 33, 64.0, 0.5, 0.0, 0, 1), (K_G, 33, 33, 1e4, 0.5, 0.0, 1, 1), (K_HALF, 28, 28, 64.0, 0.5, 0.0, 0, 255), (K_HALF, 28, 28, 1e4, 0.5, 3.0, 1, 255),
    (K_HALF, 28, 28, 4.0, 0.5, 0.0, 0, 255), (K_ZERO, 28, 28, 1e4, 0.0, 0.0, 0, 255), (K_FULL, 28, 28, 4.0, 1.0, 0.0, 1, 255), (K_R, 66, 33, 4.0, 0.5, 0.05, 0, 255),
    (K_AMP, 33, 33, 0.01, 0.98, 0.05, 1, 255), (K_CHECK, 24, 24, 0.5, 0.5, 0.0, 1, 255), (K_CHECK, 26, 26, 0.5, 0.45, 0.05, 1, 255), (K_R, 33, 33, 64.0, 1.5, 0.0, 0, 255),
    (K_R, 33, 33, 64.0, -0.5, 0.0, 0, 255), (K_R, 33, 33, 1e4, 0.02, 0.0, 0, 1), (K_R, 33, 33, 0.5, 0.02, 3.0, 0, 255), (K_G, 40, 70, 4.0, 0.5, 0.0, 0, 255),
    (K_NOISE, 84, 30, 0.5, 0.5, 0.0, 0, 255), (K_NOISE, 84, 30, 0.01, 0.45, 3.0, 0, 255), (K_NOISE, 82, 29, 0.5, 0.98, 0.0, 1, 255),
]


def ranges():
    """draw_msdf of fixture glyphs and of the noise, checkerboard, flat and threshold-byte fields in all four modes: px_range 0.01 .. 1e4,
    sd_threshold -0.5 .. 1.5, stroke_weight 0 .. 1000, sizes up to 3 W, colour alpha 1 and 255 (_RANGES).  Recorder::draw_msdf shrinks
    a fill's bounds to the ink above `cut`: a wrong cut drops pixels without any error, and FDH_INK_BOUNDS=0 must give the same frame."""
    out = [_msdf(K_HALF, -250.4, -280.6, 3.0 * W, 3.0 * W, 0.5, 0.5, 0.0, 0, 0, col=(90, 0, 140, 255)),   # 3 W: alpha 0.5 + spr / 510 all over the frame
           _msdf(K_AMP, -300.3, -200.7, 3.0 * W, 3.0 * W, 4.0, 0.5, 0.0, 1, 0, col=(0, 0, 0, 1))]
    for i, (key, w, h, rng, thr, sw, mt, a) in enumerate(_RANGES):
        col = [(200, 30, 60), (20, 120, 60), (30, 30, 200), (0, 0, 0)][i % 4] + (a,)
        x, y = (3.3 + 31.0 * (i % 8), 2.6 + 31.0 * (i // 8)) if i < 32 else (3.4 + 83.2 * (i - 32), 159.3)
        out.append(_msdf(key, x, y, w, h, rng, thr, sw, mt, i % 5 == 4, col=col))
    return out


def minified():
    """draw_image below 1:1: atlas_sample clamps the level of detail to the last level and mixes two levels.  rho just below 1 (100 texels
    on 101 pixels), exactly 1, exactly 2 (100 on 50, 80 on 40, 32 on 16), just above (100 on 49, 80 on 39: quads are snapped to whole pixels,
    so rho is a ratio of integers -- 2.04 is as near as it gets), 4, 8, and beyond the last level (100 x 100 texels on 0.3 pixels and on 3);
    rho from one axis only; flipped; the flat-level entry at whole levels, whose colour says which level a pixel came from (at fractional
    levels the reference shaders' sampler is 5 LSB off: `steep`).  draw_image_adj on an image 4 texels wide and on the 1 x 1 image: the uv
    rect, pulled in by two texels a side, is empty or inverted."""
    out = [_img(K_PHOTO, 2.3, 2.4, 101, 101), _img(K_PHOTO, 106.6, 3.7, 100, 100, VERTICAL), _img(K_PHOTO, 210.4, 2.6, 50, 50), _img(K_PHOTO, 208.3, 56.4, 49, 49, FOUR),
           _img(K_PHOTO, 2.5, 106.3, 100, 25), _img(K_PHOTO, 106.4, 106.6, 25, 80, PLAIN, 1), _img(K_PHOTO, 135.3, 108.4, 33, 33, VERTICAL, 1),
           _img(K_PHOTO, 175.8, 110.4, 0.3, 0.3), _img(K_PHOTO, 187.5, 114.2, 3, 3),
           _img(K_NOISE, 2.6, 134.2, 40, 14), _img(K_NOISE, 45.3, 134.7, 39, 14, FOUR), _img(K_NOISE, 2.4, 151.3, 20, 7),
           _img(K_NOISE, 84.7, 160.3, 81, 29, VERTICAL), _img(K_NOISE, 26.5, 150.4, 10, 3.5, PLAIN, 1)]
    for i, s in enumerate((32, 16, 8, 4, 2, 1)):
        out.append(_img(K_MIPS, 172.3 + (0, 34.4, 34.4, 52.6, 52.6, 62.3)[i], 142.6 + (0, 0, 17.3, 0, 9.2, 0)[i], s, s))
    out += [_img(K_MIPS, 205.6, 110.3, 32, 8), _img(K_MIPS, 238.4, 176.2, 16, 16, PLAIN, 1), _adj(K_THIN, 206.4, 82.3, 20, 24, (255, 255, 255, 255)),
            _adj(K_ONE, 228.6, 82.7, 9, 9, (255, 0, 0, 255)), _adj(K_CHECK, 206.3, 120.4, 40, 20.5, (40, 180, 90, 200)), _adj(K_PHOTO, 60.3, 130.2, 30, 30, (255, 255, 255, 255))]
    return out


ROTATIONS = (0.001, 45.0, 90.0, 180.0, -33.3)


def _shear(tx, ty, k):
    """a column-major 4 x 4 (apply_transform) that shears x by k y and moves by (tx, ty)"""
    return [1.0, 0.0, 0.0, 0.0, float(k), 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, float(tx), float(ty), 0.0, 1.0]


def rotated():
    """The same entries under rotations of 0.001, 45, 90, 180 and -33.3 degrees and a shear: one level of detail per triangle
    (QuadExt::lod), trilinear sampling across the diagonal, the builds of the compositor for general quads.  (The flat-level entry sits on
    a whole level under the rotations that keep rho a ratio of integers and is magnified under the others: at fractional levels its
    colours show the reference shaders' own level-of-detail precision, 5 LSB.)"""
    out = []
    for i, deg in enumerate(ROTATIONS + (None,)):
        cx, cy = 42.3 + 82.6 * (i % 3), 48.6 + 92.3 * (i // 3)
        body = [_msdf(K_R, -38.0, -38.0, 50, 50, 4.0, 0.5, 0.0, i % 2, 0, col=(20, 20, 160, 255)), _img(K_PHOTO, -6.5, -30.5, 36, 36, PLAIN, i == 2),
                _img(K_MIPS, 14.5, 8.5, *((16, 16) if deg in (0.001, 90.0, 180.0) else (40, 36))), _msdf(K_G, -8.0, -4.0, 34, 48, 4.0, 0.45, 2.5, 1, 0, col=(200, 40, 20, 230)),
                _img(K_NOISE, -36.5, 32.5, 60, 9), _adj(K_DISC, 10.5, -36.0, 52, 26, (0, 0, 0, 255))] + ([_img(COVERAGE[i % 4], -30.0, 14.0, 0, 0, FOUR)] if i in (1, 3) else [])
        ops = [["apply_transform", _shear(cx, cy, 0.35)]] if deg is None else [["translate", cx, cy], ["rotate", math.radians(deg)]]
        out += _under(ops, body)
    return out


def rotated_mix():
    """rotated SDF quads and upright atlas quads in one phase (has_rot && has_atlas: the upright quads keep their 4-wide path inside the
    build for general quads), and one rotated atlas quad among them"""
    out = []
    for i, deg in enumerate((45.0, -33.3, 0.001)):
        out += _under([["translate", 50.3 + 70.4 * i, 36.6], ["rotate", math.radians(deg)]],
                      [_sdf([-30.5, -18.25, 61.0, 36.5], (220, 40, 40, 200), (2, 9, 0.5, 14)), _sdf([-30.5, -18.25, 61.0, 36.5], (0, 0, 0, 255), (2, 9, 0.5, 14), 12, 4.0)])
        out += [_msdf(MSDF[i], 20.4 + 70.3 * i, 72.2, 60, 60, 4.0, 0.5, 0.0, i == 1, 0, col=(20, 20, 160, 220)), _img(COVERAGE[i], 30.0 + 70.0 * i, 134.0, 0, 0, SOLID),
                _img(K_PHOTO, 10.3 + 80.2 * i, 150.4, 70, 38, VERTICAL)]
    out += _under([["translate", 225.4, 110.3], ["rotate", math.radians(21.0)]], [_img(K_PHOTO, -20.5, -20.5, 41, 41)])
    return out


def far_atlas():
    """Coordinates of +-40000 and on both sides of the 1e6 of one_to_one (those quads are glyph-sized, so they are off the frame: they
    must leave nothing); quads of 16000 and 50000 pixels of which the frame shows a few texels (magnification 500: every pixel of a strip in
    one texel, a window one texel wide)."""
    out = [_img(K_PHOTO, -20000.3, -30000.6, 50000, 50000), _img(K_NOISE, -40000.5, 20.3, 40100, 56, VERTICAL), _img(K_TALL, 180.4, -40000.2, 60, 40100.5, FOUR, 1),
           _img(K_DISC, 200.5, 60.5, 8000, 4000, PLAIN, 1)]
    for x in (40000.0, -40000.0, 999000.0, 1000100.0, -999000.0, -1000100.0):
        out += [_img(COVERAGE[0], x, 40.0, 0, 0, SOLID), _img(COVERAGE[1], 40.0, x, 0, 0, SOLID)]
    out += _under([["translate", -999990.0, 0.0]], [_img(COVERAGE[2], 999990.0 + 120.0, 90.0, 0, 0, SOLID)])
    out += _under([["translate", 0.0, 1000100.0]], [_img(COVERAGE[3], 140.0, -1000100.0 + 90.0, 0, 0, FOUR)])
    return out


def far_fields():
    """... and distance fields on quads of 16000 to 80000 pixels, with px_range 0.03 .. 0.0008 so that the slope stays what a sampler
    resolves: column 25 of the disc field at 320 pixels a texel, its edge crossing the frame (the quad ends at y = 146: what lies
    below is not drawn over a layer that already differs by one); a column of the g on a band 80000 wide"""
    out = []
    out += [_msdf(K_HALF, 20.3, 150.6, 39000, 39000, 0.01, 0.5, 0.0, 1, 0, col=(90, 0, 140, 120)),
            _msdf(K_DISC, -7875.4, -382.3, 16000, 528, 0.03, 0.5, 0.0, 0, 0, col=(20, 20, 160, 200)),
            _msdf(K_DISC, 100.6, 100.3, 40000, 40, 0.01, 0.5, 3.0, 1, 0, col=(200, 30, 60, 255)), _msdf(K_G, -40000.0, 150.4, 80000, 34, 0.0008, 0.45, 0.0, 0, 0, col=(0, 90, 0, 220))]
    return out


# name -> (body builder, clear colour, the context's sub-pixel switch)
FAMILIES = {
    "window": (window, GLASS, False), "one_to_one": (one_to_one, WHITE, True), "ranges": (ranges, GLASS, False), "minified": (minified, WHITE, False),
    "rotated": (rotated, WHITE, False), "rotated_mix": (rotated_mix, GLASS, False), "far_atlas": (far_atlas, GLASS, False), "far_fields": (far_fields, GLASS, False),
    "minified_msdf": (minified_msdf, GLASS, False), "steep": (steep, GLASS, False),
}
DRAWS = ("draw_image", "draw_image_adj", "draw_msdf", "draw_rounded_rect_sdf")


def n_draws(body):
    return sum(c[0] in DRAWS for c in body)


def body_of(name):
    return FAMILIES[name][0]()


def wrap(body, clear, subpixel, form="direct", copies=None):
    """begin_frame .. end_frame around a body (the sub-pixel switch belongs to the context: set before the frame, cleared after it)"""
    out = [["set_text_subpixel", 1, 0.0]] if subpixel else []
    out.append(["begin_frame", 1, list(clear)])
    if form == "direct":
        out += body
    else:
        assert form == "lists"
        for c in range(copies):
            out += [["save_transform"], ["translate", SHIFT[0] * c, SHIFT[1] * c]] + body + [["restore_transform"]]
    out.append(["end_frame"])
    if subpixel:
        out.append(["set_text_subpixel", 0, 0.0])
    return out


LISTS_COPIES = {"far_atlas": 16}  # (most of its quads are off the frame on purpose and leave no record)


def calls(name, form="direct"):
    """the call stream of a call-level frame"""
    body_fn, clear, subpixel = FAMILIES[name]
    body = body_fn()
    return wrap(body, clear, subpixel, form, LISTS_COPIES.get(name, HC.copies_for_lists(n_draws(body))))


# ------------------------------------------------------------------------------------------------ node-level frames
NODE_FRAMES = ("nodes_text", "nodes_images")
NODE_CLEAR = GLASS
NODE_COPIES = 5


def scene(name, form="direct"):
    """nkText, nkImage, nkMsdfImage and nkMtsdfImage nodes, some under NfInvertY, rotation and clips: the front-end's decomposition and
    culling in the loop"""
    from figdraw_amd.scene import Fig, FigFlags, FigKind, Glyph, RenderList, Renders, fill, rect, rgba

    imgs = images()
    lst = RenderList()
    lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(0, 0, W, H), fill=rgba(244, 244, 238, 255)))
    for c in range(1 if form == "direct" else NODE_COPIES):
        dx, dy = SHIFT[0] * c, SHIFT[1] * c
        tint = [rgba(255, 255, 0, 255), rgba(0, 255, 255, 255), rgba(255, 0, 255, 255), rgba(30, 30, 30, 255)]
        if name == "nodes_text":
            for row, (flags, rot) in enumerate(((FigFlags(0), 0.0), (FigFlags.NfInvertY, 0.0), (FigFlags(0), 180.0), (FigFlags.NfInvertY, 90.0))):
                glyphs = [Glyph(image_id=k, x=4.3 + 15.37 * i, y=20.0 - imgs[k].shape[0], colors=tint if i % 2 else [rgba(20, 20, 20, 255)] * 4,
                                subpixel_shift=(-1.0 if row % 2 else 0.25 * i)) for i, k in enumerate(COVERAGE + COVERAGE)]
                f = Fig(kind=FigKind.nkText, screenBox=rect(6.4 + 60.3 * (row // 2) + dx, 8.6 + 44.3 * row + dy, 130, 24), glyphs=glyphs, flags=flags)
                if rot:
                    f.rotation = rot
                lst.addRoot(f)
            cl = lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(150.3 + dx, 20.6 + dy, 80, 50), fill=rgba(255, 255, 255, 255), corners=[14] * 4,
                                 flags=FigFlags.NfClipContent))
            lst.addChild(cl, Fig(kind=FigKind.nkText, screenBox=rect(140.2 + dx, 30.4 + dy, 130, 24),
                                 glyphs=[Glyph(image_id=k, x=3.0 + 14.0 * i, y=20.0 - imgs[k].shape[0], colors=tint) for i, k in enumerate(COVERAGE + COVERAGE)]))
        else:
            lst.addRoot(Fig(kind=FigKind.nkImage, screenBox=rect(4.4 + dx, 3.6 + dy, 70, 70), image_id=K_PHOTO))
            lst.addRoot(Fig(kind=FigKind.nkImage, screenBox=rect(80.3 + dx, 5.2 + dy, 27, 31), image_id=K_PHOTO, flags=FigFlags.NfInvertY, image_fill=fill(rgba(255, 200, 200, 200))))
            lst.addRoot(Fig(kind=FigKind.nkImage, screenBox=rect(80.6 + dx, 42.3 + dy, 30, 30), image_id=K_PHOTO, rotation=45.0))
            lst.addRoot(Fig(kind=FigKind.nkMsdfImage, screenBox=rect(120.4 + dx, 4.3 + dy, 60, 60), image_id=K_G, image_fill=fill(rgba(200, 40, 20, 255)), pxRange=1.5,
                            sdThreshold=0.45, strokeWeight=3.0, flags=FigFlags.NfInvertY))
            lst.addRoot(Fig(kind=FigKind.nkMtsdfImage, screenBox=rect(185.6 + dx, 6.7 + dy, 40.2, 33.4), image_id=K_R, image_fill=fill(rgba(20, 20, 160, 255)), pxRange=4.0,
                            sdThreshold=0.5))
            lst.addRoot(Fig(kind=FigKind.nkMtsdfImage, screenBox=rect(190.3 + dx, 20.4 + dy, 50, 50), image_id=K_R, rotation=-33.3, image_fill=fill(rgba(20, 20, 160, 255)),
                            pxRange=0.5, sdThreshold=0.4))
            lst.addRoot(Fig(kind=FigKind.nkMsdfImage, screenBox=rect(8.3 + dx, 80.6 + dy, 100, 48), image_id=K_DISC, image_fill=fill(rgba(0, 0, 0, 200)), pxRange=4.0,
                            sdThreshold=0.02))
            cl = lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(120.5 + dx, 80.3 + dy, 90, 70), fill=rgba(255, 255, 255, 255), corners=[18] * 4,
                                 flags=FigFlags.NfClipContent))
            lst.addChild(cl, Fig(kind=FigKind.nkImage, screenBox=rect(110.2 + dx, 70.4 + dy, 120, 100), image_id=K_PHOTO))
            lst.addChild(cl, Fig(kind=FigKind.nkMsdfImage, screenBox=rect(130.6 + dx, 90.3 + dy, 64, 64), image_id=K_AMP, rotation=180.0, image_fill=fill(rgba(0, 0, 0, 255)),
                                 pxRange=4.0, sdThreshold=0.5))
            lst.addChild(cl, Fig(kind=FigKind.nkMtsdfImage, screenBox=rect(10.2 + dx, 10.4 + dy, 24, 24), image_id=K_G, image_fill=fill(rgba(0, 0, 0, 255)), pxRange=4.0,
                                 sdThreshold=0.5))  # outside its clip: culled
            lst.addRoot(Fig(kind=FigKind.nkImage, screenBox=rect(300.5 + dx, 20.3 + dy, 50, 50), image_id=K_PHOTO))  # off the frame: culled
            rm = lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(20.4 + dx, 135.7 + dy, 90, 40), fill=rgba(230, 230, 255, 255), corners=[6] * 4,
                                 flags=FigFlags.NfRectMaskContent))
            lst.addChild(rm, Fig(kind=FigKind.nkImage, screenBox=rect(10.3 + dx, 130.2 + dy, 96, 33.6), image_id=K_NOISE))
    out = Renders()
    out.setLayer(0, lst)
    return out


# ------------------------------------------------------------------------------------------------ the frames, by name
FRAMES = tuple(FAMILIES) + NODE_FRAMES
GOLDEN_FRAMES = tuple(n for n in FRAMES if n not in ORACLE_ONLY)
FORMS = HC.FORMS
# the direct forms the library composites without a bin launch (fdh_context.cpp direct_frame: at most 64 draws in every phase, none of them on
# the slot path): the families whose quads are all upright, unmirrored and sampled at level 0.  A quad mirrored through the transform is
# recorded as a general quad (`window`, `minified_msdf`), a minified draw_image takes the trilinear slot path (`minified`, `steep`).
TAKES_DIRECT_LAUNCH = ("one_to_one", "ranges", "far_atlas", "far_fields")
STRIPES = HC.STRIPES
STRIPE_FRAMES = ("window", "one_to_one", "nodes_images")
AMPLIFIED = {}  # name, form -> [(x, y, reason)]: the rule of hostile_cases.AMPLIFIED, at most hostile_cases.MAX_AMPLIFIED per frame
MAX_AMPLIFIED = HC.MAX_AMPLIFIED
MAX_GOLDEN_OUTLIERS = HC.MAX_GOLDEN_OUTLIERS


def is_node_frame(name):
    return name in NODE_FRAMES


def clear_of(name):
    return NODE_CLEAR if is_node_frame(name) else FAMILIES[name][1]


def render(backend, name, form="direct"):
    """draw frame `name` on `backend` (an Oracle or a HipContext that holds the images: put_images)"""
    if is_node_frame(name):
        backend.render_frame(scene(name, form), W, H, color=tuple(clear_of(name)))
    else:
        backend.W, backend.H = W, H
        (backend.replay_calls if hasattr(backend, "replay_calls") else backend.replay)(calls(name, form))


# ------------------------------------------------------------------------------------------------ deliberately wrong variants (host test)
def mutate_calls(cs, kind):
    """the calls with one parameter wrong: `px_range` x 1.05, `threshold` + 1 / 255, `shift` dropped, `size` + 1 px"""
    out = []
    for c in cs:
        c = [list(a) if isinstance(a, list) else a for a in c]
        if kind == "px_range" and c[0] == "draw_msdf":
            c[5] = c[5] * 1.05
        elif kind == "threshold" and c[0] == "draw_msdf":
            c[6] = c[6] + 1.0 / 255.0
        elif kind == "shift" and c[0] == "set_text_subpixel_shift":
            c[1] = 0.0
        elif kind == "size" and c[0] in ("draw_image", "draw_image_adj", "draw_msdf"):
            k = imgs_size(c[1]) if (c[0] == "draw_image" and not (c[4][0] > 0 and c[4][1] > 0)) else c[4]
            c[4] = [k[0] + 1.0, k[1] + 1.0]
        out.append(c)
    return out


def imgs_size(key):
    v = images()[key]
    v = v[0] if isinstance(v, list) else v
    return [float(v.shape[1]), float(v.shape[0])]


def mutate_images(kind):
    """the images with one thing wrong: `mips` the levels of K_MIPS swapped in pairs (0 <-> 1, 2 <-> 3, 4 <-> 5); `roll` every image's
    texels rolled by one column"""
    out = dict(images())
    if kind == "mips":
        m = [a.copy() for a in out[K_MIPS]]
        for l in range(0, len(m) - 1, 2):
            m[l][..., :3], m[l + 1][..., :3] = MIP_COLOURS[l + 1], MIP_COLOURS[l]
        out[K_MIPS] = m
    else:
        assert kind == "roll"
        for k, v in out.items():
            out[k] = [np.roll(a, 1, axis=1) for a in v] if isinstance(v, list) else np.roll(v, 1, axis=1)
    return out
