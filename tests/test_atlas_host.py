"""The image atlas (figdraw_amd/csrc/fdh_atlas.h, class Atlas; the glyph puts: fdh_glyphs.h, class GlyphMaker) as a record-only context shows it: one packer behind every put kind, placed
where the oracle places; growth through the put kinds; a refused put leaves nothing behind; and the draw records that read the
directory (Recorder's entry lookup and axis-aligned LOD), pinned by digests made with the library of the commit before the atlas moved
out of Context (tests/golden/atlas_record_digests.json)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import msdf_cases as MC
from conftest import GOLDEN, load_flippy_levels
from figdraw_amd.context import HipContext
from oracle import oracle as O

INVALID = -1
MTSDF = 4


def _packed_area(ctx):
    out = C.c_int64()
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(out)) == 0
    return out.value


def _square(w, h):
    """a closed square outline inside a w x h image"""
    return MC.poly([(0.25, 0.25), (w - 0.25, 0.25), (w - 0.25, h - 0.25), (0.25, h - 0.25)])


def _mips(w, h):
    out = [np.full((h, w, 4), 200, np.uint8)]
    while out[-1].shape[0] > 1 and out[-1].shape[1] > 1:
        ph, pw = out[-1].shape[:2]
        out.append(np.full(((ph + 1) // 2, (pw + 1) // 2, 4), 200, np.uint8))
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. placements
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_placements_equal_the_oracles_for_every_put_kind(seed):
    rng = np.random.default_rng(seed)
    sizes = [(int(w), int(h)) for w, h in rng.integers(1, 49, size=(48, 2))]
    flippy = open(os.path.join(GOLDEN, "img1.flippy"), "rb").read()
    fh, fw = load_flippy_levels("img1.flippy")[0].shape[:2]
    orc, img = O.Oracle(atlas_size=512), HipContext(atlas_size=512, record_only=True)
    want = [orc.put_image(i, np.zeros((h, w, 4), np.uint8)) for i, (w, h) in enumerate(sizes)]  # (a fit failure raises: the test fails)
    assert [img.put_image(i, np.zeros((h, w, 4), np.uint8)) for i, (w, h) in enumerate(sizes)] == want
    want.append(orc.put_image(48, np.zeros((fh, fw, 4), np.uint8)))  # the container's level 0, as one more item
    assert img.put_image(48, np.zeros((fh, fw, 4), np.uint8)) == want[48]
    assert max(r[1] + r[3] for r in want) <= 512 and img.atlas_size() == 512
    # the same sizes through the other put kinds, in turn
    ctx = HipContext(atlas_size=512, record_only=True)
    kinds = [lambda k, w, h: ctx.put_glyph_image(k, np.zeros((h, w, 4), np.uint8)),
             lambda k, w, h: ctx.put_glyph_outline(k, _square(w, h), w, h),
             lambda k, w, h: ctx.put_glyph_outline(k, _square(w, h), w, h, mtsdf=True),
             lambda k, w, h: ctx.put_image_mips(k, _mips(w, h))]
    got = [kinds[i % 4](i, w, h) for i, (w, h) in enumerate(sizes)]
    got.append(ctx.put_flippy(48, flippy))
    assert got == want
    assert ctx.atlas_size() == 512 and all(ctx.has_image(i) for i in range(49)) and _packed_area(ctx) == _packed_area(img) > 0
    for c in (ctx, img, orc):
        c.close()


# ------------------------------------------------------------------------------------------------------------------ 2. growth, refused puts
def test_growth_through_the_glyph_put_kinds_and_refused_puts():
    ctx = HipContext(atlas_size=64, record_only=True)
    assert ctx.atlas_size() == 64
    ctx.put_glyph_image(1, np.full((20, 20, 4), 255, np.uint8))
    assert ctx.has_image(1)
    rect = ctx.put_glyph_outline(2, _square(60, 60), 60, 60, mtsdf=True)  # needs 68 px: grows to 128
    assert ctx.atlas_size() == 128 and ctx.has_image(2) and not ctx.has_image(1)
    fresh = O.Oracle(atlas_size=128)
    assert rect == fresh.put_image(2, np.zeros((60, 60, 4), np.uint8))
    fresh.close()
    # a put refused by validation leaves the directory and the packed area exactly as they were
    area = _packed_area(ctx)
    out = (C.c_int * 4)()
    open_contour = np.ascontiguousarray(_square(12, 11)[:3])
    assert ctx.L.fdh_put_glyph_outline(ctx.h, 81, 12, 11, open_contour.ctypes.data, 3, MTSDF, out) == INVALID
    assert ctx.L.fdh_put_glyph_outline(ctx.h, 82, 12, 11, open_contour.ctypes.data, 3, 8, out) == INVALID  # an unknown flag
    px = np.zeros((11, 12, 4), np.uint8)
    assert ctx.L.fdh_put_glyph_image(ctx.h, 83, 12, 11, px.ctypes.data, 8, out) == INVALID
    assert not ctx.has_image(81) and not ctx.has_image(82) and not ctx.has_image(83) and ctx.has_image(2)
    assert _packed_area(ctx) == area and ctx.atlas_size() == 128
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 3. records
WHITE = [(255, 255, 255, 255)] * 4


def build_frames(ctx):
    """-> {frame name: record_digest()} on a record-only context with a 256 atlas.  Every frame is 200 x 160."""
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, size=(18, 26, 4), dtype=np.uint8)
    img[:3] = 0; img[:, :4] = 0; img[-2:] = 0; img[:, -5:] = 0  # a transparent border: the ink boxes are smaller than the image
    ctx.put_image(1, img)
    field = rng.integers(0, 256, size=(32, 32, 4), dtype=np.uint8)
    field[:6] = 0; field[:, :5] = 0; field[-4:] = 0; field[:, -7:] = 0
    ctx.put_image(2, field)  # a field whose texels the host saw (ink boxes)
    ctx.put_glyph_outline(3, _square(28, 24), 28, 24, mtsdf=True)  # ... and one made on the device (none)
    ctx.put_glyph_image(4, img)
    out = {}

    def frame(name, body, subpixel=None):
        ctx.set_text_subpixel(subpixel is not None, subpixel or 0.0)
        ctx.begin_frame(200, 160, True, (0.1, 0.2, 0.3, 1.0))
        body()
        ctx.end_frame()
        out[name] = ctx.record_digest()

    frame("image upright 1:1", lambda: ctx.draw_image(1, (10, 12), WHITE))
    frame("image upright 1:1, glyph put", lambda: ctx.draw_image(4, (31, 40), WHITE))
    frame("image at a fractional position", lambda: ctx.draw_image(1, (10.4, 12.7), WHITE))
    frame("image flipped", lambda: ctx.draw_image(1, (10, 12), WHITE, flip_y=True))
    frame("image magnified", lambda: ctx.draw_image(1, (5, 6), WHITE, size=(65.0, 45.0)))
    frame("image minified", lambda: ctx.draw_image(1, (5, 6), [(255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255), (9, 9, 9, 128)], size=(9.0, 7.0)))
    frame("image, sub-pixel on, shift 0", lambda: ctx.draw_image(1, (10, 12), WHITE), subpixel=0.0)
    frame("image, sub-pixel on, shift 0.4", lambda: ctx.draw_image(1, (10, 12), WHITE), subpixel=0.4)

    def rotated(draw):
        def body():
            ctx.save_transform()
            ctx.translate(90, 70)
            ctx.rotate(math.radians(30))
            draw()
            ctx.restore_transform()
        return body

    def scaled(draw):
        def body():
            ctx.save_transform()
            ctx.scale(1.5, 0.75)
            draw()
            ctx.restore_transform()
        return body

    frame("image rotated", rotated(lambda: ctx.draw_image(1, (-13, -9), WHITE)))
    frame("image under a scale", scaled(lambda: ctx.draw_image(1, (10, 12), WHITE)))
    frame("image_adj", lambda: ctx.draw_image_adj(1, (20, 30), (255, 128, 0, 255), (52.0, 36.0)))
    frame("image_adj minified, sub-pixel 0.4", lambda: ctx.draw_image_adj(1, (20.5, 30.25), (255, 128, 0, 200), (11.0, 8.0)), subpixel=0.4)
    frame("image_adj rotated", rotated(lambda: ctx.draw_image_adj(1, (-20, -10), (1, 2, 3, 255), (40.0, 20.0))))
    for key, mtsdf in ((2, False), (3, True), (2, True)):
        for stroke in (0.0, 1.5):
            tag = f"{'mtsdf' if mtsdf else 'msdf'} key {key} stroke {stroke}"
            frame(tag, lambda: ctx.draw_msdf(key, (12, 14), (0, 0, 0, 255), (96.0, 96.0), 4.0, 0.5, stroke, mtsdf=mtsdf))
            frame(tag + " flipped", lambda: ctx.draw_msdf(key, (12, 14), (0, 0, 0, 255), (64.0, 48.0), 4.0, 0.5, stroke, mtsdf=mtsdf, flip_y=True))
            frame(tag + " rotated", rotated(lambda: ctx.draw_msdf(key, (-30, -30), (0, 0, 0, 255), (60.0, 60.0), 4.0, 0.45, stroke, mtsdf=mtsdf)))
    frame("rect (creates the white image)", lambda: ctx.draw_rect((10, 10, 50, 30), (200, 10, 10, 255)))
    frame("filled quad", lambda: ctx.draw_filled_quad((10, 10, 80, 20, 70, 90, 5, 60), [(255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255), (255, 255, 0, 255)]))
    frame("rect rotated", rotated(lambda: ctx.draw_rect((-20, -10, 40, 20), (0, 0, 0, 128))))
    frame("image after the white image", lambda: ctx.draw_image(1, (14, 9), WHITE))
    frame("nothing", lambda: None)

    def missing():
        ctx.draw_image(99, (10, 12), WHITE)
        ctx.draw_image_adj(99, (20, 30), (255, 128, 0, 255), (52.0, 36.0))
        ctx.draw_msdf(99, (12, 14), (0, 0, 0, 255), (96.0, 96.0), 4.0)
    frame("a missing key", missing)
    ctx.set_text_subpixel(False)
    return out


def test_records_are_the_parents():
    """The digests in tests/golden/atlas_record_digests.json were made by build_frames() above against the library built from the commit
    named in the file (tools/make_atlas_digests.py with FIGDRAW_HIP_LIB pointing at that build), never by the code under test."""
    golden = json.load(open(os.path.join(GOLDEN, "atlas_record_digests.json")))
    assert len(golden["parent_commit"]) == 40
    ctx = HipContext(atlas_size=256, record_only=True)
    got = build_frames(ctx)
    assert ctx.atlas_size() == 256
    ctx.close()
    assert got["a missing key"] == got["nothing"], "a draw of a missing key records nothing"
    assert len(set(got.values())) == len(got) - 1, "every other frame has records of its own"
    assert sorted(got) == sorted(golden["digests"])
    wrong = [name for name in got if f"{got[name]:016x}" != golden["digests"][name]]
    assert not wrong, wrong
