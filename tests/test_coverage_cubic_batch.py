"""A batch of coverage glyphs with cubic segments in one call on the device (fdh_put_glyph_coverage_batch_cubic,
include_glyphs/figdraw_hip_cubic_batch.h: the host's flattening of the single cubic call, then fdh_put_glyph_coverage_batch's launches).  Level 0 as a
whole array against single fdh_put_glyph_outline_cubic coverage calls on a second context, and against the oracle's rasteriser and
filter on the host's lines (msdf_cubic_cases.flatten_lines restates them; test_msdf_cubic_host.py holds the two together)."""
import numpy as np
import pytest

import msdf_cubic_cases as CC

pytestmark = pytest.mark.gpu
THIN = CC.cpath((0, 1), (3, 2, -2, 6, 1, 8), (0, 8), (0, 1))  # for a 1 x 9 image: placed, and nothing of it is stored


def glyphs():
    """`g&R` and twenty more glyphs of the skewed font set, a 1-texel-wide glyph in the middle -> [(name, segs8, w, h)]"""
    font = CC.skewed()
    out = [font[ord(ch) - 33][:4] for ch in "g&R"] + [c[:4] for c in font[1::5][:20]]
    return out[:11] + [("1 texel wide", THIN, 1, 9)] + out[11:]


@pytest.mark.parametrize("switch", [False, True], ids=["switch off", "switch on"])
@pytest.mark.parametrize("lcd", [False, True, "context"], ids=["plain", "lcd", "context"])
def test_the_batch_is_the_single_calls_and_the_oracle(lcd, switch):
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    gs = glyphs()
    assert len(gs) == 24
    a, b = HipContext(atlas_size=512, device=0), HipContext(atlas_size=512, device=0)
    a.set_text_lcd_filtering(switch)
    b.set_text_lcd_filtering(switch)
    keys = [10 + i for i in range(len(gs))]
    rects = a.put_glyph_coverage_batch_cubic([(k, segs, w, h) for k, (_, segs, w, h) in zip(keys, gs)], lcd_filter=lcd)
    singles = [b.put_glyph_outline_cubic(k, segs, w, h, lcd_filter=lcd) for k, (_, segs, w, h) in zip(keys, gs)]
    assert rects == singles and a.atlas_size() == b.atlas_size() == 512 and all(a.has_image(k) for k in keys)
    st = a.glyph_coverage_batch_stats()
    filtered = switch if lcd == "context" else bool(lcd)
    assert st["glyphs"] == st["written"] == 24 and st["launches"] == 2 + (1 if filtered else 0) + 2 * 10 - 1  # a 512 atlas: 10 levels
    assert st["edges"] == sum(len(CC.flatten_lines(segs)) for _, segs, _, _ in gs)
    got, single = a.debug_read_surface(4), b.debug_read_surface(4)
    a.close()
    b.close()
    assert np.array_equal(got, single), f"{int((got != single).any(axis=2).sum())} texels of level 0 differ from the single calls'"
    want = np.zeros_like(got)
    for (name, segs, w, h), (x, y, rw, rh) in zip(gs, rects):
        assert (rw, rh) == (w, h)
        if w == 1 or h == 1:
            continue  # placed and unwritten: the level chain stores nothing of such an image
        img = O.rasterize_outline(CC.lines_as_outline(CC.flatten_lines(segs)), w, h)
        want[y:y + h, x:x + w] = O.lcd_filter(img) if filtered else img
    assert want[..., 3].max() == 255 and np.array_equal(got, want)
    x, y, _, _ = rects[11]
    assert not got[max(y - 4, 0):y + 9 + 4, max(x - 4, 0):x + 1 + 4].any()  # the 1-texel-wide glyph and its margin
