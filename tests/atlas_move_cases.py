"""Content for the atlas compaction tests (tests/test_atlas_move_host.py, tests/test_atlas_move.py): every put kind as an entry that can be
put again on any context, the steps that populate an atlas (single puts and batches), the compaction order restated from the header
(include_glyphs/figdraw_hip_atlas.h), and the fresh context of the defining contract."""
import os

import numpy as np

from conftest import GOLDEN

_Z = None


def outlines():
    global _Z
    if _Z is None:
        _Z = np.load(os.path.join(GOLDEN, "outlines_ubuntu20.npz"))
    return _Z


def glyph(code):
    """-> (segs n x 6, w, h) of a glyph of the fixture"""
    z = outlines()
    w, h = (int(v) for v in z[f"size_{code}"])
    return np.ascontiguousarray(z[f"segs_{code}"], np.float32), w, h


def cubic_of(segs6):
    """the same outline with every quadratic raised to a cubic: n x 8 floats (include_glyphs/figdraw_hip_cubic.h)"""
    out = np.full((len(segs6), 8), np.nan, np.float32)
    for i, (x0, y0, cx, cy, x1, y1) in enumerate(segs6):
        out[i, 0:2] = (x0, y0)
        out[i, 6:8] = (x1, y1)
        if cx == cx:
            out[i, 2:4] = (x0 + 2.0 / 3.0 * (cx - x0), y0 + 2.0 / 3.0 * (cy - y0))
            out[i, 4:6] = (x1 + 2.0 / 3.0 * (cx - x1), y1 + 2.0 / 3.0 * (cy - y1))
    return out


def box_outline(w, h):
    """a closed box inside a w x h image (lines only)"""
    p = [(0.25, 0.25), (w - 0.25, 0.25), (w - 0.25, h - 0.25), (0.25, h - 0.25)]
    return np.array([[*p[i], np.nan, np.nan, *p[(i + 1) % 4]] for i in range(4)], np.float32)


def noise(rng, w, h, border=0):
    a = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    if border:
        a[:border] = 0; a[-border:] = 0; a[:, :border] = 0; a[:, -border:] = 0
    return a


class Entry:
    """one atlas entry: its key, the size of its rectangle, and `single(ctx)`, the put call that makes it on any context"""

    def __init__(self, key, w, h, single, kind):
        self.key, self.w, self.h, self.single, self.kind = key, w, h, single, kind


def compaction_order(entries):
    """the header's rule: height descending, then width descending, then key ascending as a signed 64-bit integer"""
    return sorted(entries, key=lambda e: (-e.h, -e.w, e.key))


def image(key, rgba):
    return Entry(key, rgba.shape[1], rgba.shape[0], lambda ctx: ctx.put_image(key, rgba), "image")


def glyph_image(key, rgba, lcd=True):
    return Entry(key, rgba.shape[1], rgba.shape[0], lambda ctx: ctx.put_glyph_image(key, rgba, lcd_filter=lcd), "glyph image")


def coverage(key, segs, w, h, lcd=False):
    return Entry(key, w, h, lambda ctx: ctx.put_glyph_outline(key, segs, w, h, lcd_filter=lcd), "coverage")


def field(key, segs, w, h, sdf_range=0):
    return Entry(key, w, h, lambda ctx: ctx.put_glyph_outline(key, segs, w, h, mtsdf=True, sdf_range=sdf_range), "field")


def coverage_cubic(key, segs8, w, h):
    return Entry(key, w, h, lambda ctx: ctx.put_glyph_outline_cubic(key, segs8, w, h), "coverage, cubic")


def field_cubic(key, segs8, w, h):
    return Entry(key, w, h, lambda ctx: ctx.put_glyph_outline_cubic(key, segs8, w, h, mtsdf=True), "field, cubic")


def image_sdf(key, rgba, pad=2, sdf_range=4):
    return Entry(key, rgba.shape[1] + 2 * pad, rgba.shape[0] + 2 * pad, lambda ctx: ctx.put_image_sdf(key, rgba, channel=3, pad=pad, sdf_range=sdf_range), "image sdf")


def image_sdf_of(key, src, pad=3, sdf_range=6):
    """the field of the texels that the entry `src` holds in the atlas (fdh_put_image_sdf_of)"""
    return Entry(key, src.w + 2 * pad, src.h + 2 * pad, lambda ctx: ctx.put_image_sdf_of(src.key, key, channel=3, pad=pad, sdf_range=sdf_range), "image sdf")


def mips(key, levels):
    return Entry(key, levels[0].shape[1], levels[0].shape[0], lambda ctx: ctx.put_image_mips(key, levels), "mips")


def flippy(key):
    from conftest import load_flippy_levels

    data = open(os.path.join(GOLDEN, "img1.flippy"), "rb").read()
    h, w = load_flippy_levels("img1.flippy")[0].shape[:2]
    return Entry(key, w, h, lambda ctx: ctx.put_flippy(key, data), "flippy")


# how a batch of entries is put in one call; the entries' own `single` is the call the batch is equal to
BATCHES = {
    "fields": lambda ctx, items: ctx.put_glyph_outlines(items),
    "coverage": lambda ctx, items: ctx.put_glyph_coverage_batch(items),
    "fields, cubic": lambda ctx, items: ctx.put_glyph_outlines_cubic(items),
    "coverage, cubic": lambda ctx, items: ctx.put_glyph_coverage_batch_cubic(items),
}


def every_kind(seed=5):
    """-> steps: a list of ("single", entry) and ("batch", kind, [entries], items).  Every put kind of the library: fdh_put_image at 100 x 100
    and at 130 x 7 (no ink boxes), fdh_put_glyph_image with the LCD filter, coverage outlines, an MTSDF field and one that is 1 texel wide,
    fdh_put_image_sdf, fdh_put_image_mips with off-chain sizes, img1.flippy, and one batch of each batch kind."""
    rng = np.random.default_rng(seed)
    steps = []

    def single(e):
        steps.append(("single", e))

    def batch(kind, make, codes, first_key):
        entries, items = [], []
        for i, code in enumerate(codes):
            segs, w, h = glyph(code)
            if "cubic" in kind:
                segs = cubic_of(segs)
            entries.append(make(first_key + i, segs, w, h))
            items.append((first_key + i, segs, w, h))
        steps.append(("batch", kind, entries, items))

    single(image(1, noise(rng, 100, 100, border=3)))
    single(image(2, noise(rng, 130, 7)))
    single(glyph_image(3, noise(rng, 23, 31, border=2)))
    for k, code in enumerate((65, 103, 81, 87)):
        single(coverage(10 + k, *glyph(code), lcd=bool(k & 1)))
    single(field(20, *glyph(82)))
    single(field(21, box_outline(1, 17), 1, 17))   # 1 texel wide: level 0 alone
    single(field(22, box_outline(19, 1), 19, 1))   # 1 texel high
    single(coverage(23, box_outline(1, 9), 1, 9))  # a coverage glyph 1 texel wide: placed, nothing stored
    single(image_sdf(30, np.repeat(noise(rng, 21, 15)[..., 3:], 4, axis=2)))
    # levels whose sizes are not the chain's: level 1 of a 40 x 24 image stored 30 wide and 16 high reaches 20 and 8 level-0 texels past the image
    single(mips(40, [noise(rng, 40, 24), noise(rng, 30, 16), noise(rng, 10, 6), noise(rng, 7, 5)]))
    single(flippy(41))
    batch("fields", field, (66, 67, 68, 105, 108), 100)
    batch("coverage", coverage, (97, 98, 99, 100, 46), 200)
    batch("fields, cubic", field_cubic, (69, 70, 71), 300)
    batch("coverage, cubic", coverage_cubic, (72, 73, 74), 400)
    return steps


def entries_of(steps):
    out = []
    for s in steps:
        out.extend([s[1]] if s[0] == "single" else s[2])
    return out


def populate(ctx, steps):
    """the steps on ctx, in order: single puts and batches"""
    for s in steps:
        if s[0] == "single":
            s[1].single(ctx)
        else:
            BATCHES[s[1]](ctx, s[3])


def fresh_context(live, size, **kw):
    """the defining contract's other side: a fresh context of `size` after the same puts of the live entries, made in compaction order"""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=size, **kw)
    for e in compaction_order(live):
        e.single(ctx)
    assert ctx.atlas_size() == size, "the fresh context grew: the comparison is not the contract's"
    return ctx


def rects(ctx, entries):
    return {e.key: ctx.image_rect(e.key) for e in entries}


def chain_rects(x, y, w, h, n_levels):
    """the level rectangles of the level chain (updateSubImage): (level, x, y, w, h) while both sizes exceed 1"""
    out, level = [], 0
    while w > 1 and h > 1 and level < n_levels:
        out.append((level, x, y, w, h))
        level, x, y, w, h = level + 1, x // 2, y // 2, (w + 1) // 2, (h + 1) // 2
    return out


def shared_deep_texels(rects, n_levels):
    """how many pairs of the given level-0 rectangles (x, y, w, h) have chain rectangles that share a texel at level 4 or deeper: where
    they do, the atlas holds the later put's value and the earlier image's own is nowhere in it"""
    deep = [[r for r in chain_rects(*xywh, n_levels) if r[0] >= 4] for xywh in rects]
    n = 0
    for i, a in enumerate(deep):
        for b in deep[i + 1:]:
            n += any(p[0] == q[0] and p[1] < q[1] + q[3] and q[1] < p[1] + p[3] and p[2] < q[2] + q[4] and q[2] < p[2] + p[4] for p in a for q in b)
    return n
