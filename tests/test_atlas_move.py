"""Atlas compaction on the device (include_glyphs/figdraw_hip_atlas.h; k_atlas_move and the level chain's kernels): after puts of every
kind, removals and fdh_compact_atlas -- or the compactions of keep mode -- EVERY level of the atlas is byte for byte what a fresh context
of that size holds after the same puts of the live entries in compaction order.  No tolerance: the texels are moved, not made."""
import numpy as np
import pytest

import atlas_move_cases as AC

pytestmark = pytest.mark.gpu
WHITE = [(255, 255, 255, 255)] * 4


def _all_levels(ctx):
    size, out = ctx.atlas_size(), []
    while size >= 1 and len(out) < 14:
        out.append(ctx.read_atlas_level(len(out)))
        size >>= 1
    return out


def _same_atlas(ctx, live, what):
    """ctx against the fresh context of the contract: size, rectangles, packed area and every level; -> level 0"""
    fresh = AC.fresh_context(live, ctx.atlas_size(), device=0)
    try:
        assert AC.rects(ctx, live) == AC.rects(fresh, live), what
        assert ctx.atlas_usage()["packed_area"] == fresh.atlas_usage()["packed_area"], what
        got, want = _all_levels(ctx), _all_levels(fresh)
        assert len(got) == len(want)
        for l, (g, w) in enumerate(zip(got, want)):
            differ = int((g != w).any(axis=2).sum())
            assert differ == 0, f"{what}: level {l}: {differ} texels differ from the fresh context's"
        assert want[0].any() and want[3].any() and want[4].any()
        return got[0]
    finally:
        fresh.close()


def _without(entries, keys):
    return [e for e in entries if e.key not in keys]


# ------------------------------------------------------------------------------------------------------------------ 6. fdh_compact_atlas
def test_every_level_after_compaction_is_the_fresh_contexts():
    from figdraw_amd.context import HipContext

    steps = AC.every_kind()
    entries = AC.entries_of(steps)
    ctx = HipContext(atlas_size=512, device=0)
    AC.populate(ctx, steps)
    assert ctx.atlas_size() == 512 and all(ctx.has_image(e.key) for e in entries)
    gone = {13, 21, 101, 201, 301, 401}  # (the 130 x 7 image, the glyph image and the fields but one thin one stay: they are moved three times)
    old = {k: ctx.image_rect(k) for k in gone}
    for k in gone:
        ctx.remove_image(k)
    live = _without(entries, gone)
    st = ctx.compact_atlas(0)  # the same size
    assert st["size_after"] == 512 and st["entries"] == len(live) and st["launches"] >= 3 and st["tiles"] > 0 and st["packed_after"] < st["packed_before"]
    level0 = _same_atlas(ctx, live, "same size")
    inside = np.zeros(level0.shape[:2], bool)
    for x, y, w, h in AC.rects(ctx, live).values():
        inside[y:y + h, x:x + w] = True
    assert not level0[~inside].any(), "texels of removed entries are gone"
    assert any(not inside[y:y + h, x:x + w].all() for x, y, w, h in old.values())
    st = ctx.compact_atlas(1024)  # larger: more levels than the old atlas had
    assert (st["size_before"], st["size_after"]) == (512, 1024)
    _same_atlas(ctx, live, "larger")
    more = {1, 41, 40, 100, 200, 202, 203, 204, 300, 302, 400, 402}  # the large images and some glyphs: what is left fits 256
    for k in more:
        ctx.remove_image(k)
    live = _without(live, more)
    st = ctx.compact_atlas(256)  # smaller
    assert (st["size_before"], st["size_after"]) == (1024, 256)
    _same_atlas(ctx, live, "smaller")
    u = ctx.atlas_usage()
    assert (u["compactions"], u["rebuilds"], u["entries"]) == (3, 0, len(live))
    ctx.close()


def test_texels_that_a_neighbour_overwrote_are_the_images_own_again():
    """Two images side by side share columns of levels 5 and 6; the later put's value stands there, the earlier image's own is nowhere in
    the atlas.  The compaction swaps the two (the second is taller): the first image is now the later one and must show its own texels
    -- which a copy of the old levels cannot produce."""
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(2)
    a, b, c = AC.image(1, AC.noise(rng, 100, 100)), AC.image(2, AC.noise(rng, 100, 104)), AC.glyph_image(3, AC.noise(rng, 30, 33, border=1))
    ctx = HipContext(atlas_size=256, device=0)
    for e in (a, b, c):
        e.single(ctx)
    old = AC.rects(ctx, [a, b, c])
    assert old[1] == (4, 4, 100, 100) and old[2] == (112, 4, 100, 104)
    assert AC.shared_deep_texels([old[1], old[2]], 9) == 1, "the test's images must share a deep texel"
    before = _all_levels(ctx)
    ctx.compact_atlas(0)
    new = AC.rects(ctx, [a, b, c])
    assert new[2] == (4, 4, 100, 104) and new[1] == (112, 4, 100, 100)
    _same_atlas(ctx, [a, b, c], "swapped neighbours")
    after = _all_levels(ctx)
    assert any(not np.array_equal(x, y) for x, y in zip(before[5:7], after[5:7]))
    ctx.close()


def test_entries_with_levels_of_their_own_keep_them_next_to_neighbours():
    """fdh_put_image_mips with off-chain sizes and the Flippy container between glyphs, at 256: their levels meet their neighbours' from
    level 1 on, in the old atlas and in the new one"""
    from figdraw_amd.context import HipContext

    steps = [s for s in AC.every_kind() if s[0] == "single" and s[1].key in (40, 41, 10, 11, 12, 13, 20, 3, 30)]
    steps = steps[2:] + steps[:2]  # the glyphs last: they overwrite what the two containers share with them
    entries = AC.entries_of(steps)
    ctx = HipContext(atlas_size=256, device=0)
    AC.populate(ctx, steps)
    assert ctx.atlas_size() == 256
    ctx.compact_atlas(0)
    _same_atlas(ctx, entries, "own levels, same size")
    ctx.remove_image(10)
    ctx.compact_atlas(512)
    _same_atlas(ctx, _without(entries, {10}), "own levels, larger")
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 7. keep mode
class Script:
    """atlas calls applied to a context and remembered, so that a record-only twin can repeat them (same packer, same sizes)"""

    def __init__(self, ctx):
        self.ctx, self.ops = ctx, []

    def do(self, *op, ctx=None):
        c = ctx or self.ctx
        if ctx is None:
            self.ops.append(op)
        if op[0] == "put":
            op[1].single(c)
        elif op[0] == "batch":
            AC.BATCHES[op[1]](c, op[3])
        elif op[0] == "remove":
            c.remove_image(op[1])
        elif op[0] == "compact":
            c.compact_atlas(op[1])

    def fill(self, first_key, side):
        """side x side images until one more would grow the atlas (a record-only twin without keep repeats the script and says when)"""
        from figdraw_amd.context import HipContext

        twin = HipContext(atlas_size=256, record_only=True)
        twin.set_atlas_keep(True)
        for op in self.ops:
            self.do(*op, ctx=twin)
        assert twin.atlas_size() == self.ctx.atlas_size() and twin.atlas_usage()["rebuilds"] == 0
        twin.set_atlas_keep(False)
        px, n = np.full((side, side, 4), 77, np.uint8), 0
        while True:
            twin.put_image(first_key + n, px)
            if twin.atlas_usage()["rebuilds"]:
                break
            n += 1
        twin.close()
        out = [AC.image(first_key + k, px) for k in range(n)]
        for e in out:
            self.do("put", e)
        return out


def _keep_case(removals):
    """a 256 atlas in keep mode, filled to the last 10 x 10 image; `removals`: then every filler is removed again.  -> script, live entries"""
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(9)
    ctx = HipContext(atlas_size=256, device=0)
    ctx.set_atlas_keep(True)
    sc = Script(ctx)
    base = [AC.image(1, AC.noise(rng, 100, 100, border=2)), AC.coverage(10, *AC.glyph(65)), AC.field(20, *AC.glyph(82)), AC.flippy(41),
            AC.mips(40, [AC.noise(rng, 40, 24), AC.noise(rng, 30, 16), AC.noise(rng, 10, 6)])]
    for e in base:
        sc.do("put", e)
    fillers = sc.fill(1000, 24) + sc.fill(2000, 10)
    assert ctx.atlas_size() == 256 and ctx.atlas_usage()["compactions"] == 0 and len(fillers) > 20
    if removals:
        for e in fillers:
            sc.do("remove", e.key)
        return sc, base
    return sc, base + fillers


def _same_as_compaction_then(ctx, live, then, what):
    """keep mode's definition: the live entries in compaction order, then the call's images in call order, on a fresh context of that size"""
    from figdraw_amd.context import HipContext

    fresh = HipContext(atlas_size=ctx.atlas_size(), device=0)
    for e in AC.compaction_order(live) + then:
        e.single(fresh)
    assert fresh.atlas_size() == ctx.atlas_size() and fresh.atlas_usage()["rebuilds"] == 0
    assert AC.rects(ctx, live + then) == AC.rects(fresh, live + then), what
    for l, (g, w) in enumerate(zip(_all_levels(ctx), _all_levels(fresh))):
        differ = int((g != w).any(axis=2).sum())
        assert differ == 0, f"{what}: level {l}: {differ} texels differ from the fresh context's"
    fresh.close()


@pytest.mark.parametrize("what", ["glyph image", "field of an entry"])
@pytest.mark.parametrize("removals,size", [(True, 256), (False, 512)])
def test_keep_mode_single_put(removals, size, what):
    """S' = S where removed entries left the room, S' = 2S where live content needs it.  "field of an entry": fdh_put_image_sdf_of, whose
    source waits in scratch while the compaction moves everything -- the source too, and entries with kept levels beside it"""
    sc, live = _keep_case(removals)
    ctx = sc.ctx
    if what == "glyph image":
        put = AC.glyph_image(50, AC.noise(np.random.default_rng(1), 37, 41, border=3))
    else:
        put = AC.image_sdf_of(50, [e for e in live if e.key == 10][0], pad=9, sdf_range=6)
    put.single(ctx)
    u = ctx.atlas_usage()
    assert (ctx.atlas_size(), u["compactions"], u["rebuilds"]) == (size, 1, 0) and all(ctx.has_image(e.key) for e in live + [put])
    _same_as_compaction_then(ctx, live, [put], f"S' = {size}")
    ctx.close()


@pytest.mark.parametrize("removals,size,kind", [(True, 256, "coverage"), (False, 512, "fields"), (False, 512, "fields, cubic"), (True, 256, "coverage, cubic")])
def test_keep_mode_batch(removals, size, kind):
    """a batch that does not fit compacts ONCE, before any of its glyphs is placed, and is then the batch it always was"""
    sc, live = _keep_case(removals)
    ctx = sc.ctx
    step = [s for s in AC.every_kind() if s[0] == "batch" and s[1] == kind][0]
    AC.BATCHES[kind](ctx, step[3])
    u = ctx.atlas_usage()
    stats = ctx.glyph_batch_stats() if kind.startswith("fields") else ctx.glyph_coverage_batch_stats()
    assert (ctx.atlas_size(), u["compactions"], u["rebuilds"]) == (size, 1, 0) and stats["dropped_by_growth"] == 0 and stats["written"] == len(step[2])
    assert all(ctx.has_image(e.key) for e in live + step[2])
    _same_as_compaction_then(ctx, live, step[2], f"{kind}, S' = {size}")
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 8. rendering
def _tree(keys):
    import ref_scenes as RS
    from figdraw_amd.scene import Fig, FigKind, RenderList, Renders

    lst = RenderList()
    lst.addRoot(Fig(kind=RS.RECT, screenBox=RS.rect(0, 0, 400, 300), fill=RS.rgba(90, 100, 110, 255)))
    lst.addRoot(Fig(kind=FigKind.nkImage, screenBox=RS.rect(10, 10, 63, 57), image_id=keys["image"]))
    lst.addRoot(Fig(kind=FigKind.nkImage, screenBox=RS.rect(90, 10, 100, 100), image_id=keys["image"]))
    lst.addRoot(Fig(kind=FigKind.nkMtsdfImage, screenBox=RS.rect(200, 20, 90, 100), image_id=keys["field"], image_fill=RS.fill(RS.rgba(10, 10, 60, 255)), pxRange=4.0, sdThreshold=0.5))
    out = Renders()
    out.layers[0] = lst
    return out


def _frame(c, glyph_keys, sizes, image, field):
    c.begin_frame(400, 300, True, (0.8, 0.85, 0.9, 1.0))
    x = 5.0
    for k in glyph_keys:  # 1:1 glyph quads
        c.draw_image(k, (x, 8.0), WHITE)
        x += sizes[k][0] + 3
    c.draw_image(image, (12.5, 60.25), WHITE, size=(41.0, 37.0))  # a scaled image: trilinear
    c.draw_image(image, (70.0, 60.0), WHITE, size=(150.0, 150.0))
    c.draw_msdf(field, (240.0, 70.0), (20, 20, 20, 255), (110.0, 120.0), 4.0, 0.5, 0.0, True, False)
    c.draw_msdf(field, (240.0, 200.0), (200, 20, 20, 255), (45.0, 50.0), 4.0, 0.5, 1.5, True, False)
    c.end_frame()
    return c.read_pixels()


def test_rendering_after_compaction_and_a_frame_in_flight():
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    steps = [s for s in AC.every_kind() if s[0] == "single" and s[1].kind not in ("mips", "flippy")]
    entries = AC.entries_of(steps)
    ctx = HipContext(atlas_size=512, device=0)
    AC.populate(ctx, steps)
    glyph_keys = [e.key for e in entries if e.kind == "coverage" and e.w > 1]
    sizes = {e.key: (e.w, e.h) for e in entries}
    before = _frame(ctx, glyph_keys, sizes, 1, 20)
    ctx.scene_retain(_tree({"image": 1, "field": 20}), 400, 300)
    retained_before = ctx.read_pixels()
    # 9. a frame in flight when the atlas is compacted: nothing has waited for it yet
    ctx.begin_frame(400, 300, True, (0.8, 0.85, 0.9, 1.0))
    for i in range(40):
        ctx.draw_image(1, (float(3 * i), float(2 * i)), WHITE, size=(180.0, 180.0))
    ctx.end_frame()
    for k in (12, 23, 11):
        ctx.remove_image(k)
    live = [e for e in entries if e.key not in (12, 23, 11)]
    ctx.compact_atlas(0)
    in_flight = ctx.read_pixels()
    fresh = AC.fresh_context(live, 512, device=0)
    fresh.begin_frame(400, 300, True, (0.8, 0.85, 0.9, 1.0))
    for i in range(40):
        fresh.draw_image(1, (float(3 * i), float(2 * i)), WHITE, size=(180.0, 180.0))
    fresh.end_frame()
    # (the same draws from another place of the atlas: the pixels of a frame do not depend on where its images lie ...)
    assert np.array_equal(in_flight, fresh.read_pixels()), "the frame in flight"
    # 8. the frames after the compaction, against the fresh context bit for bit
    glyph_keys = [k for k in glyph_keys if k not in (11, 12)]
    after = _frame(ctx, glyph_keys, sizes, 1, 20)
    want = _frame(fresh, glyph_keys, sizes, 1, 20)
    assert np.array_equal(after, want)
    ctx.scene_render()
    retained_after = ctx.read_pixels()
    fresh.render_frame(_tree({"image": 1, "field": 20}), 400, 300)
    assert np.array_equal(retained_after, fresh.read_pixels()), "the retained scene was not rebuilt from the new positions"
    assert np.array_equal(retained_after, retained_before), "... and shows the same images"
    assert before.shape == after.shape
    # ... and within the suite's bar of the oracle, which holds the texels the device made
    orc = O.Oracle(atlas_size=512, threads=8)
    level0 = ctx.read_atlas_level(0)
    for e in AC.compaction_order(live):
        x, y, w, h = ctx.image_rect(e.key)
        assert orc.put_image(e.key, level0[y:y + h, x:x + w].copy()) == (x, y, w, h)
    ref = _frame(orc, glyph_keys, sizes, 1, 20)
    d = np.abs(after.astype(int) - ref.astype(int))
    print(f"after compaction: max |hip - oracle| = {d.max()} LSB on {int((d > 0).any(axis=2).sum())} pixels")
    assert d.max() <= 1
    orc.close(); fresh.close(); ctx.close()


def test_a_frame_in_flight_is_finished_from_the_old_atlas():
    """the same frame rendered and read, then rendered again and left in flight while fdh_compact_atlas moves everything"""
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(4)
    ctx = HipContext(atlas_size=512, device=0)
    for k in range(6):
        ctx.put_image(k, AC.noise(rng, 60 + 7 * k, 50 + 3 * k))

    def frame():
        ctx.begin_frame(640, 400, True, (0.0, 0.0, 0.0, 1.0))
        for i in range(60):
            ctx.draw_image(i % 6, (float(9 * i), float(5 * i)), WHITE, size=(90.0 + i, 70.0 + i))
        ctx.end_frame()

    frame()
    want = ctx.read_pixels()
    frame()
    ctx.remove_image(0)
    st = ctx.compact_atlas(1024)
    assert st["entries"] == 5 and np.array_equal(ctx.read_pixels(), want)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 10. keep off
def test_keep_off_a_growing_put_drops_every_entry():
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=256, device=0)
    for k in range(4):
        ctx.put_image(k, np.full((100, 100, 4), 9, np.uint8))
    ctx.put_image(9, np.full((100, 100, 4), 9, np.uint8))
    assert ctx.atlas_size() == 512 and not ctx.has_image(0) and ctx.has_image(9) and ctx.atlas_usage()["rebuilds"] == 1
    ctx.close()
