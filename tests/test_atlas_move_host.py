"""Atlas compaction without a GPU (include_glyphs/figdraw_hip_atlas.h): the directory and the packer on record-only contexts -- placement
against a fresh context, transactions, keep mode, retained scenes --, the move tables and k_atlas_move's source under a host shim
(tests/atlas_move_emu, plain and under AddressSanitizer + UBSan) against a numpy restatement, and the C99 smoke."""
import os
import struct
import subprocess

import numpy as np
import pytest

import atlas_move_cases as AC
import emu_build
from figdraw_amd import context
from figdraw_amd.context import HipContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, ATLAS_FULL = -1, None  # (ATLAS_FULL is read from the header below)
WHITE = [(255, 255, 255, 255)] * 4


def _status(name):
    for line in open(os.path.join(ROOT, "include", "figdraw_hip.h")):
        if name in line and "=" in line:
            return int(line.split("=")[1].split(",")[0].split("/")[0].strip())
    raise AssertionError(name)


ATLAS_FULL = _status("FDH_ERR_ATLAS_FULL")


def _random_entries(seed, n=40):
    """entries of every single put kind with sizes 1..48 (tests/test_atlas_host.py's range), on a record-only context"""
    rng = np.random.default_rng(seed)
    out = []
    for key, (w, h) in enumerate(rng.integers(1, 49, size=(n, 2))):
        w, h = int(w), int(h)
        px = np.zeros((h, w, 4), np.uint8)
        px[h // 4:h - h // 4, w // 4:w - w // 4] = 255  # ink boxes smaller than the image
        kind = key % 6
        if kind == 0:
            out.append(AC.image(key, px))
        elif kind == 1:
            out.append(AC.glyph_image(key, px))
        elif kind == 2:
            out.append(AC.coverage(key, AC.box_outline(w, h), w, h))
        elif kind == 3:
            out.append(AC.field(key, AC.box_outline(w, h), w, h))
        elif kind == 4:
            out.append(AC.image_sdf(key, px, pad=1) if w <= 46 and h <= 46 else AC.image(key, px))
        else:
            levels, cw, ch = [px], w, h
            while cw > 1 and ch > 1:
                cw, ch = (cw + 1) // 2, (ch + 1) // 2
                levels.append(np.full((ch + 1, cw + 2, 4), 9, np.uint8))  # off-chain sizes
            out.append(AC.mips(key, levels))
    return out


def _frame_digest(ctx, entries):
    """a frame that draws every entry: 1:1, scaled, and as a field"""
    ctx.begin_frame(640, 480, True, (0.1, 0.2, 0.3, 1.0))
    for i, e in enumerate(entries):
        x, y = float(7 + 50 * (i % 12)), float(5 + 55 * (i // 12))
        if e.kind in ("field", "image sdf"):
            ctx.draw_msdf(e.key, (x, y), (0, 0, 0, 255), (e.w * 1.5, e.h * 1.5), 4.0, 0.5, 0.0, mtsdf=True)
        elif i % 3 == 0:
            ctx.draw_image(e.key, (x, y), WHITE, size=(e.w * 0.6, e.h * 0.6))
        else:
            ctx.draw_image(e.key, (x, y), WHITE)
    ctx.end_frame()
    return ctx.record_digest()


# ------------------------------------------------------------------------------------------------------------------ 1. placement
@pytest.mark.parametrize("seed,size", [(1, 0), (2, 0), (3, 512), (4, 128)])
def test_compaction_places_like_a_fresh_context(seed, size):
    entries = _random_entries(seed, 28 if size != 128 else 12)
    ctx = HipContext(atlas_size=256, record_only=True)
    for e in entries:
        e.single(ctx)
    assert ctx.atlas_size() == 256
    rng = np.random.default_rng(100 + seed)
    gone = set(int(k) for k in rng.choice(len(entries), size=len(entries) // 3, replace=False))
    for k in gone:
        ctx.remove_image(k)
    live = [e for e in entries if e.key not in gone]
    before = ctx.atlas_usage()
    st = ctx.compact_atlas(size)
    want_size = size or 256
    fresh = AC.fresh_context(live, want_size, record_only=True)
    assert ctx.atlas_size() == want_size == st["size_after"] and st["size_before"] == 256
    assert AC.rects(ctx, live) == AC.rects(fresh, live)
    assert all(not ctx.has_image(k) for k in gone)
    u, f = ctx.atlas_usage(), fresh.atlas_usage()
    assert (u["packed_area"], u["used_area"], u["entries"]) == (f["packed_area"], f["used_area"], f["entries"])
    assert st["packed_before"] == before["packed_area"] and st["packed_after"] == u["packed_area"] and st["entries"] == len(live)
    assert st["launches"] == 0 and u["epoch"] > before["epoch"] and u["compactions"] == 1
    if size == 0:
        assert u["packed_area"] < before["packed_area"], "removed entries left room"
    assert _frame_digest(ctx, live) == _frame_digest(fresh, live)  # positions, sizes and ink boxes as the records see them
    ctx.close(); fresh.close()


# ------------------------------------------------------------------------------------------------------------------ 2. transactions, modes
def test_a_compaction_that_does_not_fit_changes_nothing_and_bad_sizes_are_refused():
    entries = _random_entries(7, 30)
    ctx = HipContext(atlas_size=256, record_only=True)
    for e in entries:
        e.single(ctx)
    before, rects = ctx.atlas_usage(), AC.rects(ctx, entries)
    rc = ctx.L.fdh_compact_atlas(ctx.h, 64, None)
    assert rc == ATLAS_FULL, ctx.L.fdh_last_error()
    assert ctx.atlas_usage() == before and AC.rects(ctx, entries) == rects and ctx.atlas_size() == 256
    for bad in (-1, -256, 16385, 1 << 20):
        assert ctx.L.fdh_compact_atlas(ctx.h, bad, None) == INVALID
    assert ctx.atlas_usage() == before
    assert ctx.L.fdh_image_rect(ctx.h, 999, (context.C.c_int * 4)()) == INVALID
    ctx.close()


def test_keep_off_is_the_growth_of_old():
    ctx = HipContext(atlas_size=256, record_only=True)
    assert not ctx.atlas_keep()
    for k in range(4):
        ctx.put_image(k, np.zeros((100, 100, 4), np.uint8))
    assert ctx.atlas_size() == 256 and ctx.atlas_usage()["rebuilds"] == 0
    rect = ctx.put_image(9, np.zeros((100, 100, 4), np.uint8))  # does not fit: the atlas doubles and drops every entry
    u = ctx.atlas_usage()
    assert ctx.atlas_size() == 512 and rect == (4, 4, 100, 100) and not any(ctx.has_image(k) for k in range(4))
    assert (u["rebuilds"], u["compactions"], u["entries"]) == (1, 0, 1)
    ctx.reset_atlas()
    assert ctx.atlas_usage()["rebuilds"] == 2 and ctx.atlas_usage()["entries"] == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 3. keep mode
def test_keep_mode_grows_with_every_key_and_repacks_where_removals_left_room():
    ctx = HipContext(atlas_size=256, record_only=True)
    ctx.set_atlas_keep(True)
    assert ctx.atlas_keep()
    imgs = [AC.image(k, np.zeros((100, 100, 4), np.uint8)) for k in range(4)] + [AC.image(4, np.zeros((20, 30, 4), np.uint8))]
    for e in imgs:
        e.single(ctx)
    assert ctx.atlas_size() == 256 and ctx.atlas_usage()["compactions"] == 0
    extra = AC.image(9, np.zeros((100, 100, 4), np.uint8))
    extra.single(ctx)  # S' = 2S: live content needs it
    assert ctx.atlas_size() == 512 and all(ctx.has_image(e.key) for e in imgs + [extra])
    u = ctx.atlas_usage()
    assert (u["compactions"], u["rebuilds"]) == (1, 0)
    # the same atlas as compaction to 512 followed by the put, on a context without keep
    ref = HipContext(atlas_size=256, record_only=True)
    for e in imgs:
        e.single(ref)
    ref.compact_atlas(512)
    extra.single(ref)
    assert AC.rects(ctx, imgs + [extra]) == AC.rects(ref, imgs + [extra])
    ref.close(); ctx.close()
    # S' = S: two of four are removed, the skyline stays up, the fifth image fits only after a repack
    ctx = HipContext(atlas_size=256, record_only=True)
    ctx.set_atlas_keep(True)
    for e in imgs[:4]:
        e.single(ctx)
    ctx.remove_image(1); ctx.remove_image(2)
    extra.single(ctx)
    assert ctx.atlas_size() == 256 and [ctx.has_image(k) for k in (0, 1, 2, 3, 9)] == [True, False, False, True, True]
    assert ctx.atlas_usage()["compactions"] == 1 and ctx.atlas_usage()["rebuilds"] == 0
    ctx.close()


def test_a_batch_in_keep_mode_compacts_once_and_is_the_batch_after_a_compaction():
    rng = np.random.default_rng(3)
    first = [AC.image(k, np.zeros((int(h), int(w), 4), np.uint8)) for k, (w, h) in enumerate(rng.integers(20, 60, size=(12, 2)))]
    items = [(100 + i, *AC.glyph(code)) for i, code in enumerate(list(range(48, 91)) * 3)]  # 129 glyphs: not in what a 256 atlas has left
    keep, ref = HipContext(atlas_size=256, record_only=True), HipContext(atlas_size=256, record_only=True)
    keep.set_atlas_keep(True)
    for c in (keep, ref):
        for e in first:
            e.single(c)
        assert c.atlas_size() == 256
    got = keep.put_glyph_outlines(items)
    size = keep.atlas_size()
    assert size >= 512 and keep.atlas_usage()["compactions"] == 1 and keep.atlas_usage()["rebuilds"] == 0
    assert keep.glyph_batch_stats()["dropped_by_growth"] == 0 and all(keep.has_image(e.key) for e in first)
    ref.compact_atlas(size)
    assert ref.put_glyph_outlines(items) == got and ref.atlas_size() == size and ref.atlas_usage()["rebuilds"] == 0
    keys = [e.key for e in first] + [it[0] for it in items]
    assert [keep.image_rect(k) for k in keys] == [ref.image_rect(k) for k in keys]

    def digest(c):
        c.begin_frame(640, 480, True, (1, 1, 1, 1))
        for i, k in enumerate(keys):
            c.draw_image(k, (float(5 + 22 * (i % 28)), float(5 + 40 * (i // 28))), WHITE)
        c.end_frame()
        return c.record_digest()
    assert digest(keep) == digest(ref)
    # the size is the smallest that takes the live entries and the batch: at half of it the batch grows the atlas
    small = HipContext(atlas_size=256, record_only=True)
    for e in first:
        e.single(small)
    small.compact_atlas(size // 2)
    small.put_glyph_outlines(items)
    assert small.atlas_usage()["rebuilds"] > 0
    for c in (keep, ref, small):
        c.close()


def test_keep_mode_at_the_largest_size_reports_a_full_atlas_where_it_always_did():
    """nine 4096 x 4096 outlines fill a 16384 atlas; the tenth finds no size: the atlas is compacted to 16384 and the placement throws"""
    ctx = HipContext(atlas_size=16384, record_only=True)
    ctx.set_atlas_keep(True)
    ctx.put_image(1, np.zeros((10, 10, 4), np.uint8))
    out = (context.C.c_int * 4)()
    big = AC.box_outline(4096, 4096)  # (an outline put: nobody reads the texels of an image that large)
    for k in range(9):
        assert ctx.L.fdh_put_glyph_outline(ctx.h, 10 + k, 4096, 4096, big.ctypes.data, 4, 0, out) == 0
    assert ctx.atlas_usage()["compactions"] == 0
    assert ctx.L.fdh_put_glyph_outline(ctx.h, 99, 4096, 4096, big.ctypes.data, 4, 0, out) == ATLAS_FULL
    u = ctx.atlas_usage()
    assert (u["size"], u["entries"], u["compactions"], u["rebuilds"]) == (16384, 10, 1, 0) and ctx.has_image(1) and not ctx.has_image(99)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 4. retained scenes
def test_a_retained_scene_is_rebuilt_after_a_compaction():
    import ref_scenes as RS
    from figdraw_amd.scene import Fig, FigKind, RenderList, Renders

    def tree():
        lst = RenderList()
        lst.addRoot(Fig(kind=RS.RECT, screenBox=RS.rect(0, 0, 300, 200), fill=RS.rgba(40, 40, 40, 255)))
        for i, key in enumerate((1, 2, 3)):
            lst.addRoot(Fig(kind=FigKind.nkImage, screenBox=RS.rect(10 + 90 * i, 20, 60 + 10 * i, 50), image_id=key))
        lst.addRoot(Fig(kind=FigKind.nkMtsdfImage, screenBox=RS.rect(30, 100, 80, 80), image_id=4, image_fill=RS.fill(RS.rgba(0, 0, 0, 255)), pxRange=4.0, sdThreshold=0.5))
        out = Renders()
        out.layers[0] = lst
        return out

    def puts(c):
        c.put_image(7, np.zeros((90, 90, 4), np.uint8))  # (removed below: the others move left)
        for key, (w, h) in zip((1, 2, 3), ((40, 30), (28, 44), (64, 20))):
            px = np.zeros((h, w, 4), np.uint8); px[3:-3, 5:-5] = 200
            c.put_image(key, px)
        c.put_glyph_outline(4, AC.box_outline(32, 32), 32, 32, mtsdf=True)
        c.remove_image(7)

    ctx = HipContext(atlas_size=256, record_only=True)
    puts(ctx)
    ctx.scene_retain(tree(), 300, 200)
    old = ctx.record_digest()
    ctx.scene_render()
    assert ctx.record_digest() == old and ctx.scene_stats()[1] > 0  # the second frame came from cached roots
    ctx.compact_atlas(0)
    ctx.scene_render()
    retained = ctx.record_digest()
    ctx.render_frame(tree(), 300, 200)
    assert retained == ctx.record_digest() != old, "the epoch must have invalidated the cached roots"
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 5. tables and kernel
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_atlas_move.hip and fdh_atlas_move.h compiled as plain C++ under the sequential shim of tests/emu with the driver of
    tests/atlas_move_emu -> the directory of ./emu and ./emu_san"""
    return emu_build.build(tmp_path_factory, "atlas_move_emu", ("k_atlas_move.hip", "fdh_atlas_move.h"), {"emu": (), "emu_san": emu_build.SAN}, opt="-O2")


def _levels(size):
    out = []
    while size >= 1 and len(out) < 14:
        out.append(size)
        size >>= 1
    return out


def _chain(x, y, w, h, n_levels):
    """the level rectangles of the chain (Atlas::each_level): (level, x, y, w, h)"""
    out, level = [], 0
    while w > 1 and h > 1 and level < n_levels:
        out.append((level, x, y, w, h))
        level, x, y, w, h = level + 1, x // 2, y // 2, (w + 1) // 2, (h + 1) // 2
    return out


def _move_case():
    """A layout by hand: (old position, new position, level sizes or None for the chain) per entry in compaction order, a 256 atlas into a
    128 one.  Rectangles: the painter's order of the destination."""
    entries = [
        # old x, y, new x, y, w, h, own level sizes
        (150, 4, 4, 4, 40, 24, [(40, 24), (30, 16), (10, 6)]),  # a mips entry whose level 1 (30 x 16 at (2, 2)) reaches into its neighbour's
        (10, 100, 52, 4, 17, 23, None),                       # odd sizes; level 1 at (26, 2) is 9 x 12: the mips entry's level 1 ends at 32
        (40, 60, 4, 70, 65, 20, None),                        # one texel wider than a 64-wide tile row
        (200, 200, 4, 40, 9, 19, None),                       # one texel wider than an 8-wide tile
        (100, 200, 16, 48, 17, 17, None),                     # x = 16, w = 17 and ...
        (130, 200, 41, 48, 20, 17, None),                     # ... its neighbour 8 texels on: they share a texel at level 4
        (3, 3, 80, 40, 1, 13, "level0"),                      # 1 x N: level 0 alone
        (7, 3, 90, 40, 13, 1, "level0"),                      # N x 1
    ]
    rects = []
    for ox, oy, nx, ny, w, h, own in entries:
        if own == "level0":
            rects.append((0, ox, oy, 0, nx, ny, w, h, 1))
        elif own:
            for l, (lw, lh) in enumerate(own):
                rects.append((l, ox >> l, oy >> l, l, nx >> l, ny >> l, lw, lh, 1))
        else:
            for (l, x, y, cw, ch), (_, sx, sy, _, _) in zip(_chain(nx, ny, w, h, 8), _chain(ox, oy, w, h, 9)):
                rects.append((l, sx, sy, l, x, y, cw, ch, 1))
    return 256, 128, rects


def _restate(from_levels, to_sizes, rects, buf_in, out_words):
    """the move in numpy: the rectangles painted in order"""
    to = [np.zeros((s, s), np.uint32) for s in to_sizes]
    buf_out = np.full(out_words, 0xEEEEEEEE, np.uint32)
    for sl, sx, sy, dl, dx, dy, w, h, copy in rects:
        if sl < 0:
            src = buf_in[sx:sx + w * h].reshape(h, w)
        else:
            src = from_levels[sl][sy:sy + h, sx:sx + w]
        if not copy:
            src = None
        if dl < 0:
            buf_out[dx:dx + w * h] = src.reshape(-1)
        elif src is not None:
            to[dl][dy:dy + h, dx:dx + w] = src
        else:
            to[dl][dy:dy + h, dx:dx + w] = 0xFFFFFFFF  # somebody else's texels: marked, and taken out of the comparison
    return to, buf_out


def _run(shim, exe, from_size, to_size, from_levels, rects, buf_in, out_words):
    with open(os.path.join(shim, "case.bin"), "wb") as f:
        f.write(struct.pack("<5i", from_size, to_size, len(rects), len(buf_in), out_words))
        for lv in from_levels:
            f.write(lv.tobytes())
        f.write(buf_in.tobytes())
        for r in rects:
            f.write(struct.pack("<9i", *r))
    r = subprocess.run([exe, "case.bin", "out.bin"], cwd=shim, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (exe, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    raw = np.fromfile(os.path.join(shim, "out.bin"), np.uint32)
    to, at = [], 0
    for s in _levels(to_size):
        to.append(raw[at:at + s * s].reshape(s, s)); at += s * s
    said = dict(zip(r.stdout.split()[0::2], (int(v) for v in r.stdout.split()[1::2])))
    return to, raw[at:at + out_words], said


@pytest.mark.parametrize("exe", ["./emu", "./emu_san"])
def test_tables_and_kernel_under_the_emulator(shim, exe):
    from_size, to_size, rects = _move_case()
    rng = np.random.default_rng(11)
    from_levels = [rng.integers(1, 0xFFFFFFFF, size=(s, s), dtype=np.uint32) for s in _levels(from_size)]  # (no zero: a texel left out shows)
    # the cases this test is about exist in this layout
    level1 = [r for r in rects if r[3] == 1]
    a, b = level1[0], level1[1]
    assert a[4] + a[6] > b[4] and a[5] + a[7] > b[5], "the mips entry's level 1 must reach into its neighbour's"
    deep = [r for r in rects if r[3] >= 4]
    shared = [(p, q) for i, p in enumerate(deep) for q in deep[i + 1:] if p[3] == q[3] and p[4] < q[4] + q[6] and q[4] < p[4] + p[6] and p[5] < q[5] + q[7] and q[5] < p[5] + p[7]]
    assert any(p[6] * p[7] > 0 and p[3] >= 4 for p, q in shared), "two glyphs must share a texel at level 4 or deeper"
    # one more record each way through the dense buffers: level 0 of an entry out, a kept level in
    buf_in = rng.integers(1, 0xFFFFFFFF, size=7 * 5 + 3, dtype=np.uint32)
    rects = rects + [(0, 40, 60, -1, 5, 0, 65, 20, 1), (-1, 3, 0, 2, 20, 25, 7, 5, 1), (2, 0, 0, 2, 24, 27, 6, 4, 0)]
    out_words = 5 + 65 * 20 + 2
    want, want_buf = _restate(from_levels, _levels(to_size), rects, buf_in, out_words)
    got, got_buf, said = _run(shim, exe, from_size, to_size, from_levels, rects, buf_in, out_words)
    assert said["records"] == len([r for r in rects if r[8]]) and said["owner_level"] == 1 and said["owner_words"] > 0
    assert said["tiles"] == said["workgroups"] > 0
    for l, (g, w) in enumerate(zip(got, want)):
        theirs = w == 0xFFFFFFFF
        assert np.array_equal(g[~theirs], w[~theirs]), f"level {l}"
        assert not g[theirs].any(), f"level {l}: a texel of a rectangle that is not copied was written"
    assert np.array_equal(got_buf, want_buf)


def test_atlas_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "atlas_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_glyphs"),
                           os.path.join(ROOT, "tests", "atlas_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "atlas_abi_smoke: OK" in r.stdout
