"""Exact damage readback on the GPU (include/figdraw_hip_exact.h, k_damage_filter): with the mode on, the tiles of a read are exactly the
bins in which the frame differs from what the receiver held -- computed here in numpy from a host mirror and fdh_read_pixels --, in
row-major order, whichever of the three reads is used; a fresh read returns the pending bins as with the mode off.  Everything here is
equality of bytes and of counts; no count is fixed but 0 for a frame that did not change and the grid's size for a first read."""
import threading

import numpy as np
import pytest

import ref_scenes as RS
from figdraw_amd.context import FigdrawHipError, HipContext
from figdraw_amd.scene import rect
from figdraw_amd.scenes import make_render_tree_100
from test_damage import REF, _imm, _scene
from test_damage_readback import SENTINEL, TILE, _box, _ctx, _exact, _mirror, _tiles_of
from test_damage_stream import _checked_read, _same_as_reference

INVALID = -1
KINDS = ("raw", "into", "coded")


def _bins_that_differ(a, b):
    """(bins_y, bins_x) bool: the bins in which two frames (h, w, 4) differ"""
    h, w = a.shape[:2]
    gy, gx = (h + 63) // 64, (w + 63) // 64
    d = np.zeros((gy * 64, gx * 64), bool)
    d[:h, :w] = (a != b).any(axis=2)
    return d.reshape(gy, 64, gx, 64).any(axis=(1, 3))


class _Receiver:
    """a context with damage readback and the exact mode on, and what a receiver holds: a host mirror that takes every read"""

    def __init__(self, w, h, kind="raw", route=None, tracking=True, exact=True):
        self.w, self.h, self.kind = w, h, kind
        self.grid = ((h + 63) // 64, (w + 63) // 64)
        self.nb = self.grid[0] * self.grid[1]
        self.ctx = _ctx(route, tracking)
        self.ctx.set_damage_exact(exact)
        self.mirror = _mirror(w, h)

    def resize(self, w, h):
        self.w, self.h = w, h
        self.grid = ((h + 63) // 64, (w + 63) // 64)
        self.nb = self.grid[0] * self.grid[1]
        self.mirror = _mirror(w, h)

    def read(self, what, fresh=None, pending=None, exact=True):
        """one read of self.kind, checked; -> the number of tiles.  fresh: the bins (a mask, or True for every bin) a fresh read must
        return, which are the pending ones; else the read must return the bins in which the mirror differs from the frame.  pending:
        the mask the filter started from, when the caller knows it.  exact=False: the mode is off, `fresh` is the pending set."""
        ctx, w, h = self.ctx, self.w, self.h
        now = ctx.read_pixels()
        if fresh is not None:
            want = np.ones(self.grid, bool) if fresh is True else fresh
        else:
            want = _bins_that_differ(self.mirror, now)
        rects = _tiles_of(want, w, h)
        if self.kind == "raw":
            tiles, pixels, full = ctx.read_damage()
            assert np.array_equal(tiles, rects), f"{what}: {len(tiles)} tiles, {len(rects)} bins changed; the tiles are not those bins in row-major order"
            assert pixels.shape == (len(tiles), TILE, TILE, 4)
            for (x, y, tw, th), px in zip(tiles, pixels):
                assert not px[th:].any() and not px[:, tw:].any(), f"{what}: slot bytes past the tile's edge are not zero (tile at {x}, {y})"
            HipContext.apply_damage(self.mirror, tiles, pixels)
            n = len(tiles)
        elif self.kind == "into":
            n = ctx.read_damage_into(self.mirror)
            assert n == len(rects), f"{what}: {n} tiles, {len(rects)} bins changed"
            full = n == self.nb
        else:
            tiles, payload, full = _checked_read(ctx, rects, what)
            _same_as_reference(tiles, payload, now, what)
            HipContext.decode_damage(self.mirror, tiles, payload)
            n = len(tiles)
        assert full == (n == self.nb), what
        _exact(ctx, self.mirror, what)
        if exact:
            n_pending, n_changed, was_fresh = ctx.damage_exact_stats()
            assert (n_changed, was_fresh) == (n, fresh is not None and n > 0), f"{what}: stats {(n_pending, n_changed, was_fresh)}, {n} tiles"
            assert n <= n_pending <= self.nb, f"{what}: stats {(n_pending, n_changed, was_fresh)}"
            if pending is not None:
                assert n_pending == int(np.asarray(pending).sum()), f"{what}: {n_pending} bins were pending, expected {int(np.asarray(pending).sum())}"
            if fresh is not None:
                assert n_pending == n
        return n

    def close(self):
        self.ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 1. tracking off
def _tree(w, h, **kw):
    return lambda ctx: ctx.render_frame(make_render_tree_100(float(w), float(h), **kw), w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["rgb_boxes_sdf", "backdrop_blur", "bench tree"])
def test_tracking_off_the_same_frame_twice(kind, case):
    """without the mode the second read returns every bin (test_readback_with_tracking_off); with it, none"""
    w, h = (1920, 1080) if case == "bench tree" else (640, 480)
    frame = _tree(w, h, frame=0) if case == "bench tree" else _scene(getattr(RS, case), w, h)
    r = _Receiver(w, h, kind, tracking=False)
    try:
        with pytest.raises(FigdrawHipError) as e:  # no read yet
            r.ctx.damage_exact_stats()
        assert e.value.code == INVALID
        frame(r.ctx)
        assert r.read("first", fresh=True) == r.nb
        for i in range(2):
            frame(r.ctx)
            assert r.read(f"the same frame again ({i})", pending=np.ones(r.grid, bool)) == 0
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the bench tree
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("ffb", [False, True])
def test_bench_tree_moved_roots_then_frames(kind, route, ffb):
    w, h = 1920, 1080
    r = _Receiver(w, h, kind, route)
    try:
        sc = make_render_tree_100(float(w), float(h), frame=0, full_frame_blur=ffb)
        lst = next(iter(sc.layers.values()))
        r.ctx.render_frame(sc, w, h)
        assert r.read("first", fresh=True) == r.nb
        for k in (1, 2, 3):  # the roots test_skipped_reads_bench_tree moves, moved as it moves them
            node = lst.nodes[lst.rootIds[len(lst.rootIds) * k // 4]]
            x, y, bw, bh = node.screenBox
            node.screenBox = rect(x + 3.0, y + 2.0, bw, bh)
            r.ctx.render_frame(sc, w, h)
            tracked = r.ctx.damage_bins()
            n = r.read(f"root {k}/4 moved", pending=tracked)
            print(f"full_frame_blur={ffb} route {route} {kind}: root {k}/4 moved: {n} bins changed, tracking reports {int(tracked.sum())} of {r.nb}")
            if ffb:
                assert tracked.all() and n < r.nb, f"root {k}/4: {n} tiles of {r.nb} while fdh_damage_bins reports every bin"
        counts = []
        for i, k in enumerate((0, 1, 2, 2, 3)):
            _tree(w, h, frame=k, full_frame_blur=ffb)(r.ctx)
            counts.append(r.read(f"frame {k} (read {i})", pending=r.ctx.damage_bins()))
        assert counts[3] == 0, "frame 2 again"
        print(f"full_frame_blur={ffb} route {route} {kind}: frames 0, 1, 2, 2, 3: {counts} bins changed of {r.nb}")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------ 3. A, B, A
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_an_edit_undone_before_the_read(kind):
    w, h = 700, 500
    r = _Receiver(w, h, kind)
    try:
        _imm(w, h, _box(40))(r.ctx)
        assert r.read("A", fresh=True) == r.nb
        _imm(w, h, _box(200))(r.ctx)
        _imm(w, h, _box(40))(r.ctx)
        assert r.read("A, B, A") == 0
        assert r.ctx.damage_exact_stats()[0] > 0, "tracking had bins pending: the filter dropped them"
        _imm(w, h, _box(200))(r.ctx)  # ... and the edit itself
        n = r.read("B")
        assert 0 < n <= r.ctx.damage_exact_stats()[0] < r.nb
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------ 4. what forces a full frame
@pytest.mark.gpu
def test_frames_rendered_in_full_read_as_what_changed():
    w, h = 320, 240
    img_a = np.zeros((32, 32, 4), np.uint8); img_a[..., 0] = 255; img_a[..., 3] = 255
    img_b = img_a.copy(); img_b[8:24, 8:24, 1] = 255
    r = _Receiver(w, h)
    ctx, every = r.ctx, np.ones(r.grid, bool)
    try:
        ctx.put_image(7, img_a)
        draw = _imm(w, h, lambda c: (c.draw_rect((0, 0, 40, 40), (0, 0, 0, 255)), c.draw_image(7, (100.0, 80.0), [(255, 255, 255, 255)] * 4, (32.0, 32.0))))
        draw(ctx)
        assert r.read("first", fresh=True) == r.nb
        # fdh_update_image between frames
        ctx.update_image(7, img_b)
        draw(ctx)
        assert ctx.damage_bins().all()
        n = r.read("after fdh_update_image", pending=every)
        assert 0 < n < r.nb and (r.mirror[88:104, 108:124, 1] == 255).all()
        draw(ctx)
        assert r.read("after fdh_update_image, unchanged") == 0
        # a frame that does not clear (an opaque rectangle on pixel edges: drawing it twice leaves the pixels of drawing it once)
        over = _imm(w, h, lambda c: c.draw_rect((200, 150, 50, 50), (0, 0, 255, 255)), clear=False)
        over(ctx)
        assert ctx.damage_bins().all()
        assert 0 < r.read("no clear", pending=every) < r.nb
        over(ctx)
        assert ctx.damage_bins().all()
        assert r.read("no clear, unchanged", pending=every) == 0
        # an untracked frame between tracked ones
        draw(ctx)
        assert 0 < r.read("cleared again") < r.nb
        ctx.set_damage_tracking(False)
        draw(ctx)
        assert r.read("untracked, unchanged", pending=every) == 0
        ctx.set_damage_tracking(True)
        draw(ctx)  # the first tracked frame after it is a full one
        assert ctx.damage_bins().all()
        assert r.read("tracked again, unchanged", pending=every) == 0
        # a change of clear colour
        tinted = _imm(w, h, lambda c: c.draw_rect((0, 0, 40, 40), (0, 0, 0, 255)), color=(0.9, 1.0, 1.0, 1.0))
        tinted(ctx)
        assert ctx.damage_bins().all()
        assert r.read("another clear colour", pending=every) == r.nb
        tinted(ctx)
        assert r.read("another clear colour, unchanged") == 0
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------ 5. the mode's life
@pytest.mark.gpu
def test_mode_on_off_on_and_readback_off_on():
    w, h = 700, 500
    r = _Receiver(w, h, exact=False)
    ctx = r.ctx
    a, b = _imm(w, h, _box(40)), _imm(w, h, _box(200))
    try:
        a(ctx)
        assert r.read("mode off", fresh=True, exact=False) == r.nb
        with pytest.raises(FigdrawHipError) as e:
            ctx.damage_exact_stats()
        assert e.value.code == INVALID
        # on with an empty pending set: a read with nothing pending fills nothing, the next one with a pending bin is the fresh one
        ctx.set_damage_exact(True)
        assert r.read("on, nothing pending", fresh=np.zeros(r.grid, bool)) == 0
        b(ctx)
        tracked = ctx.damage_bins()
        assert 0 < r.read("on: the fresh read is the pending set", fresh=tracked) == tracked.sum() < r.nb
        a(ctx); b(ctx)
        assert r.read("A, B, A, B") == 0
        a(ctx)
        assert 0 < r.read("A") < r.nb
        ctx.set_damage_exact(True)  # already on: nothing is reset
        a(ctx)
        assert r.read("still on") == 0
        # off: reads are the pending set again; the receiver moves on to B while no device mirror follows
        ctx.set_damage_exact(False)
        b(ctx)
        tracked = ctx.damage_bins()
        assert r.read("off", fresh=tracked, exact=False) == tracked.sum() > 0
        a(ctx)
        tracked = ctx.damage_bins()
        b(ctx)
        tracked = tracked | ctx.damage_bins()
        assert r.read("off: B, A, B is a pending set", fresh=tracked, exact=False) == tracked.sum() > 0
        # on again, and the frame goes back to A, which is what the mirror held when the mode was turned off: a stale mirror would drop it
        ctx.set_damage_exact(True)
        a(ctx)
        tracked = ctx.damage_bins()
        assert 0 < r.read("on again: fresh", fresh=tracked) == tracked.sum()
        b(ctx); a(ctx)
        assert r.read("on again: A, B, A") == 0
        # a refused read leaves the set and the mirror as they were
        b(ctx)
        with pytest.raises(FigdrawHipError) as e:
            ctx.read_damage_into(np.zeros((h, w + 1, 4), np.uint8))
        assert e.value.code == INVALID
        assert 0 < r.read("after a refused read") < r.nb
        # readback off and on: every bin is pending, and the read is fresh; then the frame the mirror held before
        ctx.set_damage_readback(False)
        a(ctx)
        ctx.set_damage_readback(True)
        with pytest.raises(FigdrawHipError) as e:
            ctx.damage_exact_stats()
        assert e.value.code == INVALID
        a(ctx)
        r.mirror[:] = SENTINEL
        assert r.read("readback on again", fresh=True) == r.nb
        b(ctx)
        assert 0 < r.read("B") < r.nb
        b(ctx)
        assert r.read("B again") == 0
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_frame_size_change(kind):
    w, h = 700, 500
    r = _Receiver(w, h, kind)
    ctx = r.ctx
    try:
        _imm(w, h, _box(40))(ctx)
        assert r.read("first", fresh=True) == r.nb
        for w2, h2 in ((690, 490), (737, 489), (700, 500)):  # the same bin grid, another one, and back
            _imm(w2, h2, _box(40))(ctx)
            r.resize(w2, h2)
            assert r.read(f"{w2} x {h2}", fresh=True) == r.nb
            _imm(w2, h2, _box(40))(ctx)
            assert r.read(f"{w2} x {h2}, unchanged") == 0
            _imm(w2, h2, _box(70))(ctx)
            assert 0 < r.read(f"{w2} x {h2}, the box moved") < 8
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", [(513, 389), (130, 70)])
@pytest.mark.parametrize("tracking", [False, True])
def test_clipped_sizes(kind, size, tracking):
    w, h = size
    r = _Receiver(w, h, kind, tracking=tracking)
    try:
        counts = []
        for i, s in enumerate((3, 3, 4, 5, 5, 6, 3)):
            r.ctx.render_frame(RS.random_scene(s, float(w), float(h), **({"n": 40} if w > 200 else {"n": 25, "clips": False, "blur": False})), w, h)
            counts.append(r.read(f"scene {s} (read {i})", fresh=True if i == 0 else None))
        assert counts[0] == r.nb and counts[1] == 0 and counts[4] == 0 and all(c > 0 for c in (counts[2], counts[3], counts[5], counts[6])), counts
        # one pixel in the last, clipped tile: the corner bin alone
        base = lambda c: c.draw_rect((10, 10, 30, 30), (255, 0, 0, 255))  # noqa: E731
        _imm(w, h, base)(r.ctx)
        assert r.read("a flat frame") > 0
        _imm(w, h, lambda c: (base(c), c.draw_rect((w - 1, h - 1, 1, 1), (255, 0, 255, 255))))(r.ctx)
        before = r.mirror.copy()
        assert r.read("the last pixel") == 1
        assert (r.mirror[:h - 1] == before[:h - 1]).all() and (r.mirror[h - 1, w - 1] == (255, 0, 255, 255)).all()
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------ 7. mode off
@pytest.mark.gpu
def test_a_context_that_never_turns_the_mode_on():
    w, h = 513, 389
    ctx = _ctx(tracking=False)
    mirror = _mirror(w, h)
    try:
        for i in range(2):
            ctx.render_frame(RS.random_scene(3, float(w), float(h), n=40), w, h)
            tiles, pixels, full = ctx.read_damage()
            assert full and len(tiles) == 63, f"read {i}"
            HipContext.apply_damage(mirror, tiles, pixels)
            _exact(ctx, mirror, f"read {i}")
            with pytest.raises(FigdrawHipError) as e:
                ctx.damage_exact_stats()
            assert e.value.code == INVALID
        ctx.set_damage_exact(False)  # off while off: accepted, nothing happens
        ctx.render_frame(RS.random_scene(3, float(w), float(h), n=40), w, h)
        assert ctx.read_damage_into(mirror) == 63
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 8. threads
@pytest.mark.gpu
def test_four_contexts_on_four_threads_with_the_mode_on():
    w, h = 800, 600
    errors = []

    def work(j):
        try:
            ctx = _ctx(tracking=j % 2 == 0)
            ctx.set_damage_exact(True)
            mirror = _mirror(w, h)
            try:
                for k in range(20):
                    ctx.render_frame(make_render_tree_100(float(w), float(h), frame=(k // 2) + j, copies=20), w, h)
                    if k % 5 != 4:  # a skipped read now and then
                        now = ctx.read_pixels()
                        want = int(_bins_that_differ(mirror, now).sum())
                        n = ctx.read_damage_into(mirror)
                        if not np.array_equal(mirror, now):
                            errors.append(f"context {j}, frame {k}: the mirror differs")
                            return
                        if k > 0 and n != want:
                            errors.append(f"context {j}, frame {k}: {n} tiles, {want} bins changed")
                            return
                        if k % 2 == 1 and k % 5 != 0 and n != 0:  # the frame of the read before, again
                            errors.append(f"context {j}, frame {k}: an unchanged frame read as {n} tiles")
                            return
            finally:
                ctx.close()
        except Exception as e:  # noqa: BLE001
            errors.append(f"context {j}: {e!r}")

    threads = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors, errors
