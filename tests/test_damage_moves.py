"""Moved damage readback on the GPU (include_readback/figdraw_hip_moves.h; k_damage_move_match, k_damage_encode_moved, k_damage_move_votes):
what fdh_read_damage_moved returns is, byte for byte, what tests/tilemove_ref.py makes of (the previous fdh_read_pixels, the new one, the
moves); a host mirror that takes every read through fdh_decode_damage_moved stays fdh_read_pixels; and fdh_find_damage_moves returns the
reference's candidates and votes.  Everything here is equality of bytes and of counts.  Scenes are drawn through the C ABI: rectangles,
gradient quads and glyph images on a solid ground, at whole-pixel positions, so that a scroll moves pixels exactly."""
import os

import numpy as np
import pytest

import tilecode_ref as T
import tilemove_ref as M
from figdraw_amd.context import FigdrawHipError, HipContext
from figdraw_amd.scenes import load_glyph_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
GROUND = (0.9, 0.92, 0.95, 1.0)
WHITE = [(255, 255, 255, 255)] * 4
# the issue's scrolls as moves (tile (x, y) now holds what (x + dx, y + dy) held): up by 17, down by 64, sideways by 5, a diagonal
MOVES = {"up 17": (0, 17), "down 64": (0, -64), "sideways 5": (5, 0), "diagonal": (3, -9)}
SIZES = [(131, 70), (256, 192)]  # clipped bins and W & 3 != 0; three by four whole bins
# every scroll at every size -- but a frame 70 rows high has no tile whose source 17 rows further down is inside it: that scroll runs at
# 131 x 150 instead (clipped bins and W & 3 != 0 as well)
CASES = [(name, size) for size in SIZES for name in MOVES if (name, size) != ("up 17", (131, 70))] + [("up 17", (131, 150))]


def _glyphs():
    images = load_glyph_fixture(os.path.join(ROOT, "tests", "golden", "glyphs_ubuntu20.npz"))
    return {k: images[k] for k in range(1000 + 65, 1000 + 91)}  # coverage glyphs A .. Z


def _items(w, h, seed=4):
    """a page much larger than the frame, so that whatever scrolls in is content too: (kind, x, y, ...) at whole-pixel positions, dense
    enough that no bin of any view is one colour"""
    rng = np.random.RandomState(seed)
    items = []
    for y in range(-160, h + 160, 14):
        for x in range(-160, w + 160, 24):
            kind = rng.randint(0, 8)
            col = tuple(int(v) for v in rng.randint(0, 256, 3)) + (255,)
            if kind < 4:
                items.append(("rect", x + int(rng.randint(0, 6)), y + int(rng.randint(0, 4)), int(rng.randint(4, 20)), int(rng.randint(3, 11)), col))
            elif kind < 7:
                items.append(("glyph", x + int(rng.randint(0, 6)), y, 1000 + 65 + int(rng.randint(0, 26))))
            else:
                col2 = tuple(int(v) for v in rng.randint(0, 256, 3)) + (255,)
                items.append(("gradient", x, y, 20, 10, col, col2))
    return items


def _frame(ctx, w, h, items, glyphs, sx=0, sy=0, blur=None):
    """the page scrolled by (sx, sy): page pixel (x, y) is drawn at (x - sx, y - sy)"""
    ctx.begin_frame(w, h, True, GROUND)
    for it in items:
        x, y = it[1] - sx, it[2] - sy
        if it[0] == "rect":
            ctx.draw_rect((x, y, it[3], it[4]), it[5])
        elif it[0] == "glyph":
            g = glyphs[it[3]]
            ctx.draw_image(it[3], (float(x), float(y)), WHITE, (float(g.shape[1]), float(g.shape[0])))
        else:
            bw, bh = it[3], it[4]
            ctx.draw_filled_quad((x, y, x + bw, y, x + bw, y + bh, x, y + bh), [it[5], it[6], it[6], it[5]])
    if blur is not None:
        ctx.draw_backdrop_blur(blur, (6.0,) * 4, (6.0,) * 4, 5.0)
    ctx.end_frame()


def _painted(w, h, items, sx, sy):
    """what the rectangles alone leave of that frame, in numpy: the CPU side's stand-in for the frame when a case's content is chosen"""
    px = np.zeros((h, w), np.uint32)
    for it in items:
        if it[0] == "rect":
            x, y = it[1] - sx, it[2] - sy
            c = it[5]
            px[max(y, 0):max(y + it[4], 0), max(x, 0):max(x + it[3], 0)] = c[0] | c[1] << 8 | c[2] << 16 | 0xFF000000
    return px


@pytest.mark.parametrize("name,size", CASES)
def test_the_chosen_content_gives_every_case_copies(name, size):
    """(no GPU) the rectangles of the page alone, painted in numpy: each case's reference COPY count is above zero"""
    w, h = size
    dx, dy = MOVES[name]
    items = _items(w, h)
    old, new = _painted(w, h, items, 0, 0), _painted(w, h, items, dx, dy)
    _, _, copied = M.encode_frame_moved(T.as_rgba(old), T.as_rgba(new), [(dx, dy)], T.tiles_of(w, h))
    assert copied > 0, (size, name)


class _Receiver:
    """a context with damage readback and exact mode on, and a host mirror that takes every read"""

    def __init__(self, w, h, tracking=True):
        self.w, self.h = w, h
        self.glyphs = _glyphs()
        self.ctx = HipContext(device=0)
        self.ctx.set_damage_tracking(tracking)
        self.ctx.set_damage_readback(True)
        self.ctx.set_damage_exact(True)
        for k, v in self.glyphs.items():
            self.ctx.put_image(k, v)
        self.items = _items(w, h)
        self.mirror = np.full((h, w, 4), 0xA5, np.uint8)

    def frame(self, sx=0, sy=0, blur=None):
        _frame(self.ctx, self.w, self.h, self.items, self.glyphs, sx, sy, blur)

    def resize(self, w, h):
        self.w, self.h = w, h
        self.mirror = np.full((h, w, 4), 0xA5, np.uint8)

    def grid(self):
        return (self.h + 63) // 64, (self.w + 63) // 64

    def differs(self, now):
        gy, gx = self.grid()
        d = np.zeros((gy * 64, gx * 64), bool)
        d[:self.h, :self.w] = (self.mirror != now).any(axis=2)
        return d.reshape(gy, 64, gx, 64).any(axis=(1, 3))

    def read_moved(self, what, moves, fresh=False, need_copies=False):
        """one moved read, held to the reference and decoded into the mirror -> (tiles, COPY tiles)"""
        ctx, w, h = self.ctx, self.w, self.h
        now = ctx.read_pixels()
        gy, gx = self.grid()
        want = self.differs(now) if fresh is False else np.ones((gy, gx), bool) if fresh is True else fresh  # (a mask: the fresh read's pending set)
        rects = [rc for rc, m in zip(T.tiles_of(w, h), want.reshape(-1)) if m]
        if fresh is not False:
            wdir, wblob = T.encode_frame(now, rects)
            wcopied = 0
        else:
            wdir, wblob, wcopied = M.encode_frame_moved(self.mirror, now, [tuple(m) for m in moves], rects)
        if need_copies:
            assert wcopied > 0, f"{what}: the reference finds no COPY tile in this case: the case shows nothing"
        tiles, payload, full, n_copied = ctx.read_damage_moved(moves)
        print(f"{what}: {len(tiles)} tiles, {n_copied} COPY, {24 * len(tiles) + len(payload)} bytes; without moves {T.wire_bytes(T.encode_frame(now, rects)[0])}")
        got = np.stack([tiles[f].astype(np.int32) for f in "xywh"], axis=1).reshape(-1, 4)
        assert np.array_equal(got, np.asarray(rects, np.int32).reshape(-1, 4)), f"{what}: the tiles are not the bins that changed, in row-major order"
        assert full == (len(tiles) == gx * gy) and n_copied == wcopied == int((tiles["mode"] == M.COPY).sum()), f"{what}: n_copied {n_copied}, the reference {wcopied}"
        assert len(payload) == len(wblob) == sum(T.ceil16(s) for s in tiles["size"].tolist()), what
        used = np.zeros(len(payload), bool)
        for a, b in zip(tiles, wdir):
            assert all(a[f] == b[f] for f in ("mode", "bits", "n", "size", "solid")), f"{what}: {a} against the reference's {b}"
            size, at, ref = int(a["size"]), int(a["offset"]), int(b["offset"])
            if size == 0:
                assert at == 0, what
                continue
            assert at % 16 == 0 and at + T.ceil16(size) <= len(payload) and not used[at:at + T.ceil16(size)].any(), what
            used[at:at + T.ceil16(size)] = True
            assert payload[at:at + size] == wblob[ref:ref + size], f"{what}: the payload of {a}"
            assert not any(payload[at + size:at + T.ceil16(size)]), what
        assert used.all(), what
        HipContext.decode_damage_moved(self.mirror, tiles, payload)
        assert np.array_equal(self.mirror, now), f"{what}: the mirror is not fdh_read_pixels"
        return len(tiles), n_copied

    def close(self):
        self.ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the reads
@pytest.mark.gpu
@pytest.mark.parametrize("tracking", [True, False])
@pytest.mark.parametrize("name,size", CASES)
def test_moved_reads_are_byte_exact_against_the_reference(name, size, tracking):
    w, h = size
    dx, dy = MOVES[name]
    r = _Receiver(w, h, tracking)
    try:
        r.frame()
        n, c = r.read_moved("first", [(dx, dy)], fresh=True)
        assert (n, c) == (r.grid()[0] * r.grid()[1], 0)
        r.frame(dx, dy)
        # the mover first: it changes nothing.  The pending set is the frame's damage, or every bin without tracking
        pending = r.ctx.damage_bins() if tracking else np.ones(r.grid(), bool)
        want = M.find_moves(r.mirror, r.ctx.read_pixels(), pending, 64)
        moves, votes = r.ctx.find_damage_moves(64, 8)
        assert [(tuple(int(v) for v in m), int(k)) for m, k in zip(moves, votes)] == want[:8], f"the mover: {moves.tolist()}, {votes.tolist()} against {want[:8]}"
        on_axis = [tuple(int(v) for v in m) for m in moves if (m[0] == 0) == (dx == 0)]
        can_vote = name != "diagonal" and (w, h, name) != (131, 70, "down 64")  # (131 x 70 has no whole tile with row y0 + 32 - 64 in the frame)
        if can_vote:
            assert on_axis and on_axis[0] == (dx, dy), f"the mover's first candidate on the scroll's axis is {on_axis[0]}, the scroll was {(dx, dy)}"
            hint = [tuple(int(v) for v in m) for m in moves[:2]]
            assert (dx, dy) in hint
        else:
            hint = [(dx, dy)]  # no probe sees this one: the application says it
        n, c = r.read_moved(f"{name} at {w} x {h}, tracking {tracking}", hint, need_copies=True)
        assert 0 < c <= n
        assert r.read_moved("again", hint) == (0, 0)
    finally:
        r.close()


@pytest.mark.gpu
def test_one_bin_has_no_source_inside_the_frame():
    r = _Receiver(64, 64)
    try:
        r.frame()
        assert r.read_moved("first", [], fresh=True) == (1, 0)
        r.frame(0, 9)
        moves, votes = r.ctx.find_damage_moves(32, 4)
        assert len(moves) and tuple(moves[0]) == (0, 9), "the mover still sees the scroll"
        assert r.read_moved("64 x 64 scrolled", [(0, 9), (0, -9), (1, 0)]) == (1, 0)
    finally:
        r.close()


@pytest.mark.gpu
def test_no_moves_is_the_coded_read_of_a_twin_context():
    w, h = 256, 192
    a, b = _Receiver(w, h), _Receiver(w, h)
    try:
        for step, (sx, sy) in enumerate(((0, 0), (0, 17), (0, 17), (4, 30))):
            a.frame(sx, sy); b.frame(sx, sy)
            ta, pa, fa, ca = a.ctx.read_damage_moved([])
            tb, pb, fb = b.ctx.read_damage_coded()
            assert ca == 0 and fa == fb and len(pa) == len(pb) and len(ta) == len(tb), step
            for x, y in zip(ta, tb):  # (payloads lie in the order the workgroups claimed their space: compared tile by tile)
                assert all(x[f] == y[f] for f in ("x", "y", "w", "h", "mode", "bits", "n", "size", "solid")), step
                assert pa[int(x["offset"]):int(x["offset"]) + int(x["size"])] == pb[int(y["offset"]):int(y["offset"]) + int(y["size"])], step
            assert a.ctx.damage_exact_stats() == b.ctx.damage_exact_stats()
        assert len(ta) > 0
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ a chain of frames
@pytest.mark.gpu
@pytest.mark.parametrize("tracking", [True, False])
def test_a_chain_of_frames_through_the_decoder(tracking):
    w, h = 256, 192
    r = _Receiver(w, h, tracking)
    ctx = r.ctx
    try:
        r.frame()
        r.read_moved("first", [(0, 17)], fresh=True)
        r.frame(0, 17)
        assert r.read_moved("scroll", [(0, 17)], need_copies=True)[1] > 0
        r.frame(0, 0)
        assert r.read_moved("scroll back", [(0, 17), (0, -17)], need_copies=True)[1] > 0
        r.frame(0, 0)
        assert r.read_moved("unchanged", [(0, -17)]) == (0, 0)
        r.frame(0, 23, blur=(70.0, 40.0, 100.0, 60.0))
        n, c = r.read_moved("a blur node over scrolled content", [(0, 23)], need_copies=True)
        assert 0 < c < n, "the bins under the blur are not copies of anything"
        r.resize(200, 150)
        r.frame(0, 23)
        assert r.read_moved("resized: a fresh read", [(0, 23)], fresh=True) == (12, 0)
        r.frame(0, 40)
        assert r.read_moved("scroll after the resize", [(0, 17)], need_copies=True)[1] > 0
        # the other kinds of read in between: the mirror the device keeps follows them too
        r.frame(6, 40)
        tiles, pixels, _ = ctx.read_damage()
        HipContext.apply_damage(r.mirror, tiles, pixels)
        assert len(tiles) > 0 and np.array_equal(r.mirror, ctx.read_pixels())
        r.frame(6, 47)
        assert r.read_moved("after fdh_read_damage", [(0, 7)], need_copies=True)[1] > 0
        r.frame(1, 47)
        tiles, payload, _ = ctx.read_damage_coded()
        HipContext.decode_damage(r.mirror, tiles, payload)
        assert len(tiles) > 0 and np.array_equal(r.mirror, ctx.read_pixels())
        r.frame(1, 30)
        assert r.read_moved("after fdh_read_damage_coded", [(5, 0), (0, -17)], need_copies=True)[1] > 0
        r.frame(1, 30)
        assert r.read_moved("unchanged again", [(0, -17)]) == (0, 0)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_refusals_leave_the_pending_set_and_the_mirror_alone():
    w, h = 131, 70
    r = _Receiver(w, h)
    ctx = r.ctx
    try:
        with pytest.raises(FigdrawHipError) as e:  # before the first frame
            ctx.read_damage_moved([(0, 17)])
        assert e.value.code == INVALID
        r.frame()
        r.read_moved("first", [], fresh=True)
        r.frame(-2, 6)
        L = ctx.L
        one = np.array([(0, 17)], np.int16)
        bad = [ctx.L.fdh_read_damage_moved(ctx.h, one.ctypes.data, -1, None, None, None, None, None, None, None, None),
               ctx.L.fdh_read_damage_moved(ctx.h, one.ctypes.data, 9, None, None, None, None, None, None, None, None),
               ctx.L.fdh_read_damage_moved(ctx.h, None, 1, None, None, None, None, None, None, None, None),
               ctx.L.fdh_find_damage_moves(ctx.h, 0, None, None, 0, None), ctx.L.fdh_find_damage_moves(ctx.h, 257, None, None, 0, None),
               ctx.L.fdh_find_damage_moves(ctx.h, 8, None, None, -1, None), ctx.L.fdh_find_damage_moves(ctx.h, 8, None, None, 2, None)]
        assert bad == [INVALID] * len(bad), bad
        for moves in ([(0, 0)], [(0, 17), (0, 0)]):
            with pytest.raises(FigdrawHipError) as e:
                ctx.read_damage_moved(moves)
            assert e.value.code == INVALID and b"(0, 0)" in L.fdh_last_error()
        ctx.set_damage_exact(False)  # (drops the mirror: turned on again, the next read is a fresh one)
        for call in (lambda: ctx.read_damage_moved([(-2, 6)]), lambda: ctx.find_damage_moves(8, 2)):
            with pytest.raises(FigdrawHipError) as e:
                call()
            assert e.value.code == INVALID
        ctx.set_damage_exact(True)
        assert len(ctx.find_damage_moves(8, 2)[0]) == 0, "no valid mirror: the mover proposes nothing"
        n, c = r.read_moved("after the refusals", [(-2, 6)], fresh=ctx.damage_bins())
        assert c == 0 and n > 0, "the refused calls consumed nothing"
        r.frame(-4, 12)
        assert r.read_moved("and the moves work afterwards", [(-2, 6)], need_copies=True)[1] > 0
        assert len(ctx.find_damage_moves(8, 2)[0]) == 0, "nothing pending: the mover proposes nothing"
    finally:
        r.close()
