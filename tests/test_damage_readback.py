"""Damage readback (include/figdraw_hip_readback.h): a context keeps the bins composited since the application's last read and a read
moves only those to the host.  Everything here is equality of bytes: the feature copies pixels.  CPU tests pin the C ABI and the
host-only fdh_apply_damage; GPU tests hold a mirror that receives every read against fdh_read_pixels of the whole frame."""
import ctypes as C
import os
import random
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import ref_scenes as RS
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext
from figdraw_amd.scene import rect, rgba, fill
from figdraw_amd.scenes import make_non_clip_benchmark, make_render_tree_100
from test_damage import REF, _imm, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "figdraw_hip_readback.h")
NEW_API = ("fdh_set_damage_readback", "fdh_read_damage", "fdh_read_damage_into", "fdh_apply_damage")
INVALID, NO_DEVICE = -1, -2
TILE, PITCH, SLOT = 64, 256, 16384
SENTINEL = 0xA5


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_header_declares_and_library_exports_the_readback_api():
    src = open(HEADER).read()
    assert '#include "figdraw_hip.h"' in src
    declared = re.findall(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(", src)
    assert sorted(declared) == sorted(NEW_API)
    assert re.search(r"FDH_TILE_PX\s*=\s*64\b", src) and re.search(r"FDH_TILE_PITCH\s*=\s*256\b", src) and re.search(r"FDH_TILE_BYTES\s*=\s*16384\b", src)
    L = context.load()
    for name in NEW_API:
        assert hasattr(L, name), name
    for other in ("figdraw_hip.h", "figdraw_hip_damage.h", "figdraw_hip_pick.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(r"\b%s\b" % n, text) for n in NEW_API), other


def test_readback_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "readback_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "readback_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "readback_abi_smoke: OK" in r.stdout
    src = open(os.path.join(ROOT, "tests", "readback_abi_smoke.c")).read()
    assert all(re.search(r"\b%s\b" % n, src) for n in NEW_API)


def _pattern(k, h, w):
    """tile k's pixels: a byte per (tile, row, column, channel), never the sentinel"""
    r, c, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(4), indexing="ij")
    v = (k * 53 + r * 17 + c * 5 + ch * 3) % 160
    return v.astype(np.uint8)  # 0 .. 159: below SENTINEL (0xA5 = 165) and below the slots' filler (0xEE)


def _apply_case():
    """130 x 70: a 3 x 2 grid whose last column is 2 pixels wide and whose last row is 6 high; four of its six bins, row-major"""
    w, h = 130, 70
    bins = [(0, 0), (2, 0), (1, 1), (2, 1)]
    tiles = np.array([(64 * bx, 64 * by, min(64, w - 64 * bx), min(64, h - 64 * by)) for bx, by in bins], np.int32)
    slots = np.full((len(bins), TILE, TILE, 4), 0xEE, np.uint8)
    want = np.full((h, w, 4), SENTINEL, np.uint8)
    for k, (x, y, tw, th) in enumerate(tiles):
        slots[k, :th, :tw] = _pattern(k, th, tw)
        want[y:y + th, x:x + tw] = _pattern(k, th, tw)
    return w, h, tiles, slots, want


def test_apply_damage_known_answers():
    w, h, tiles, slots, want = _apply_case()
    assert tiles[1].tolist() == [128, 0, 2, 64] and tiles[2].tolist() == [64, 64, 64, 6] and tiles[3].tolist() == [128, 64, 2, 6]
    store = np.full((h, w + 9, 4), SENTINEL, np.uint8)  # a pitch of 4 (w + 9) bytes
    image = store[:, :w]
    HipContext.apply_damage(image, tiles, slots)
    assert np.array_equal(image, want)
    assert (store[:, w:] == SENTINEL).all(), "the pitch padding was written"
    assert not (image == 0xEE).any(), "bytes of a slot beyond the tile's w, h reached the image"
    # an empty list touches nothing and needs no arrays
    L = context.load()
    keep = store.copy()
    assert L.fdh_apply_damage(store.ctypes.data, store.strides[0], w, h, None, None, 0) == 0
    assert L.fdh_apply_damage(None, store.strides[0], w, h, None, None, 0) == 0
    HipContext.apply_damage(image, np.zeros((0, 4), np.int32), np.zeros((0, TILE, TILE, 4), np.uint8))
    assert np.array_equal(store, keep)


def test_apply_damage_refusals_leave_the_image_alone():
    w, h, tiles, slots, _ = _apply_case()
    L = context.load()
    store = np.full((h, w + 9, 4), SENTINEL, np.uint8)
    pitch, n = store.strides[0], len(tiles)

    def call(image=store.ctypes.data, pitch=pitch, t=tiles, px=slots.ctypes.data, n=n, tp=True):
        t = np.ascontiguousarray(t, np.int32)
        return L.fdh_apply_damage(image, pitch, w, h, t.ctypes.data if tp else None, px, n)

    assert call() == 0
    store[:] = SENTINEL
    assert call(image=None) == INVALID
    assert call(tp=False) == INVALID
    assert call(px=None) == INVALID
    assert call(n=-1) == INVALID
    assert call(pitch=4 * w - 1) == INVALID
    for col, bad in ((2, 0), (2, 65), (3, 0), (3, 65)):  # w, h outside 1 .. 64
        t = tiles.copy(); t[0, col] = bad
        assert call(t=t) == INVALID, (col, bad)
    for row, col, bad in ((0, 0, -1), (0, 1, -1), (1, 0, 129), (2, 1, 65), (3, 2, 3), (3, 3, 7)):  # not inside the image
        t = tiles.copy(); t[row, col] = bad
        assert call(t=t) == INVALID, (row, col, bad)
    # a bad LAST tile: the earlier ones must not have been copied
    t = tiles.copy(); t[3, 3] = 7
    assert call(t=t) == INVALID
    assert (store == SENTINEL).all(), "a refused call wrote into the image"
    assert b"tile" in L.fdh_last_error()


def test_record_only_context_refuses_readback():
    ctx = HipContext(record_only=True)
    with pytest.raises(FigdrawHipError) as e:
        ctx.set_damage_readback(True)
    assert e.value.code == INVALID
    ctx.set_damage_readback(False)
    with pytest.raises(FigdrawHipError) as e:
        ctx.read_damage()
    assert e.value.code == NO_DEVICE
    with pytest.raises(FigdrawHipError) as e:
        ctx.read_damage_into(np.zeros((8, 8, 4), np.uint8))
    assert e.value.code == NO_DEVICE
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ GPU
def _ctx(route=None, tracking=True, readback=True):
    c = HipContext(device=0)
    if route is not None:
        c.set_blur_route(route)
    c.set_damage_tracking(tracking)
    c.set_damage_readback(readback)
    return c


def _mirror(w, h):
    return np.full((h, w, 4), SENTINEL, np.uint8)


def _tiles_of(mask, w, h):
    """the tiles of a (bins_y, bins_x) mask, row-major, clipped to the frame"""
    return np.array([(64 * bx, 64 * by, min(64, w - 64 * bx), min(64, h - 64 * by)) for by, bx in zip(*np.nonzero(mask))], np.int32).reshape(-1, 4)


def _exact(ctx, mirror, what):
    want = ctx.read_pixels()
    assert mirror.shape == want.shape, what
    if not np.array_equal(mirror, want):
        ys, xs = np.nonzero((mirror != want).any(axis=2))
        pytest.fail(f"{what}: the mirror differs from fdh_read_pixels in {len(ys)} pixels, first at ({xs[0]}, {ys[0]}); bins "
                    f"{sorted(set(zip((xs // 64).tolist(), (ys // 64).tolist())))[:8]}")


def _read_checked(ctx, mirror, want_mask, what):
    """fdh_read_damage + fdh_apply_damage; the tiles must be want_mask's bins.  Returns the number of tiles."""
    h, w = mirror.shape[:2]
    tiles, pixels, full = ctx.read_damage()
    assert np.array_equal(tiles, _tiles_of(want_mask, w, h)), f"{what}: the tiles are not the pending bins in row-major order"
    assert full == bool(want_mask.all()), what
    assert pixels.shape == (len(tiles), TILE, TILE, 4)
    for (x, y, tw, th), px in zip(tiles, pixels):
        assert not px[th:].any() and not px[:, tw:].any(), f"{what}: slot bytes past the tile's edge are not zero (tile at {x}, {y})"
    before = mirror.copy() if len(tiles) == 0 else None
    HipContext.apply_damage(mirror, tiles, pixels)
    if before is not None:
        assert np.array_equal(mirror, before)
    _exact(ctx, mirror, what)
    return len(tiles)


def _run_every_frame(frames, w, h, route=None):
    """a read after every frame: the tiles are that frame's fdh_damage_bins"""
    ctx = _ctx(route)
    mirror = _mirror(w, h)
    counts = []
    try:
        for i, fr in enumerate(frames):
            fr(ctx)
            mask = ctx.damage_bins()
            if i == 0:
                assert mask.all()
            counts.append(_read_checked(ctx, mirror, mask, f"frame {i}"))
            if not mask.any():
                assert counts[-1] == 0
    finally:
        ctx.close()
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1])
def test_reference_scenes_each_twice(route):
    w, h = 640, 480
    frames = []
    for name in REF:
        fn = getattr(RS, name)
        frames += [_scene(fn, w, h), _scene(fn, w, h)]
    counts = _run_every_frame(frames, w, h, route)
    assert counts[0] == 10 * 8
    assert 0 in counts, "no unchanged frame gave an empty read"


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1])
def test_random_scenes_clipped_last_column_and_row(route):
    w, h = 513, 389
    frames = [(lambda s: (lambda ctx: ctx.render_frame(RS.random_scene(s, float(w), float(h), n=40), w, h)))(s) for s in (3, 3, 4, 5, 5, 6)]
    counts = _run_every_frame(frames, w, h, route)
    assert counts[0] == 9 * 7 and counts[1] == 0
    # the clipped tiles themselves, from a context of its own
    ctx = _ctx(route)
    try:
        frames[0](ctx)
        tiles, pixels, full = ctx.read_damage()
        assert full and len(tiles) == 63
        assert tiles[8].tolist() == [512, 0, 1, 64] and tiles[6 * 9].tolist() == [0, 384, 64, 5] and tiles[62].tolist() == [512, 384, 1, 5]
        assert not pixels[8][:, 1:].any() and not pixels[54][5:].any() and not pixels[62][5:].any() and not pixels[62][:, 1:].any()
        assert np.array_equal(pixels[62][:5, :1], ctx.read_pixels()[384:, 512:])
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("ffb", [False, True])
def test_bench_tree_frames_read_every_frame(route, ffb):
    w, h = 1920, 1080
    frames = [(lambda k: (lambda ctx: ctx.render_frame(make_render_tree_100(float(w), float(h), frame=k, full_frame_blur=ffb), w, h)))(k)
              for k in (0, 1, 2, 2, 3)]
    counts = _run_every_frame(frames, w, h, route)
    assert counts[0] == 30 * 17
    if not ffb:
        assert counts[3] == 0  # frame 2 again


def _skipped(frames, w, h):
    ctx = _ctx()
    mirror = _mirror(w, h)
    try:
        union = None
        for i, fr in enumerate(frames):
            fr(ctx)
            mask = ctx.damage_bins()
            union = mask if union is None else (union | mask)
            if i % 3 == 2:
                n = _read_checked(ctx, mirror, union, f"read after frame {i}")
                assert n == union.sum()
                if i > 2:
                    assert 0 < n < union.size, "the later reads of this sequence are partial ones"
                union = None
    finally:
        ctx.close()


@pytest.mark.gpu
def test_skipped_reads_bench_tree():
    w, h = 1920, 1080
    sc = make_render_tree_100(float(w), float(h), frame=0)
    lst = next(iter(sc.layers.values()))
    roots = [lst.rootIds[len(lst.rootIds) * k // 4] for k in (1, 2, 3)]

    def frame(i):
        def fr(ctx):
            n = lst.nodes[roots[i % 3]]
            x, y, bw, bh = n.screenBox
            n.screenBox = rect(x + 3.0, y + 2.0, bw, bh)
            ctx.render_frame(sc, w, h)
        return fr
    _skipped([frame(i) for i in range(9)], w, h)


@pytest.mark.gpu
def test_skipped_reads_non_clip_benchmark():
    sc = make_non_clip_benchmark()
    lst = next(iter(sc.layers.values()))

    def frame(i):
        def fr(ctx):
            lst.nodes[5 + 3 * i].fill = fill(rgba(255, 0, 0, 255) if i % 2 else rgba(0, 0, 255, 255))
            ctx.render_frame(sc, 1200, 800)
        return fr
    _skipped([frame(i) for i in range(9)], 1200, 800)


def _box(x, y=40, color=(255, 0, 0, 255)):
    return lambda c: (c.draw_rect((300, 200, 120, 90), (20, 120, 60, 255)), c.draw_rect((x, y, 50, 40), color))


def _into(ctx, mirror, what, want=None):
    n = ctx.read_damage_into(mirror)
    _exact(ctx, mirror, what)
    if want is not None:
        assert n == want, f"{what}: {n} tiles, expected {want}"
    return n


@pytest.mark.gpu
def test_full_after_turning_the_mode_on_and_off_and_on_again():
    w, h, nb = 700, 500, 11 * 8
    ctx = HipContext(device=0)
    ctx.set_damage_tracking(True)
    mirror = _mirror(w, h)
    try:
        with pytest.raises(FigdrawHipError) as e:  # the mode is off
            ctx.read_damage()
        assert e.value.code == INVALID
        ctx.set_damage_readback(True)
        with pytest.raises(FigdrawHipError) as e:  # no frame yet
            ctx.read_damage_into(mirror)
        assert e.value.code == INVALID
        fr = _imm(w, h, _box(40))
        fr(ctx); fr(ctx); fr(ctx)  # the last two composite nothing; the first read still brings every bin
        assert ctx.damage_bins().sum() == 0
        _into(ctx, mirror, "first read", nb)
        fr(ctx)
        _into(ctx, mirror, "unchanged", 0)
        ctx.set_damage_readback(False)
        with pytest.raises(FigdrawHipError) as e:
            ctx.read_damage_into(mirror)
        assert e.value.code == INVALID
        _imm(w, h, _box(200))(ctx)  # a frame the pending set never saw
        ctx.set_damage_readback(True)
        fr2 = _imm(w, h, _box(200))
        fr2(ctx)
        assert ctx.damage_bins().sum() == 0
        mirror[:] = SENTINEL
        _into(ctx, mirror, "on again", nb)
        _imm(w, h, _box(330))(ctx)
        n = _into(ctx, mirror, "partial")
        assert 0 < n < 12 and n == ctx.damage_bins().sum()
        ctx.set_damage_readback(True)  # already on: nothing is reset
        _into(ctx, mirror, "still on", 0)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_full_after_an_untracked_frame_and_after_a_frame_that_does_not_clear():
    w, h, nb = 700, 500, 11 * 8
    ctx = _ctx()
    mirror = _mirror(w, h)
    try:
        _imm(w, h, _box(40))(ctx)
        _into(ctx, mirror, "first", nb)
        _imm(w, h, _box(60))(ctx)
        assert 0 < _into(ctx, mirror, "partial") < 8
        ctx.set_damage_tracking(False)
        _imm(w, h, _box(60))(ctx)
        _into(ctx, mirror, "tracking off", nb)
        ctx.set_damage_tracking(True)
        _imm(w, h, _box(60))(ctx)  # the first tracked frame after it is a full one
        _into(ctx, mirror, "tracking on again", nb)
        _imm(w, h, _box(60))(ctx)
        _into(ctx, mirror, "unchanged", 0)
        # an untracked frame among skipped reads: partial, untracked, partial -> everything
        _imm(w, h, _box(90))(ctx)
        ctx.set_damage_tracking(False)
        _imm(w, h, _box(120))(ctx)
        ctx.set_damage_tracking(True)
        _imm(w, h, _box(150))(ctx)
        _imm(w, h, _box(180))(ctx)
        _into(ctx, mirror, "untracked in between", nb)
        # clear_main = 0
        _imm(w, h, _box(180))(ctx)
        _into(ctx, mirror, "unchanged", 0)
        _imm(w, h, lambda c: c.draw_rect((100, 300, 50, 50), (0, 0, 255, 128)), clear=False)(ctx)
        assert ctx.damage_bins().all()
        _into(ctx, mirror, "no clear", nb)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_frame_size_change():
    ctx = _ctx()
    try:
        w, h = 700, 500
        mirror = _mirror(w, h)
        _imm(w, h, _box(40))(ctx)
        _into(ctx, mirror, "first", 88)
        for w2, h2, nb2 in ((690, 490, 88), (737, 489, 96)):  # the same bin grid, then another one
            _imm(w2, h2, _box(40))(ctx)
            keep = mirror.copy()
            with pytest.raises(FigdrawHipError) as e:
                ctx.read_damage_into(mirror)
            assert e.value.code == INVALID and np.array_equal(mirror, keep)
            _imm(w2, h2, _box(40))(ctx)  # composites nothing: what is pending must still be everything
            assert ctx.damage_bins().sum() == 0
            mirror = _mirror(w2, h2)
            _into(ctx, mirror, f"{w2} x {h2}", nb2)
            _imm(w2, h2, _box(70))(ctx)
            assert 0 < _into(ctx, mirror, "partial at the new size") < 8
    finally:
        ctx.close()


@pytest.mark.gpu
def test_update_image_between_frames():
    w, h = 320, 240
    img_a = np.zeros((32, 32, 4), np.uint8); img_a[..., 0] = 255; img_a[..., 3] = 255
    img_b = img_a.copy(); img_b[8:24, 8:24, 1] = 255
    ctx = _ctx()
    mirror = _mirror(w, h)
    try:
        ctx.put_image(7, img_a)
        draw = _imm(w, h, lambda c: (c.draw_rect((0, 0, 40, 40), (0, 0, 0, 255)), c.draw_image(7, (100.0, 80.0), [(255, 255, 255, 255)] * 4, (32.0, 32.0))))
        draw(ctx)
        _into(ctx, mirror, "first", 20)
        draw(ctx)
        _into(ctx, mirror, "unchanged", 0)
        ctx.update_image(7, img_b)
        draw(ctx)
        _into(ctx, mirror, "after fdh_update_image", 20)
        assert (mirror[88:104, 108:124, 1] == 255).all()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_full_frame_blur_then_partial_frames():
    w, h = 1280, 720
    ctx = _ctx(route=1)
    mirror = _mirror(w, h)
    try:
        frames = [_scene(lambda ww, hh: make_render_tree_100(ww, hh, frame=0, full_frame_blur=True), w, h),
                  _scene(lambda ww, hh: make_render_tree_100(ww, hh, frame=0, full_frame_blur=True), w, h),
                  _imm(w, h, lambda c: c.draw_rect((10, 10, 80, 80), (255, 0, 0, 255))),
                  _imm(w, h, lambda c: c.draw_rect((10, 10, 80, 80), (255, 0, 0, 255))),
                  _imm(w, h, lambda c: c.draw_rect((30, 10, 80, 80), (255, 0, 0, 255)))]
        want = [240, 240, None, 0, None]  # (k_blur_fx flips the surfaces: a full frame even when nothing changed)
        for i, fr in enumerate(frames):
            fr(ctx)
            n = _into(ctx, mirror, f"frame {i}", want[i])
            assert n == ctx.damage_bins().sum()
        assert 0 < n < 8
    finally:
        ctx.close()


@pytest.mark.gpu
def test_every_way_to_submit():
    w, h = 640, 480
    rnd = random.Random(9)
    sc = RS.random_scene(9, float(w), float(h), n=60, clips=True, blur=True)
    lst = next(iter(sc.layers.values()))
    ctx = _ctx()
    mirror = _mirror(w, h)
    try:
        # immediate mode
        _imm(w, h, _box(40))(ctx)
        _into(ctx, mirror, "immediate 0", 80)
        _imm(w, h, _box(90))(ctx)
        assert 0 < _into(ctx, mirror, "immediate 1") < 8
        # fdh_replay of that frame: nothing changes, nothing is pending -- also when no read came in between
        ctx.replay(2)
        _into(ctx, mirror, "replay", 0)
        ctx.replay_async(1)
        _into(ctx, mirror, "replay_async", 0)
        _imm(w, h, _box(140))(ctx)
        mask = ctx.damage_bins()
        ctx.replay(1)
        assert ctx.damage_bins().sum() == 0
        assert _read_checked(ctx, mirror, mask, "a frame, then its replay") > 0
        # an untracked replay composites every bin
        ctx.set_damage_tracking(False)
        _imm(w, h, _box(140))(ctx)
        _into(ctx, mirror, "untracked", 80)
        ctx.replay(1)
        _into(ctx, mirror, "untracked replay", 80)
        ctx.set_damage_tracking(True)
        # a retained scene edited node by node
        ctx.scene_retain(sc, w, h)
        ctx.scene_render()
        _into(ctx, mirror, "retained 0", 80)
        for step in range(6):
            i = rnd.randrange(len(lst.nodes))
            n = lst.nodes[i]
            x, y, bw, bh = n.screenBox
            n.screenBox = rect(x + rnd.uniform(-9, 9), y + rnd.uniform(-9, 9), bw, bh)
            ctx.scene_update_nodes(0, i, [n])
            ctx.scene_render()
            assert _read_checked(ctx, mirror, ctx.damage_bins(), f"retained step {step}") == ctx.damage_bins().sum()
        ctx.scene_render()
        mask = ctx.damage_bins()
        ctx.replay(2)
        _read_checked(ctx, mirror, mask | ctx.damage_bins(), "retained, unchanged, and replayed")
        # fdh_render_frame
        ctx.render_frame(sc, w, h)
        _into(ctx, mirror, "render_frame", int(ctx.damage_bins().sum()))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_readback_with_tracking_off():
    w, h = 513, 389
    ctx = _ctx(tracking=False)
    mirror = _mirror(w, h)
    try:
        for i, s in enumerate((3, 3, 4)):
            ctx.render_frame(RS.random_scene(s, float(w), float(h), n=40), w, h)
            tiles, pixels, full = ctx.read_damage()
            assert full and len(tiles) == 63
            HipContext.apply_damage(mirror, tiles, pixels)
            _exact(ctx, mirror, f"frame {i}")
            mirror[:] = SENTINEL
            ctx.render_frame(RS.random_scene(s, float(w), float(h), n=40), w, h)
            _into(ctx, mirror, f"frame {i} again", 63)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_the_mode_does_not_disturb_rendering():
    w, h = 1920, 1080
    a, b = _ctx(), _ctx(readback=False)
    mirror = _mirror(w, h)
    try:
        for i, k in enumerate((0, 1, 2, 2, 3)):
            sc = make_render_tree_100(float(w), float(h), frame=k)
            a.render_frame(sc, w, h)
            b.render_frame(sc, w, h)
            assert np.array_equal(a.damage_bins(), b.damage_bins()), f"frame {i}"
            a.read_damage_into(mirror)
            assert np.array_equal(a.read_pixels(), b.read_pixels()), f"frame {i}"
            assert np.array_equal(a.damage_bins(), b.damage_bins()), f"frame {i}, after the read"
            _exact(b, mirror, f"frame {i}")
    finally:
        a.close(); b.close()


@pytest.mark.gpu
def test_pointers_survive_further_frames_and_null_out_pointers():
    w, h = 700, 500
    ctx = _ctx()
    L = ctx.L
    try:
        _imm(w, h, _box(40))(ctx)
        assert L.fdh_read_damage(ctx.h, None, None, None, None, None, None) == 0  # consumes the set all the same
        _imm(w, h, _box(200))(ctx)
        t, p = C.c_void_p(), C.c_void_p()
        n, fw, fh, full = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        assert L.fdh_read_damage(ctx.h, C.byref(t), C.byref(p), C.byref(n), C.byref(fw), C.byref(fh), C.byref(full)) == 0
        assert (fw.value, fh.value, full.value) == (w, h, 0) and 0 < n.value < 12
        held = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value, TILE, TILE, 4))
        tiles = np.ctypeslib.as_array(C.cast(t, C.POINTER(C.c_int32)), shape=(n.value, 4))
        snap, tsnap = held.copy(), tiles.copy()
        frame = ctx.read_pixels()
        for (x, y, tw, th), px in zip(tsnap, snap):
            assert np.array_equal(px[:th, :tw], frame[y:y + th, x:x + tw])
        for x in (260, 320, 380):
            _imm(w, h, _box(x))(ctx)
        ctx.sync()
        assert np.array_equal(held, snap) and np.array_equal(tiles, tsnap), "submitting frames changed what the last read returned"
    finally:
        ctx.close()


@pytest.mark.gpu
def test_read_into_a_mirror_with_a_row_pitch():
    """both ways fdh_read_damage_into fills the mirror -- the whole frame in one copy when most of the grid is pending, tile by tile
    otherwise -- respect the pitch and leave its padding alone"""
    w, h = 700, 500
    ctx = _ctx()
    store = np.full((h, w + 13, 4), SENTINEL, np.uint8)
    mirror = store[:, :w]
    try:
        _imm(w, h, _box(40))(ctx)
        _into(ctx, mirror, "every bin pending", 88)
        _imm(w, h, _box(200))(ctx)
        assert 0 < _into(ctx, mirror, "a few bins pending") < 12
        for k, x in enumerate((20, 150, 280, 410, 540)):  # 30 bins and more of 88 over a skipped stretch
            _imm(w, h, lambda c, x=x: c.draw_rect((x, 10 + 90 * k, 150, 100), (0, 0, 200, 255)))(ctx)
        n = _into(ctx, mirror, "a third of the grid pending")
        assert 0 < n < 88
        assert (store[:, w:] == SENTINEL).all(), "the pitch padding was written"
    finally:
        ctx.close()


@pytest.mark.gpu
def test_four_contexts_on_four_threads():
    w, h = 800, 600
    errors = []

    def work(j):
        try:
            ctx = _ctx()
            mirror = _mirror(w, h)
            try:
                for k in range(20):
                    ctx.render_frame(make_render_tree_100(float(w), float(h), frame=(k // 2) + j, copies=20), w, h)
                    if k % 5 != 4:  # a skipped read now and then
                        ctx.read_damage_into(mirror)
                        if not np.array_equal(mirror, ctx.read_pixels()):
                            errors.append(f"context {j}, frame {k}: the mirror differs")
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


@pytest.mark.gpu
def test_at_size_glyph_rows_4k():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import damage_bench

    w, h, setup, frame = damage_bench.frames_for("a", 10)
    assert (w, h) == (3840, 2160)
    ctx = _ctx()
    mirror = _mirror(w, h)
    try:
        setup(ctx)
        for i in range(10):
            frame(ctx, i)
            n = ctx.read_damage_into(mirror)
            assert n == ctx.damage_bins().sum(), f"frame {i}"
            assert n == 60 * 34 if i == 0 else 0 < n < 200, f"frame {i}: {n} tiles"
            _exact(ctx, mirror, f"frame {i}")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_stripes_refuse_readback():
    ctx = HipContext(device=0)
    try:
        ctx.set_stripe(0, 64)
        with pytest.raises(FigdrawHipError) as e:
            ctx.set_damage_readback(True)
        assert e.value.code == INVALID
        ctx.set_stripe(0, 0)
        ctx.set_damage_readback(True)
        with pytest.raises(FigdrawHipError) as e:
            ctx.set_stripe(0, 64)
        assert e.value.code == INVALID
        ctx.set_damage_readback(False)
        ctx.set_stripe(0, 64)
    finally:
        ctx.close()
