"""Coded damage readback on the GPU (include/figdraw_hip_stream.h, k_damage_encode): what fdh_read_damage_coded returns is, byte for
byte, what tests/tilecode_ref.py -- a numpy encoder written from the header's text -- makes of the same pixels; and a mirror that receives
every coded read through fdh_decode_damage is fdh_read_pixels of the whole frame.  Everything here is equality of bytes."""
import os
import random

import numpy as np
import pytest

import ref_scenes as RS
import tilecode_ref as T
from figdraw_amd.context import FigdrawHipError, HipContext
from figdraw_amd.scene import rect
from figdraw_amd.scenes import load_glyph_fixture, make_render_tree_100
from test_damage import _imm, _scene
from test_damage_readback import SENTINEL, _box, _ctx, _exact, _mirror, _tiles_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_DEVICE = -1, -2


def _checked_read(ctx, want_rects, what):
    """fdh_read_damage_coded -> (tiles, payload, full), with everything the header promises of a stream checked: the tiles are
    want_rects in order, payloads aligned, disjoint and inside the blob, the blob within the bound and without a byte that was not written"""
    h, w = ctx.read_pixels().shape[:2]
    tiles, payload, full = ctx.read_damage_coded()
    got = np.stack([tiles[f].astype(np.int32) for f in "xywh"], axis=1).reshape(-1, 4)
    assert np.array_equal(got, np.asarray(want_rects, np.int32).reshape(-1, 4)), f"{what}: the tiles are not the pending bins in row-major order"
    assert full == (len(tiles) == ((w + 63) // 64) * ((h + 63) // 64)), what
    assert len(payload) <= HipContext.coded_damage_bound(w, h), what
    assert len(payload) == sum(T.ceil16(s) for s in tiles["size"].tolist()), f"{what}: payload_bytes is not the end of the last space claimed"
    blob = np.frombuffer(payload, np.uint8)
    used = np.zeros(len(payload), bool)
    for t in tiles:
        off, size = int(t["offset"]), int(t["size"])
        if t["mode"] == T.SOLID:
            assert (off, size) == (0, 0), what
            continue
        assert off % 16 == 0 and off + T.ceil16(size) <= len(payload), f"{what}: tile at ({t['x']}, {t['y']}) has offset {off}, size {size}"
        assert not used[off:off + T.ceil16(size)].any(), f"{what}: payloads overlap at {off}"
        used[off:off + T.ceil16(size)] = True
        assert not blob[off + size:off + T.ceil16(size)].any(), f"{what}: the round-up to 16 bytes is not zeros"
    assert used.all(), f"{what}: the blob has bytes that belong to no tile"
    return tiles, payload, full


def _same_as_reference(tiles, payload, frame, what):
    """every tile against tilecode_ref.encode of the same pixels: the entry's fields and the payload's bytes.  -> the tiles per mode"""
    px = T.as_u32(frame)
    for t in tiles:
        x, y, w, h = (int(t[f]) for f in "xywh")
        mode, n, solid, data = T.encode(px[y:y + h, x:x + w])
        got = (int(t["mode"]), int(t["n"]), int(t["solid"]), int(t["size"]), int(t["bits"]))
        assert got == (mode, n, solid, len(data), T.pal_bits(n) if mode == T.PAL else 0), f"{what}: tile at ({x}, {y}) {w} x {h}: (mode, n, solid, size, bits) = {got}"
        off = int(t["offset"])
        if payload[off:off + len(data)] != data:
            a, b = np.frombuffer(payload[off:off + len(data)], np.uint8), np.frombuffer(data, np.uint8)
            at = int(np.flatnonzero(a != b)[0])
            pytest.fail(f"{what}: tile at ({x}, {y}) {w} x {h}, mode {mode}, n {n}: payload byte {at} of {len(data)} is {a[at]:#x}, the reference has {b[at]:#x}")
    return np.bincount(tiles["mode"], minlength=4)


# ------------------------------------------------------------------------------------------------------------------ byte-exact
def _noise_image():
    img = np.random.RandomState(11).randint(0, 256, (128, 128, 4)).astype(np.uint8)
    img[..., 3] = 255
    return img


def _glyph_images():
    return load_glyph_fixture(os.path.join(ROOT, "tests", "golden", "glyphs_ubuntu20.npz"))


def _frames():
    """name -> (w, h, setup(ctx), frame(ctx))"""
    none = lambda ctx: None  # noqa: E731
    glyphs = _glyph_images()
    gl = RS.glyphs_small(330.0, 90.0, glyphs)
    used = RS.used_images(gl, glyphs)
    white = [(255, 255, 255, 255)] * 4
    return {
        "flat clear": (700, 500, none, _imm(700, 500, lambda c: None, color=(0.2, 0.4, 0.6, 1.0))),
        "rgb boxes": (800, 600, none, _scene(RS.rgb_boxes, 800, 600)),
        "rgb boxes with shadows": (800, 600, none, _scene(RS.rgb_boxes_sdf, 800, 600)),
        "linear gradient": (800, 600, none, _scene(RS.linear_gradient, 800, 600)),
        "glyphs": (330, 90, lambda ctx: [ctx.put_image(k, v) for k, v in used.items()], lambda ctx: ctx.render_frame(gl, 330, 90)),
        "backdrop blur": (320, 240, none, _scene(RS.backdrop_blur, 320, 240)),
        "bench tree with a full-frame blur": (1280, 720, none, lambda ctx: ctx.render_frame(make_render_tree_100(1280.0, 720.0, frame=0, full_frame_blur=True), 1280, 720)),
        "noise image 1:1": (320, 240, lambda ctx: ctx.put_image(7, _noise_image()),
                            _imm(320, 240, lambda c: (c.draw_rect((10, 10, 30, 200), (200, 0, 0, 255)), c.draw_image(7, (64.0, 64.0), white, (128.0, 128.0))))),
        "130 x 70": (130, 70, none, lambda ctx: ctx.render_frame(RS.random_scene(3, 130.0, 70.0, n=25, clips=False, blur=False), 130, 70)),
        "130 x 70 flat": (130, 70, none, _imm(130, 70, lambda c: c.draw_rect((100, 30, 29, 37), (0, 90, 200, 255)))),
        "513 x 389": (513, 389, none, lambda ctx: ctx.render_frame(RS.random_scene(4, 513.0, 389.0, n=40), 513, 389)),
    }


@pytest.mark.gpu
def test_coded_reads_are_byte_exact_against_the_reference_encoder():
    seen = np.zeros(4, np.int64)
    for name, (w, h, setup, frame) in _frames().items():
        fresh = HipContext(device=0)
        ctx = _ctx()
        try:
            setup(fresh); frame(fresh)
            want = fresh.read_pixels()
            setup(ctx); frame(ctx)
            tiles, payload, full = _checked_read(ctx, T.tiles_of(w, h), name)
            assert full, name
            modes = _same_as_reference(tiles, payload, want, name)
            print(f"{name}: {w} x {h}, {len(tiles)} tiles, SOLID / PAL / RUNS / RAW {modes.tolist()}, {24 * len(tiles) + len(payload)} of {4 * w * h} bytes")
            if name == "noise image 1:1":
                assert modes[T.RAW] >= 4, "the bins the noise covers are RAW"
            if name.startswith("130 x 70"):
                assert [int(tiles[k][f]) for k in (2, 5) for f in "xywh"] == [128, 0, 2, 64, 128, 64, 2, 6]
            seen += modes
            # the stream decodes to the frame, and the set is empty now
            mirror = _mirror(w, h)
            HipContext.decode_damage(mirror, tiles, payload)
            assert np.array_equal(mirror, want), name
            tiles, payload, full = ctx.read_damage_coded()
            assert len(tiles) == 0 and payload == b"" and not full, f"{name}: a second read"
        finally:
            ctx.close(); fresh.close()
    assert (seen > 0).all(), f"a mode never occurred: {seen.tolist()}"


@pytest.mark.gpu
def test_coded_partial_reads_are_byte_exact_4k_glyph_rows():
    """the pending bins of a partial read (stamps, ranks among the pending bins) at the size the feature is for"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import damage_bench

    w, h, setup, frame = damage_bench.frames_for("a", 4)
    ctx = _ctx()
    try:
        setup(ctx)
        for i in range(4):
            frame(ctx, i)
            mask = ctx.damage_bins()
            tiles, payload, full = _checked_read(ctx, _tiles_of(mask, w, h), f"frame {i}")
            assert len(tiles) == (60 * 34 if i == 0 else mask.sum()) and (i == 0 or 0 < len(tiles) < 200)
            modes = _same_as_reference(tiles, payload, ctx.read_pixels(), f"frame {i}")
            print(f"frame {i}: {len(tiles)} tiles, SOLID / PAL / RUNS / RAW {modes.tolist()}, {24 * len(tiles) + len(payload)} of {16384 * len(tiles)} bytes")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the mirror invariant
def _coded_into(ctx, mirror, what, want=None, mask=None):
    """a coded read decoded into the mirror, which must then be the frame.  want: the number of tiles; mask: the bins they must be"""
    h, w = mirror.shape[:2]
    tiles, payload, full = ctx.read_damage_coded()
    if mask is not None:
        got = np.stack([tiles[f].astype(np.int32) for f in "xywh"], axis=1).reshape(-1, 4)
        assert np.array_equal(got, _tiles_of(mask, w, h)), f"{what}: the tiles are not the pending bins"
    before = mirror.copy() if len(tiles) == 0 else None
    HipContext.decode_damage(mirror, tiles, payload)
    if before is not None:
        assert np.array_equal(mirror, before) and payload == b""
    _exact(ctx, mirror, what)
    if want is not None:
        assert len(tiles) == want, f"{what}: {len(tiles)} tiles, expected {want}"
    assert full == (len(tiles) == ((w + 63) // 64) * ((h + 63) // 64))
    return len(tiles)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1])
def test_mirror_reference_scenes_each_twice(route):
    from test_damage import REF
    w, h = 640, 480
    ctx = _ctx(route)
    mirror = _mirror(w, h)
    counts = []
    try:
        for name in REF:
            for k in (0, 1):
                _scene(getattr(RS, name), w, h)(ctx)
                mask = ctx.damage_bins()
                counts.append(_coded_into(ctx, mirror, f"{name} #{k}", int(mask.sum()), mask))
    finally:
        ctx.close()
    assert counts[0] == 80 and 0 in counts, "no unchanged frame gave an empty read"


@pytest.mark.gpu
def test_mirror_mode_on_off_on_and_tracking_on_off():
    w, h, nb = 700, 500, 11 * 8
    ctx = HipContext(device=0)
    ctx.set_damage_tracking(True)
    mirror = _mirror(w, h)
    try:
        with pytest.raises(FigdrawHipError) as e:  # the mode is off
            ctx.read_damage_coded()
        assert e.value.code == INVALID
        ctx.set_damage_readback(True)
        with pytest.raises(FigdrawHipError) as e:  # no frame yet
            ctx.read_damage_coded()
        assert e.value.code == INVALID
        fr = _imm(w, h, _box(40))
        fr(ctx); fr(ctx); fr(ctx)
        _coded_into(ctx, mirror, "first read", nb)
        fr(ctx)
        _coded_into(ctx, mirror, "unchanged", 0)
        ctx.set_damage_readback(False)
        with pytest.raises(FigdrawHipError) as e:
            ctx.read_damage_coded()
        assert e.value.code == INVALID
        _imm(w, h, _box(200))(ctx)  # a frame the pending set never saw
        ctx.set_damage_readback(True)
        _imm(w, h, _box(200))(ctx)
        assert ctx.damage_bins().sum() == 0
        mirror[:] = SENTINEL
        _coded_into(ctx, mirror, "on again", nb)
        _imm(w, h, _box(330))(ctx)
        n = _coded_into(ctx, mirror, "partial", mask=ctx.damage_bins())
        assert 0 < n < 12
        # tracking off: every frame is a full one
        ctx.set_damage_tracking(False)
        _imm(w, h, _box(60))(ctx)
        _coded_into(ctx, mirror, "tracking off", nb)
        ctx.set_damage_tracking(True)
        _imm(w, h, _box(60))(ctx)
        _coded_into(ctx, mirror, "tracking on again", nb)
        _imm(w, h, _box(60))(ctx)
        _coded_into(ctx, mirror, "unchanged", 0)
        # an untracked frame among skipped reads: partial, untracked, partial -> everything
        _imm(w, h, _box(90))(ctx)
        ctx.set_damage_tracking(False)
        _imm(w, h, _box(120))(ctx)
        ctx.set_damage_tracking(True)
        _imm(w, h, _box(150))(ctx)
        _imm(w, h, _box(180))(ctx)
        _coded_into(ctx, mirror, "untracked in between", nb)
        _imm(w, h, _box(180))(ctx)
        _coded_into(ctx, mirror, "unchanged", 0)
        _imm(w, h, lambda c: c.draw_rect((100, 300, 50, 50), (0, 0, 255, 128)), clear=False)(ctx)
        _coded_into(ctx, mirror, "no clear", nb)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_mirror_skipped_reads_bench_tree():
    w, h = 1920, 1080
    sc = make_render_tree_100(float(w), float(h), frame=0)
    lst = next(iter(sc.layers.values()))
    roots = [lst.rootIds[len(lst.rootIds) * k // 4] for k in (1, 2, 3)]
    ctx = _ctx()
    mirror = _mirror(w, h)
    try:
        union = None
        for i in range(9):
            n = lst.nodes[roots[i % 3]]
            x, y, bw, bh = n.screenBox
            n.screenBox = rect(x + 3.0, y + 2.0, bw, bh)
            ctx.render_frame(sc, w, h)
            mask = ctx.damage_bins()
            union = mask if union is None else (union | mask)
            if i % 3 == 2:
                got = _coded_into(ctx, mirror, f"read after frame {i}", int(union.sum()), union)
                if i > 2:
                    assert 0 < got < union.size, "the later reads of this sequence are partial ones"
                union = None
    finally:
        ctx.close()


@pytest.mark.gpu
def test_mirror_frame_size_change():
    ctx = _ctx()
    try:
        w, h = 700, 500
        mirror = _mirror(w, h)
        _imm(w, h, _box(40))(ctx)
        _coded_into(ctx, mirror, "first", 88)
        for w2, h2, nb2 in ((690, 490, 88), (737, 489, 96), (130, 70, 6)):  # the same bin grid, another one, a small one
            _imm(w2, h2, _box(40))(ctx)
            _imm(w2, h2, _box(40))(ctx)  # composites nothing: what is pending must still be everything
            assert ctx.damage_bins().sum() == 0
            mirror = _mirror(w2, h2)
            _coded_into(ctx, mirror, f"{w2} x {h2}", nb2)
            _imm(w2, h2, _box(70))(ctx)
            assert 0 < _coded_into(ctx, mirror, "partial at the new size", mask=ctx.damage_bins()) < 8
    finally:
        ctx.close()


@pytest.mark.gpu
def test_mirror_every_way_to_submit():
    w, h = 640, 480
    rnd = random.Random(9)
    sc = RS.random_scene(9, float(w), float(h), n=60, clips=True, blur=True)
    lst = next(iter(sc.layers.values()))
    ctx = _ctx()
    mirror = _mirror(w, h)
    try:
        _imm(w, h, _box(40))(ctx)
        _coded_into(ctx, mirror, "immediate 0", 80)
        _imm(w, h, _box(90))(ctx)
        assert 0 < _coded_into(ctx, mirror, "immediate 1") < 8
        ctx.replay(2)
        _coded_into(ctx, mirror, "replay", 0)
        ctx.replay_async(1)
        _coded_into(ctx, mirror, "replay_async", 0)
        _imm(w, h, _box(140))(ctx)
        mask = ctx.damage_bins()
        ctx.replay(1)
        assert ctx.damage_bins().sum() == 0
        assert _coded_into(ctx, mirror, "a frame, then its replay", mask=mask) > 0
        ctx.set_damage_tracking(False)
        _imm(w, h, _box(140))(ctx)
        _coded_into(ctx, mirror, "untracked", 80)
        ctx.replay(1)
        _coded_into(ctx, mirror, "untracked replay", 80)
        ctx.set_damage_tracking(True)
        ctx.scene_retain(sc, w, h)
        ctx.scene_render()
        _coded_into(ctx, mirror, "retained 0", 80)
        for step in range(6):
            i = rnd.randrange(len(lst.nodes))
            n = lst.nodes[i]
            x, y, bw, bh = n.screenBox
            n.screenBox = rect(x + rnd.uniform(-9, 9), y + rnd.uniform(-9, 9), bw, bh)
            ctx.scene_update_nodes(0, i, [n])
            ctx.scene_render()
            _coded_into(ctx, mirror, f"retained step {step}", int(ctx.damage_bins().sum()), ctx.damage_bins())
        ctx.scene_render()
        mask = ctx.damage_bins()
        ctx.replay(2)
        _coded_into(ctx, mirror, "retained, unchanged, and replayed", mask=mask | ctx.damage_bins())
        ctx.render_frame(sc, w, h)
        _coded_into(ctx, mirror, "render_frame", int(ctx.damage_bins().sum()))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ interleaving
@pytest.mark.gpu
def test_raw_and_coded_reads_interleaved():
    """each read, of whichever kind, returns exactly the bins pending since the previous read of any kind"""
    w, h = 700, 500
    ctx = _ctx()
    mirror = _mirror(w, h)
    try:
        kinds = ["coded", "raw", "coded", "coded", "into", "coded", "raw", "raw", "coded", "into", "coded"]
        for i, kind in enumerate(kinds):
            union = np.zeros((8, 11), bool)
            for k in range(1 + i % 3):  # one to three frames between reads
                _imm(w, h, _box(30 + 47 * ((3 * i + k) % 13), 40 + 31 * (i % 9)))(ctx)
                union |= ctx.damage_bins().astype(bool)
            if i == 0:
                union[:] = True  # the mode was just turned on
            assert i == 0 or 0 < union.sum() < 40
            want = _tiles_of(union, w, h)
            if kind == "coded":
                _coded_into(ctx, mirror, f"read {i} (coded)", len(want), union)
            elif kind == "raw":
                tiles, pixels, _ = ctx.read_damage()
                assert np.array_equal(tiles, want), f"read {i} (raw)"
                HipContext.apply_damage(mirror, tiles, pixels)
                _exact(ctx, mirror, f"read {i} (raw)")
            else:
                assert ctx.read_damage_into(mirror) == len(want), f"read {i} (into)"
                _exact(ctx, mirror, f"read {i} (into)")
        # a raw read's pointers' worth of data is not what a coded read returns: both are copies here; nothing is pending after either
        assert len(ctx.read_damage_coded()[0]) == 0 and len(ctx.read_damage()[0]) == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ errors, null out-pointers
@pytest.mark.gpu
def test_coded_read_errors_and_null_out_pointers():
    import ctypes as C
    w, h = 700, 500
    ctx = HipContext(device=0)
    L = ctx.L
    try:
        _imm(w, h, _box(40))(ctx)
        with pytest.raises(FigdrawHipError) as e:  # a frame, but the mode is off
            ctx.read_damage_coded()
        assert e.value.code == INVALID and b"fdh_read_damage_coded" in L.fdh_last_error()
        ctx.set_damage_tracking(True)
        ctx.set_damage_readback(True)
        _imm(w, h, _box(40))(ctx)
        assert L.fdh_read_damage_coded(ctx.h, None, None, None, None, None, None, None) == 0  # consumes the set all the same
        _imm(w, h, _box(200))(ctx)
        t, p = C.c_void_p(), C.c_void_p()
        n, fw, fh, full, nbytes = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        assert L.fdh_read_damage_coded(ctx.h, C.byref(t), C.byref(p), C.byref(n), C.byref(nbytes), C.byref(fw), C.byref(fh), C.byref(full)) == 0
        assert (fw.value, fh.value, full.value) == (w, h, 0) and 0 < n.value < 12 and nbytes.value % 16 == 0
        held = np.frombuffer(C.string_at(t.value, 24 * n.value), T.ENTRY)
        for x in (260, 320, 380):  # submitting frames does not change what the last read returned
            _imm(w, h, _box(x))(ctx)
        ctx.sync()
        assert np.array_equal(np.frombuffer(C.string_at(t.value, 24 * n.value), T.ENTRY), held)
    finally:
        ctx.close()
    rec = HipContext(record_only=True)
    with pytest.raises(FigdrawHipError) as e:
        rec.read_damage_coded()
    assert e.value.code == NO_DEVICE
    rec.close()


# ------------------------------------------------------------------------------------------------------------------ nothing else moved
@pytest.mark.gpu
def test_coded_reads_do_not_disturb_rendering():
    """a context that takes a coded read after every frame renders what one that never calls it renders: pixels, damage, bin digest"""
    w, h = 1920, 1080
    a, b = _ctx(), _ctx(readback=False)
    mirror = _mirror(w, h)
    try:
        for i, k in enumerate((0, 1, 2, 2, 3)):
            sc = make_render_tree_100(float(w), float(h), frame=k)
            a.render_frame(sc, w, h)
            b.render_frame(sc, w, h)
            assert a.bin_digest() == b.bin_digest(), f"frame {i}"
            assert np.array_equal(a.damage_bins(), b.damage_bins()), f"frame {i}"
            tiles, payload, _ = a.read_damage_coded()
            HipContext.decode_damage(mirror, tiles, payload)
            assert np.array_equal(a.read_pixels(), b.read_pixels()), f"frame {i}"
            assert np.array_equal(a.damage_bins(), b.damage_bins()) and a.bin_digest() == b.bin_digest(), f"frame {i}, after the read"
            _exact(b, mirror, f"frame {i}")
    finally:
        a.close(); b.close()
