"""Moved damage readback, the host side (include_readback/figdraw_hip_moves.h): the header and the C ABI, the host-only decoder
fdh_decode_damage_moved against tests/tilemove_ref.py -- stream version 2 and the mover in numpy, written from the header's text -- and the
source of the three kernels of k_damage_move.hip under the threaded host shim of tests/emu (tests/move_emu).  Everything here is equality of
bytes and of counts."""
import os
import re
import subprocess

import numpy as np
import pytest

import emu_build
import tilecode_ref as T
import tilemove_ref as M
from conftest import load_png
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_readback", "figdraw_hip_moves.h")
CSRC = os.path.join(ROOT, "figdraw_amd", "csrc")
NEW_API = ("fdh_read_damage_moved", "fdh_decode_damage_moved", "fdh_find_damage_moves")
INVALID, NO_DEVICE = -1, -2
SENTINEL = 0xA5
EPOCH = 7  # what tests/move_emu/emu.cpp passes as the epoch
GROUND = 0xFFF0E8E0


# ------------------------------------------------------------------------------------------------------------------ header and ABI
def test_header_declares_and_library_exports_the_moves_api():
    src = open(HEADER).read()
    assert '#include "../include/figdraw_hip_stream.h"' in src
    declared = re.findall(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(", src)
    assert sorted(declared) == sorted(NEW_API)
    assert re.search(r"FDH_TILE_COPY\s*=\s*4\b", src) and re.search(r"FDH_DAMAGE_MOVES_MAX\s+8\b", src) and re.search(r"FDH_DAMAGE_SHIFT_MAX\s+256\b", src)
    assert "VERSION 2" in src, "the header says that a receiver must know the stream's version"
    L = context.load()
    for name in NEW_API:
        assert hasattr(L, name), name
    six = ("figdraw_hip.h", "figdraw_hip_damage.h", "figdraw_hip_pick.h", "figdraw_hip_readback.h", "figdraw_hip_stream.h", "figdraw_hip_exact.h")
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(six)
    for other in six:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(r"\b%s\b" % n, text) for n in NEW_API + ("FDH_TILE_COPY",)), other
    assert os.listdir(os.path.join(ROOT, "include_readback")) == ["figdraw_hip_moves.h"]
    assert (HipContext.TILE_COPY, HipContext.DAMAGE_MOVES_MAX, HipContext.DAMAGE_SHIFT_MAX) == (M.COPY, M.MOVES_MAX, M.SHIFT_MAX) == (4, 8, 256)
    assert HipContext.DAMAGE_MOVE.itemsize == 4


def test_moves_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "moves_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_readback"),
                           os.path.join(ROOT, "tests", "moves_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "moves_abi_smoke: OK" in r.stdout
    src = open(os.path.join(ROOT, "tests", "moves_abi_smoke.c")).read()
    assert all(re.search(r"\b%s\b" % n, src) for n in NEW_API + ("FDH_TILE_COPY", "FdhDamageMove"))


def test_record_only_context_refuses_the_read_and_the_mover():
    ctx = HipContext(record_only=True)
    for call in (lambda: ctx.read_damage_moved([(0, 17)]), lambda: ctx.read_damage_moved(), lambda: ctx.find_damage_moves(),
                 lambda: ctx.find_damage_moves(0, 3), lambda: ctx.read_damage_moved([(0, 0)])):
        with pytest.raises(FigdrawHipError) as e:
            call()
        assert e.value.code == NO_DEVICE
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ frames
def _content(w, h, seed):
    """uint32 (h, w): a solid ground with solid boxes, two-colour 'text' rows, a gradient card and a noise card on it"""
    rng = np.random.RandomState(seed)
    px = np.full((h, w), GROUND, np.uint32)
    for _ in range(max(3, w * h // 6000)):
        x, y, bw, bh = rng.randint(0, w), rng.randint(0, h), rng.randint(3, 60), rng.randint(3, 40)
        px[y:y + bh, x:x + bw] = 0xFF000000 | rng.randint(0, 1 << 24)
    for y in range(5, h - 8, 23):  # text rows: ink where a random mask says so
        ink = rng.rand(7, w) < 0.35
        px[y:y + 7][ink] = 0xFF202020
    gy, gx = min(h, 50), min(w, 90)
    yy, xx = np.mgrid[0:gy, 0:gx]
    px[h - gy:, :gx] = (0xFF000000 | (xx * 2) | ((yy * 5) << 8) | (((xx + yy) & 255) << 16)).astype(np.uint32)
    ny, nx = min(h, 40), min(w, 70)
    px[:ny, w - nx:] = rng.randint(0, 1 << 32, (ny, nx), dtype=np.uint64).astype(np.uint32)
    return px


def _scrolled(px, dx, dy, seed=99):
    """the frame after its content moved so that pixel (x, y) now shows what (x + dx, y + dy) showed; what scrolls in is new content"""
    h, w = px.shape
    out = _content(w, h, seed)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    out[ys, xs] = px[max(0, dy):max(0, dy) + (ys.stop - ys.start), max(0, dx):max(0, dx) + (xs.stop - xs.start)]
    return out


def _decode_c(old, directory, blob, pitch_pad=5):
    """the stream through fdh_decode_damage_moved into a copy of `old` with a row pitch -> the image"""
    h, w = old.shape[:2]
    store = np.full((h, w + pitch_pad, 4), SENTINEL, np.uint8)
    store[:, :w] = old
    HipContext.decode_damage_moved(store[:, :w], directory, blob)
    assert (store[:, w:] == SENTINEL).all(), "the pitch padding was written"
    return store[:, :w].copy()


def _roundtrip(old_px, new_px, moves, rects=None):
    """reference encoder -> C decoder and reference decoder, both into the old image -> (directory, copies)"""
    old, new = T.as_rgba(old_px), T.as_rgba(new_px)
    h, w = old_px.shape
    rects = T.tiles_of(w, h) if rects is None else rects
    directory, blob, copied = M.encode_frame_moved(old, new, moves, rects)
    assert copied == int((directory["mode"] == M.COPY).sum())
    want = old.copy()
    for x, y, tw, th in rects:
        want[y:y + th, x:x + tw] = new[y:y + th, x:x + tw]
    got = _decode_c(old, directory, blob)
    assert np.array_equal(got, want), "fdh_decode_damage_moved"
    ref = old.copy()
    M.decode_moved(ref, directory, blob)
    assert np.array_equal(ref, want), "tilemove_ref.decode_moved"
    return directory, copied


# ------------------------------------------------------------------------------------------------------------------ known answers
def test_copy_known_answers():
    w, h = 256, 192
    old = _content(w, h, 1)
    old[64:128, 64:128] = 0xFF123456            # a one-colour tile's worth, and more of it 17 rows further down
    old[128:150, 64:128] = 0xFF123456
    new = _scrolled(old, 0, 17)
    directory, copied = _roundtrip(old, new, [(0, 17)])
    by_xy = {(int(e["x"]), int(e["y"])): e for e in directory}
    assert copied > 0
    # a one-colour moved tile is SOLID, never COPY, though it matches the move
    assert (new[64:128, 64:128] == 0xFF123456).all() and M.matching_move(old, new[64:128, 64:128], 64, 64, [(0, 17)]) == 0
    assert by_xy[(64, 64)]["mode"] == T.SOLID and by_xy[(64, 64)]["solid"] == 0xFF123456
    # every tile of the first two bin rows has its source inside the frame; the last bin row's would leave it: skipped, coded from scratch
    for (x, y), e in by_xy.items():
        if y == 128:
            assert e["mode"] != M.COPY
        elif (x, y) != (64, 64):
            assert e["mode"] == M.COPY and M.word_move(e["solid"]) == (0, 17) and (e["bits"], e["n"], e["offset"], e["size"]) == (0, 0, 0, 0)
    assert copied == 7
    # the first matching move wins: a frame that repeats every 8 rows matches (0, 8), (0, 16) and (0, -8) alike
    rep = np.tile(_content(w, 8, 3), (h // 8, 1))
    for moves, first in (([(0, 16), (0, 8)], (0, 16)), ([(0, 8), (0, 16)], (0, 8)), ([(0, -8), (0, 8)], (0, 8)), ([(5, 0), (0, -8), (0, 8)], (0, 8))):
        d, _ = _roundtrip(rep, rep, moves)
        e = {(int(t["x"]), int(t["y"])): t for t in d}[(64, 0)]
        assert e["mode"] == M.COPY and M.word_move(e["solid"]) == first, (moves, M.word_move(e["solid"]))  # ((0, -8) leaves the frame from row 0)
    e = {(int(t["x"]), int(t["y"])): t for t in _roundtrip(rep, rep, [(0, -8), (0, 8)])[0]}[(64, 64)]
    assert M.word_move(e["solid"]) == (0, -8)
    # no moves: version 1, byte for byte
    d2, blob2, c2 = M.encode_frame_moved(T.as_rgba(old), T.as_rgba(new), [], T.tiles_of(w, h))
    d1, blob1 = T.encode_frame(T.as_rgba(new))
    assert c2 == 0 and d2.tobytes() == d1.tobytes() and blob2 == blob1
    # negative components survive the 16-bit packing
    assert M.word_move(M.move_word(-256, 255)) == (-256, 255) and M.move_word(-1, -2) == 0xFFFEFFFF


@pytest.mark.parametrize("move", [(0, 17), (0, -64), (5, 0), (3, -9), (-2, 6)])
def test_clipped_tiles_move(move):
    """131 x 70: a 3 x 2 grid, last column 3 wide, last row 6 high, rows that are not 16-byte aligned"""
    w, h = 131, 70
    old = _content(w, h, 5)
    new = _scrolled(old, *move)
    directory, copied = _roundtrip(old, new, [move])
    want = sum(1 for x, y, tw, th in T.tiles_of(w, h)
               if 0 <= x + move[0] and x + move[0] + tw <= w and 0 <= y + move[1] and y + move[1] + th <= h and len(np.unique(new[y:y + th, x:x + tw])) > 1)
    assert copied == want, (move, copied, want)
    if move in ((5, 0), (-2, 6)):
        assert copied > 0 and any(int(e["w"]) < 64 or int(e["h"]) < 64 for e in directory[directory["mode"] == M.COPY]), "a clipped tile is among the copies"


def test_golden_frames_scrolled_through_the_c_decoder():
    total = 0
    for name in ("ss_glyphs_small.png", "ref_render_rgb_boxes.png", "ref_render_linear_gradient.png", "ss_blur_big_noise_r18.png"):
        old = T.as_u32(load_png(name)).copy()
        h, w = old.shape
        for move in ((0, 17), (-5, 0)):
            new = _scrolled(old, *move)
            directory, copied = _roundtrip(old, new, [move, (0, 120)])
            d1, _ = T.encode_frame(T.as_rgba(new))
            assert T.wire_bytes(directory) <= T.wire_bytes(d1)
            total += copied
            print(f"{name} moved by {move}: {copied} of {len(directory)} tiles COPY, {T.wire_bytes(directory)} bytes against {T.wire_bytes(d1)}")
    assert total > 50


@pytest.mark.parametrize("dy", [17, -17])
def test_in_place_decode_with_every_tile_a_copy_and_overlapping_sources(dy):
    """a scroll by 17: every tile's source reaches into a tile the same stream writes.  Decoding in place, in directory order and without
    staging, would read rows the stream has already overwritten (dy = -17: tile (0, 64) reads rows 47 .. 63, which tile (0, 0) wrote)."""
    w, h = 128, 128 + 17
    old = np.random.RandomState(8).randint(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    y0 = 0 if dy > 0 else 17
    rects = [(x, y0 + y, 64, 64) for y in (0, 64) for x in (0, 64)]  # (not bins of the frame for dy < 0: the decoder takes any tile inside the image)
    new = old.copy()
    new[y0:y0 + 128] = old[y0 + dy:y0 + dy + 128]
    directory, copied = _roundtrip(old, new, [(0, dy)], rects)
    assert copied == 4 and (directory["mode"] == M.COPY).all()
    naive = old.copy()
    for x, y, tw, th in rects:
        naive[y:y + th, x:x + tw] = naive[y + dy:y + dy + th, x:x + tw]
    if dy < 0:
        assert not np.array_equal(naive, new), "the case would not tell a decoder without staging from one with"


# ------------------------------------------------------------------------------------------------------------------ malformed streams
def _stream():
    """131 x 70 moved by (-2, 6), coded against [(-2, 6)]: COPY tiles, clipped ones among them, beside tiles with payloads"""
    w, h = 131, 70
    old = _content(w, h, 5)
    new = _scrolled(old, -2, 6)
    directory, blob, copied = M.encode_frame_moved(T.as_rgba(old), T.as_rgba(new), [(-2, 6)], T.tiles_of(w, h))
    assert copied >= 2 and copied < len(directory)
    return w, h, directory, blob, T.as_rgba(old), T.as_rgba(new)


def test_malformed_version_2_streams_are_refused_and_leave_the_image_alone():
    w, h, directory, blob, old, new = _stream()
    L = context.load()
    store = np.full((h, w + 9, 4), SENTINEL, np.uint8)
    store[:, :w] = old
    before = store.copy()
    pitch = store.strides[0]
    raw = np.frombuffer(blob, np.uint8)

    def call(d=directory, b=raw, image=True, pitch=pitch, n=None, tp=True, bp=True, nbytes=None, iw=w, ih=h, fn=L.fdh_decode_damage_moved):
        d, b = np.ascontiguousarray(d), np.ascontiguousarray(b)
        return fn(store.ctypes.data if image else None, pitch, iw, ih, d.ctypes.data if tp else None, len(d) if n is None else n,
                  b.ctypes.data if bp else None, len(b) if nbytes is None else nbytes)

    assert call() == 0 and np.array_equal(store[:, :w], new) and (store[:, w:] == SENTINEL).all()
    store[:] = before

    def edit(k, **fields):
        d = directory.copy()
        for name, v in fields.items():
            d[name][k] = v
        return d

    copies = np.flatnonzero(directory["mode"] == M.COPY)
    coded = np.flatnonzero((directory["mode"] != M.COPY) & (directory["mode"] != T.SOLID))
    c0, c1, p0 = int(copies[0]), int(copies[-1]), int(coded[0])
    x, y, tw, th = (int(directory[f][c1]) for f in "xywh")
    bad = [("null image", call(image=False)), ("null tiles", call(tp=False)), ("null payload", call(bp=False)), ("n_tiles < 0", call(n=-1)),
           ("payload_bytes < 0", call(nbytes=-1)), ("pitch", call(pitch=4 * w - 1))]
    # a COPY entry with a field it does not use
    bad += [("COPY with bits", call(edit(c0, bits=1))), ("COPY with n", call(edit(c0, n=1))), ("COPY with an offset", call(edit(c0, offset=16))),
            ("COPY with a size", call(edit(c0, size=4))), ("COPY with a size and an offset", call(edit(c1, size=16, offset=16)))]
    # a COPY source that is not inside the image: by one pixel on each side, and far away
    for what, dx, dy in (("left", -x - 1, 0), ("up", 0, -y - 1), ("right", w - tw - x + 1, 0), ("down", 0, h - th - y + 1), ("far", 0, 32767), ("far left", -32768, 0),
                         ("both", -x - 1, -y - 1)):
        bad.append((f"COPY source leaves the image: {what}", call(edit(c1, solid=M.move_word(dx, dy)))))
    bad.append(("COPY in an image that is smaller than the source", call(iw=w - 1)))
    # the modes beyond COPY, and the tile box
    bad += [("mode 5", call(edit(c0, mode=5))), ("mode 255", call(edit(p0, mode=255))), ("COPY w = 0", call(edit(c0, w=0))), ("COPY h = 65", call(edit(c0, h=65))),
            ("COPY x = -1", call(edit(c0, x=-1)))]
    # what version 1 refuses is still refused
    bad += [("size + 4", call(edit(p0, size=int(directory["size"][p0]) + 4))), ("offset + 4", call(edit(p0, offset=int(directory["offset"][p0]) + 4))),
            ("a colour outside SOLID and COPY", call(edit(p0, solid=1))), ("payload cut", call(nbytes=16)),
            ("a payload tile turned COPY keeps its size", call(edit(p0, mode=M.COPY, solid=M.move_word(0, 0))))]
    for what, rc in bad:
        assert rc == INVALID, f"{what}: returned {rc}"
    assert len(bad) >= 28
    assert np.array_equal(store, before), "a refused call wrote into the image"
    assert b"fdh_decode_damage_moved" in L.fdh_last_error()
    # the sources at the image's very edge are accepted, and so is a move of (0, 0): decodable, not canonical
    for dx, dy in ((-x, 0), (0, -y), (w - tw - x, 0), (0, h - th - y), (0, 0)):
        assert call(edit(c1, solid=M.move_word(dx, dy))) == 0, (dx, dy)
        want = new.copy()
        want[y:y + th, x:x + tw] = old[y + dy:y + dy + th, x + dx:x + dx + tw]
        assert np.array_equal(store[:, :w], want) and (store[:, w:] == SENTINEL).all(), (dx, dy)
        store[:] = before
    # fdh_decode_damage keeps refusing mode 4, and takes the same stream once its COPY tiles are left out
    assert call(fn=L.fdh_decode_damage) == INVALID and b"unknown mode" in L.fdh_last_error()
    assert np.array_equal(store, before)
    assert call(directory[directory["mode"] != M.COPY], fn=L.fdh_decode_damage) == 0
    store[:] = before
    # nothing to decode needs no arrays
    assert L.fdh_decode_damage_moved(None, pitch, w, h, None, 0, None, 0) == 0
    with pytest.raises(FigdrawHipError) as e:
        HipContext.decode_damage_moved(store[:, :w], edit(c0, n=3), blob)
    assert e.value.code == INVALID and np.array_equal(store, before)


# ------------------------------------------------------------------------------------------------------------------ the kernels' source on a CPU
def _tile_major(px):
    h, w = px.shape
    gx, gy = (w + 63) // 64, (h + 63) // 64
    full = np.zeros((gy * 64, gx * 64), np.uint32)
    full[:h, :w] = px
    return np.ascontiguousarray(full.reshape(gy, 64, gx, 64).transpose(0, 2, 1, 3)).reshape(gx * gy, 64, 64)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_damage_move.hip, fdh_damage_move.h and fdh_damage_read.h compiled as plain C++20 under the threaded shim of tests/emu with the
    driver of tests/move_emu -> the directory of ./emu and ./emu_san, the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "move_emu", ("k_damage_move.hip", "fdh_damage_move.h", "fdh_damage_read.h"), {"emu": (), "emu_san": emu_build.SAN},
                           flags=("-Wno-unknown-pragmas",), threads=True)


def _through_the_shim(tmp, what, old, new, moves, pre=None, max_shift=24, exe="./emu", garbage=False):
    """the three kernels over (the mirror of `old`, the surface `new`) against the reference.  pre: the pending bins before the filter
    ((bins_y, bins_x) bool; None: all = 1).  -> (moved per bin, the COPY tiles, the reference's candidates)"""
    h, w = new.shape
    gx, gy = (w + 63) // 64, (h + 63) // 64
    nb = gx * gy
    new.astype("<u4").tofile(tmp / "new.raw")
    mirror = _tile_major(old)
    if garbage:  # the words of a slot that lie past a clipped tile's edge are no pixels: the kernels may not read them as such
        if w % 64:
            mirror[gx - 1::gx, :, w % 64:] = 0xDEADBEEF
        if h % 64:
            mirror[nb - gx:, h % 64:, :] = 0xDEADBEEF
    mirror.astype("<u4").tofile(tmp / "mirror.raw")
    mine = np.ones((gy, gx), bool) if pre is None else pre
    differs = (_tile_major(old) != _tile_major(new)).any(axis=(1, 2)).reshape(gy, gx)
    post = mine & differs  # what k_damage_filter leaves
    others = np.array([EPOCH - 1, 3, 0], np.uint32)[np.arange(nb) % 3]  # the stamps a bin that is not pending can have
    if pre is not None:
        np.where(pre.reshape(-1), EPOCH, others).astype("<u4").tofile(tmp / "pre.raw")
    np.where(post.reshape(-1), EPOCH, others).astype("<u4").tofile(tmp / "post.raw")
    args = [exe, str(w), str(h), "new.raw", "mirror.raw", "-" if pre is None else "pre.raw", "post.raw", str(max_shift), str(len(moves))]
    r = subprocess.run(args + [str(v) for m in moves for v in m], cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{what}: {r.stdout}{r.stderr}"
    n, nbytes, n_copied = (int(v) for v in r.stdout.split())
    # k_damage_move_match: the first matching move for every bin that was pending, whatever its colours; nothing for the others
    moved = np.fromfile(tmp / "moved.bin", np.uint8).reshape(gy, gx)
    new_px = new
    for by in range(gy):
        for bx in range(gx):
            x, y = 64 * bx, 64 * by
            tile = new_px[y:y + 64, x:x + 64]
            k = M.matching_move(old, tile, x, y, moves)
            want = 0xEE if not mine[by, bx] else 0 if k is None else k + 1
            assert moved[by, bx] == want, f"{what}: moved[{by}, {bx}] = {moved[by, bx]}, the reference says {want}"
    # k_damage_move_votes
    got = np.fromfile(tmp / "votes.bin", "<u4").reshape(2, 513)
    Vv, Vh = M.votes(T.as_rgba(old), T.as_rgba(new), mine, max_shift)
    want = np.zeros((2, 513), np.uint32)
    for d, v in Vv.items():
        want[0, d + 256] = v
    for d, v in Vh.items():
        want[1, d + 256] = v
    assert np.array_equal(got, want), f"{what}: votes differ at (axis, d) {[(int(a), int(d) - 256) for a, d in zip(*np.nonzero(got != want))][:8]}"
    # k_damage_encode_moved
    rects = [rc for rc, m in zip(T.tiles_of(w, h), post.reshape(-1)) if m]
    wdir, wblob, wcopied = M.encode_frame_moved(T.as_rgba(old), T.as_rgba(new), moves, rects)
    if not rects:
        assert n == 0, what
        return moved, 0, M.find_moves(T.as_rgba(old), T.as_rgba(new), mine, max_shift)
    gdir, blob = np.fromfile(tmp / "dir.bin", T.ENTRY), open(tmp / "payload.bin", "rb").read()
    assert n == len(wdir) == len(gdir) and nbytes == len(wblob) == len(blob) and n_copied == wcopied, f"{what}: {(n, nbytes, n_copied)} against {(len(wdir), len(wblob), wcopied)}"
    used = np.zeros(len(blob), bool)
    for a, b in zip(gdir, wdir):
        assert all(a[f] == b[f] for f in ("x", "y", "w", "h", "mode", "bits", "n", "size", "solid")), f"{what}: {a} against {b}"
        size, at, ref = int(a["size"]), int(a["offset"]), int(b["offset"])
        if size == 0:
            assert at == 0, what
            continue
        assert at % 16 == 0 and not used[at:at + T.ceil16(size)].any(), what
        used[at:at + T.ceil16(size)] = True
        assert blob[at:at + size] == wblob[ref:ref + size], f"{what}: the payload of {a}"
        assert not any(blob[at + size:at + T.ceil16(size)]), what
    assert used.all(), what
    return moved, n_copied, M.find_moves(T.as_rgba(old), T.as_rgba(new), mine, max_shift)


def test_the_move_kernels_source_under_a_host_shim(shim):
    """figdraw_amd/csrc/k_damage_move.hip itself on a CPU (threads for lanes, barriers for __syncthreads and for a wave's lock step):
    moved[], the votes, and every entry and payload byte against tilemove_ref.  No device: the GPU tests hold the compiled kernels to the same."""
    total = 0
    # 256 x 192, nothing clipped: vertical, horizontal, a diagonal given as a hint, several moves of which the second is the true one
    old = _content(256, 192, 1)
    old[64:128, 64:128] = 0xFF123456
    old[128:150, 64:128] = 0xFF123456
    for move, moves in (((0, 17), [(0, 17)]), ((0, -64), [(3, 3), (0, -64)]), ((5, 0), [(5, 0), (0, 17)]), ((3, -9), [(0, -9), (3, 0), (3, -9)])):
        new = _scrolled(old, *move)
        moved, copied, cands = _through_the_shim(shim, f"256 x 192 moved by {move}", old, new, moves, max_shift=64 if move == (0, -64) else 24)
        assert copied > 0 and (moved == moves.index(move) + 1).sum() >= copied
        if 0 in move:
            assert cands[0][0] == move, (move, cands[:3])
        total += copied
    # a one-colour tile that matches the move: k_damage_move_match says so, the encoder stores SOLID
    new = _scrolled(old, 0, 17)
    moved, copied, _ = _through_the_shim(shim, "one colour", old, new, [(0, 17)])
    assert moved[1, 1] == 1 and copied == 7
    # some bins pending, the last one not; then the last one alone
    pre = np.random.RandomState(2).rand(3, 4) < 0.5
    pre[0, 0], pre[2, 3] = True, False
    _through_the_shim(shim, "some bins pending", old, new, [(0, 17)], pre)
    _through_the_shim(shim, "the last bin alone", old, new, [(0, -17), (0, 17)], np.arange(12).reshape(3, 4) == 11)
    # the same frame again: the filter leaves nothing; and no moves at all
    _through_the_shim(shim, "unchanged", old, old.copy(), [(0, 17)])
    _through_the_shim(shim, "no moves", old, new, [])
    # 131 x 70: clipped bins, rows that are not 16-byte aligned; the mirror's words past the tiles' edges hold garbage
    old = _content(131, 70, 5)
    for move in ((0, 6), (-2, 6), (5, 0), (3, -4)):
        new = _scrolled(old, *move)
        moved, copied, _ = _through_the_shim(shim, f"131 x 70 moved by {move}", old, new, [(7, 7), move], garbage=True)
        total += copied
        if move in ((-2, 6), (5, 0)):
            assert copied > 0, move
    # 64 x 64: one bin, no source inside the frame for any move
    old = _content(64, 64, 7)
    moved, copied, cands = _through_the_shim(shim, "64 x 64", old, _scrolled(old, 0, 9), [(0, 9), (0, -9), (1, 0)])
    assert copied == 0 and not moved.any() and cands and cands[0][0] == (0, 9)
    # the mover at its full reach, on a frame taller than 2 x 256 rows
    old = _content(128, 640, 9)
    _, _, cands = _through_the_shim(shim, "128 x 640 moved by (0, 256)", old, _scrolled(old, 0, 256), [(0, 256)], max_shift=256)
    assert cands[0][0] == (0, 256)
    _, _, cands = _through_the_shim(shim, "128 x 640 moved by (0, -200)", old, _scrolled(old, 0, -200), [(0, -200)], max_shift=200)
    assert cands[0][0] == (0, -200)
    assert total > 20


def test_the_move_kernels_once_under_sanitizers(shim):
    old = _content(131, 70, 5)
    _through_the_shim(shim, "131 x 70 under ASan and UBSan", old, _scrolled(old, -2, 6), [(7, 7), (-2, 6)], exe="./emu_san", garbage=True)


def test_the_decoder_fuzzed_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/move_emu/fuzz.cpp + figdraw_amd/csrc/fdh_tile_decode.cpp, which includes no HIP: a stand-alone program under AddressSanitizer
    and UBSan over mutated version-2 streams"""
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "move_emu", "fuzz.cpp"), os.path.join(CSRC, "fdh_tile_decode.cpp"), "-o", str(tmp_path / "fuzz")])
    for name in ("fdh_tile_decode.cpp", "fdh_tile_decode.h"):
        included = re.findall(r'#include\s+[<"]([^>"]+)', open(os.path.join(CSRC, name)).read())
        assert not any(i.startswith("hip/") or i.startswith("fdh_") and i != "fdh_tile_decode.h" for i in included), (name, included)
    w, h, directory, blob, old, _ = _stream()
    old.tofile(tmp_path / "image.raw")
    directory.tofile(tmp_path / "dir.bin")
    open(tmp_path / "payload.bin", "wb").write(blob)
    r = subprocess.run([str(tmp_path / "fuzz"), str(w), str(h), "image.raw", "dir.bin", "payload.bin", "3000"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    accepted, refused = (int(v) for v in re.search(r"fuzz: OK (\d+) (\d+)", r.stdout).groups())
    assert accepted > 30 and refused > 300, (accepted, refused)
