"""Coded damage readback, the host side (include/figdraw_hip_stream.h): the header and the C ABI, and the host-only decoder
fdh_decode_damage against tests/tilecode_ref.py -- a numpy encoder and decoder written from the header's text.  Everything here is
equality of bytes and of byte counts: the code is lossless, and its sizes are rules, not measurements."""
import os
import re
import subprocess

import numpy as np
import pytest

import emu_build
import tilecode_ref as T
from conftest import load_png
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "figdraw_hip_stream.h")
NEW_API = ("fdh_read_damage_coded", "fdh_decode_damage", "fdh_coded_damage_bound")
INVALID, NO_DEVICE = -1, -2
SENTINEL = 0xA5

# the committed frames and what each codes to: 24 bytes of directory per tile plus each payload rounded up to 16 bytes
GOLDEN = {"ref_render_circle_rect.png": 11856, "ref_render_line_rect.png": 15888, "ref_render_layers_clip.png": 19632,
          "ref_render_rgb_boxes.png": 62272, "ref_render_rgb_boxes_sdf.png": 124928, "ref_render_image.png": 124800,
          "ref_render_linear_gradient.png": 204944, "ss_blur_big_checker_r64.png": 231552, "ss_glyphs_small.png": 41072,
          "ss_blur_big_noise_r18.png": 2100224}


# ------------------------------------------------------------------------------------------------------------------ header and ABI
def test_header_declares_and_library_exports_the_stream_api():
    src = open(HEADER).read()
    assert '#include "figdraw_hip.h"' in src
    declared = re.findall(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(", src)
    assert sorted(declared) == sorted(NEW_API)
    for name, value in (("SOLID", 0), ("PAL", 1), ("RUNS", 2), ("RAW", 3)):
        assert re.search(r"FDH_TILE_%s\s*=\s*%d\b" % (name, value), src)
    L = context.load()
    for name in NEW_API:
        assert hasattr(L, name), name
    for other in ("figdraw_hip.h", "figdraw_hip_damage.h", "figdraw_hip_pick.h", "figdraw_hip_readback.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(r"\b%s\b" % n, text) for n in NEW_API), other
    assert HipContext.CODED_TILE == T.ENTRY and T.ENTRY.itemsize == 24
    assert HipContext.coded_damage_bound(3840, 2160) == 60 * 34 * 16384 and HipContext.coded_damage_bound(130, 70) == 6 * 16384
    assert HipContext.coded_damage_bound(0, 5) == 0


def test_stream_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "stream_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "stream_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream_abi_smoke: OK" in r.stdout
    src = open(os.path.join(ROOT, "tests", "stream_abi_smoke.c")).read()
    assert all(re.search(r"\b%s\b" % n, src) for n in NEW_API)
    assert all(re.search(r"\bFDH_TILE_%s\b" % m, src) for m in ("SOLID", "PAL", "RUNS", "RAW")), "the smoke decodes one tile per mode"


def test_record_only_context_refuses_the_coded_read():
    ctx = HipContext(record_only=True)
    with pytest.raises(FigdrawHipError) as e:
        ctx.read_damage_coded()
    assert e.value.code == NO_DEVICE
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ known answers
SIZES = ((64, 64), (2, 6), (1, 1), (64, 6))  # w x h: a whole bin, the clipped corner of a 130 x 70 frame, one pixel, a clipped last row


def _colours(n, seed=1):
    """n distinct colours, among them the extremes 0 and 0xFFFFFFFF (their order as UNSIGNED values is what a palette sorts by)"""
    rng = np.random.RandomState(seed)
    fixed = [0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF][:n]
    more = [int(v) for v in np.unique(rng.randint(1, 0x7FFFFFFF, 2 * n + 8, dtype=np.int64) * 2 + 2) if v not in fixed]
    c = np.array(fixed + more[:n - len(fixed)], np.uint32)
    assert len(np.unique(c)) == n
    return c


def _tile(w, h, kind, seed=0):
    """a hand-built tile (uint32 (h, w)) of w h = px pixels"""
    px = w * h
    rng = np.random.RandomState(100 + seed)
    if kind == "solid":
        flat = np.full(px, 0xFF336699, np.uint32)
    elif kind.startswith("pal"):  # n colours scattered pixel by pixel: runs are short, so PAL beats RUNS where it beats RAW
        n = int(kind[3:])
        flat = _colours(n, seed)[np.concatenate((np.arange(n), rng.randint(0, n, max(px - n, 0))))[:px]]
        rng.shuffle(flat)
    elif kind == "runs":  # a few long runs, none of which ends where a row ends
        cuts = sorted(set(rng.randint(1, px, 5).tolist()) - set(range(0, px + 1, w))) if px > 2 else [1]
        flat = np.repeat(_colours(len(cuts) + 1, seed), np.diff([0] + cuts + [px])).astype(np.uint32)
    else:  # "raw": every pixel another colour
        flat = (np.arange(px, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5A5A5A5A)
    return flat.reshape(h, w)


def _decode_one(tile_px):
    """the tile through tilecode_ref.encode and fdh_decode_damage, into a sentinel image a little larger than the tile with a row pitch"""
    h, w = tile_px.shape
    mode, n, solid, data = T.encode(tile_px)
    store = np.full((h + 2, w + 2 + 3, 4), SENTINEL, np.uint8)
    image = store[:, :w + 2]
    e = T.entry(1, 1, w, h, mode, n, solid, len(data), 0)
    blob = data + bytes(T.ceil16(len(data)) - len(data))
    HipContext.decode_damage(image, e, blob)
    return mode, n, image, store, (e, blob)


@pytest.mark.parametrize("w,h", SIZES)
def test_known_answers_one_tile_per_mode(w, h):
    # which mode each hand-built tile must get, by the header's size rules.  12 pixels (2 x 6) can never be RUNS: two runs are 12 bytes
    # and tie with PAL's 8 + 4, which is the lower mode; three runs are 20 against 12 + 4.  One pixel is one colour.
    cases = {(64, 64): (("solid", T.SOLID), ("pal2", T.PAL), ("runs", T.RUNS), ("raw", T.RAW)),
             (64, 6): (("solid", T.SOLID), ("pal2", T.PAL), ("runs", T.RUNS), ("raw", T.RAW)),
             (2, 6): (("solid", T.SOLID), ("pal2", T.PAL), ("runs", T.PAL), ("raw", T.RAW)),
             (1, 1): (("solid", T.SOLID), ("raw", T.SOLID))}[(w, h)]
    for kind, want_mode in cases:
        tile = _tile(w, h, kind)
        mode, n, solid, data = T.encode(tile)
        assert mode == want_mode, (kind, mode)
        assert np.array_equal(T.decode(mode, n, solid, data, w, h), tile), kind
        _, _, image, store, _ = _decode_one(tile)
        assert np.array_equal(T.as_u32(image[1:1 + h, 1:1 + w]), tile), kind
        frame = store.copy()
        frame[1:1 + h, 1:1 + w] = SENTINEL
        assert (frame == SENTINEL).all(), f"{kind}: bytes around the tile, or the pitch padding, were written"


@pytest.mark.parametrize("n,bits", [(2, 1), (3, 2), (4, 2), (5, 4), (16, 4), (17, 8), (256, 8)])
def test_palette_tiles_at_each_index_width(n, bits):
    tile = _tile(64, 64, "pal%d" % n)
    mode, got_n, solid, data = T.encode(tile)
    assert (mode, got_n, solid) == (T.PAL, n, 0) and T.pal_bits(n) == bits
    assert len(data) == 4 * n + 4 * (4096 * bits // 32)
    pal = np.frombuffer(data, "<u4", n)
    assert (np.diff(pal.astype(np.int64)) > 0).all(), "the palette ascends as unsigned values"
    assert pal[0] == 0 and pal[-1] == 0xFFFFFFFF
    # pixel i's index sits in bits [(i b) % 32, +b) of word (i b) / 32
    words = np.frombuffer(data, "<u4", offset=4 * n)
    for i in (0, 1, 31, 32, 33, 4095):
        at = i * bits
        assert pal[(int(words[at // 32]) >> (at % 32)) & ((1 << bits) - 1)] == tile.flat[i]
    _, _, image, _, _ = _decode_one(tile)
    assert np.array_equal(T.as_u32(image[1:65, 1:65]), tile)
    assert np.array_equal(T.decode(mode, n, 0, data, 64, 64), tile)


def test_a_clipped_palette_tile_leaves_its_last_words_unused_bits_zero():
    tile = _tile(2, 6, "pal3")  # 12 pixels at 2 bits: 24 bits of one word
    mode, n, _, data = T.encode(tile)
    assert (mode, n, len(data)) == (T.PAL, 3, 16)
    assert np.frombuffer(data, "<u4", offset=12)[0] >> 24 == 0
    _, _, image, _, _ = _decode_one(tile)
    assert np.array_equal(T.as_u32(image[1:7, 1:3]), tile)


def test_257_colours_are_not_a_palette():
    cols = _colours(257)
    flat = np.concatenate((cols, np.full(4096 - 257, cols[5], np.uint32))).astype(np.uint32)
    np.random.RandomState(5).shuffle(flat)
    tile = flat.reshape(64, 64)
    assert len(np.unique(tile)) == 257
    mode, n, _, data = T.encode(tile)
    assert mode in (T.RUNS, T.RAW) and mode == T.RUNS and n > 257  # (about 480 runs: 2.9 KB against RAW's 16 KB)
    _, _, image, _, _ = _decode_one(tile)
    assert np.array_equal(T.as_u32(image[1:65, 1:65]), tile)
    assert T.encode(_tile(64, 64, "pal256"))[0] == T.PAL  # one colour fewer, scattered: a palette


def test_runs_cross_row_ends_and_one_run_is_solid():
    flat = np.repeat(np.array([0x11111111, 0x22222222, 0x11111111], np.uint32), [100, 3000, 996])  # 64-pixel rows: every run crosses some
    tile = flat.reshape(64, 64)
    mode, n, _, data = T.encode(tile)
    assert (mode, n, len(data)) == (T.RUNS, 3, 20)
    assert np.frombuffer(data, "<u2", 3, offset=12).tolist() == [99, 2999, 995] and data[18:] == b"\0\0"
    _, _, image, _, _ = _decode_one(tile)
    assert np.array_equal(T.as_u32(image[1:65, 1:65]), tile)
    one = np.full((64, 64), 0xDEADBEEF, np.uint32)  # one run of 4096
    assert T.encode(one) == (T.SOLID, 0, 0xDEADBEEF, b"")
    assert T.payloads(one)[T.RUNS][0] == 1
    _, _, image, _, _ = _decode_one(one)
    assert (T.as_u32(image[1:65, 1:65]) == 0xDEADBEEF).all()


def test_ties_go_to_the_lower_mode():
    # 64 x 1, two colours alternating in runs of ... : PAL = 8 + 8 = 16 bytes; RUNS of 2 runs = 12 bytes -> RUNS; of 3 runs = 20 -> PAL
    a, b = 0x01020304, 0x0A0B0C0D
    assert T.encode(np.repeat(np.array([a, b], np.uint32), [10, 54]).reshape(1, 64))[0] == T.RUNS
    assert T.encode(np.repeat(np.array([a, b, a], np.uint32), [10, 44, 10]).reshape(1, 64))[0] == T.PAL
    # 2 x 2 with two runs: PAL = 8 + 4 = 12, RUNS = 12, RAW = 16: the tie goes to PAL
    assert T.encode(np.array([[a, a], [b, b]], np.uint32))[0] == T.PAL
    # 2 x 1 with two colours: PAL = 12, RUNS = 12, RAW = 8
    assert T.encode(np.array([[a, b]], np.uint32))[0] == T.RAW
    # a non-canonical but decodable stream is accepted: the same tile as split runs
    tile = np.full((2, 3), a, np.uint32)
    data = np.array([a, a], "<u4").tobytes() + np.array([3, 1], "<u2").tobytes()
    image = np.full((2, 3, 4), SENTINEL, np.uint8)
    HipContext.decode_damage(image, T.entry(0, 0, 3, 2, T.RUNS, 2, 0, 12, 0), data + bytes(4))
    assert np.array_equal(T.as_u32(image), tile)
    # ... and an unsorted palette
    data = np.array([b, a], "<u4").tobytes() + np.array([0b010101], "<u4").tobytes()
    HipContext.decode_damage(image, T.entry(0, 0, 3, 2, T.PAL, 2, 0, 12, 0), data + bytes(4))
    assert (T.as_u32(image).reshape(-1) == [a, b, a, b, a, b]).all()


# ------------------------------------------------------------------------------------------------------------------ golden frames
def test_golden_frames_through_the_c_decoder():
    seen = np.zeros(4, np.int64)
    for name, coded in GOLDEN.items():
        want = load_png(name)
        h, w = want.shape[:2]
        directory, blob = T.encode_frame(want)
        assert len(directory) == ((w + 63) // 64) * ((h + 63) // 64), f"{name}: a tile was left out"
        assert T.wire_bytes(directory) == coded, f"{name}: {T.wire_bytes(directory)} bytes, the size rules give {coded}"
        assert len(blob) <= HipContext.coded_damage_bound(w, h)
        store = np.full((h, w + 5, 4), SENTINEL, np.uint8)
        image = store[:, :w]
        HipContext.decode_damage(image, directory, blob)
        assert np.array_equal(image, want), name
        assert (store[:, w:] == SENTINEL).all(), f"{name}: the pitch padding was written"
        # payloads out of directory order decode to the same frame
        order = np.random.RandomState(3).permutation(len(directory))
        moved, blob2, at = directory.copy(), bytearray(len(blob)), 0
        for k in order:
            size, off = int(directory["size"][k]), int(directory["offset"][k])
            blob2[at:at + size] = blob[off:off + size]
            moved["offset"][k] = at if size else 0
            at += T.ceil16(size)
        image[:] = SENTINEL
        HipContext.decode_damage(image, moved, bytes(blob2))
        assert np.array_equal(image, want), f"{name}, payloads shuffled"
        seen += np.bincount(directory["mode"], minlength=4)
    assert (seen > 0).all(), f"a mode was never chosen over the golden frames: {seen.tolist()}"


# ------------------------------------------------------------------------------------------------------------------ malformed streams
def _stream():
    """130 x 70 (a 3 x 2 grid, last column 2 wide, last row 6 high), one tile of each mode and two more: directory, blob, the frame"""
    w, h = 130, 70
    px = np.zeros((h, w), np.uint32)
    px[0:64, 0:64] = 0xFF0000FF                                  # bin (0, 0): SOLID
    px[0:64, 64:128] = _tile(64, 64, "pal5")                     # bin (1, 0): PAL, 4 bits
    px[0:64, 128:130] = _tile(2, 64, "runs", 1)                  # bin (2, 0): RUNS
    px[64:70, 0:64] = _tile(64, 6, "raw")                        # bin (0, 1): RAW
    px[64:70, 64:128] = _tile(64, 6, "pal2", 2)                  # bin (1, 1): PAL, 1 bit
    px[64:70, 128:130] = _tile(2, 6, "pal3", 3)                  # bin (2, 1): PAL, 2 bits (12 pixels are never RUNS)
    directory, blob = T.encode_frame(T.as_rgba(px))
    assert directory["mode"].tolist() == [T.SOLID, T.PAL, T.RUNS, T.RAW, T.PAL, T.PAL]
    return w, h, directory, blob, T.as_rgba(px)


def test_malformed_streams_are_refused_and_leave_the_image_alone():
    w, h, directory, blob, want = _stream()
    L = context.load()
    store = np.full((h, w + 9, 4), SENTINEL, np.uint8)
    pitch = store.strides[0]
    raw = np.frombuffer(blob, np.uint8)

    def call(d=directory, b=raw, image=True, pitch=pitch, n=None, tp=True, bp=True, nbytes=None, iw=w, ih=h):
        d = np.ascontiguousarray(d)
        b = np.ascontiguousarray(b)
        return L.fdh_decode_damage(store.ctypes.data if image else None, pitch, iw, ih, d.ctypes.data if tp else None, len(d) if n is None else n,
                                   b.ctypes.data if bp else None, len(b) if nbytes is None else nbytes)

    assert call() == 0 and np.array_equal(store[:, :w], want) and (store[:, w:] == SENTINEL).all()
    store[:] = SENTINEL
    bad = []

    def edit(k, **fields):
        d = directory.copy()
        for name, v in fields.items():
            d[name][k] = v
        return d

    SOL, PAL4, RUN, RAW, PAL1, PAL2 = range(6)
    # null pointers, counts, the pitch
    bad += [("null image", call(image=False)), ("null tiles", call(tp=False)), ("null payload", call(bp=False)), ("n_tiles < 0", call(n=-1)),
            ("payload_bytes < 0", call(nbytes=-1)), ("pitch", call(pitch=4 * w - 1))]
    # a tile outside the image, or with w or h outside 1 .. 64
    for k, f, v in ((SOL, "w", 0), (SOL, "w", 65), (SOL, "h", 0), (SOL, "h", 65), (SOL, "x", -1), (SOL, "y", -64), (RUN, "x", 129), (PAL2, "y", 65),
                    (RAW, "h", 7)):
        bad.append((f"tile {k} {f} = {v}", call(edit(k, **{f: v}))))
    bad.append(("an image smaller than the frame", call(iw=w - 1)))
    bad.append(("an image lower than the frame", call(ih=h - 1)))
    # the mode
    bad += [("mode 4", call(edit(RAW, mode=4))), ("mode 255", call(edit(SOL, mode=255)))]
    # bits that do not match n
    bad += [("PAL 5 colours at 8 bits", call(edit(PAL4, bits=8))), ("PAL 5 colours at 2 bits", call(edit(PAL4, bits=2))), ("PAL bits 0", call(edit(PAL1, bits=0))),
            ("PAL bits 3", call(edit(PAL4, bits=3))), ("bits outside PAL", call(edit(RAW, bits=8))), ("PAL n = 0", call(edit(PAL1, n=0, bits=1))),
            ("PAL n = 257", call(edit(PAL4, n=257, bits=8)))]
    # a size that does not match (mode, n, w, h)
    for k in (SOL, PAL4, RUN, RAW):
        bad.append((f"tile {k} size + 4", call(edit(k, size=int(directory["size"][k]) + 4))))
    bad += [("RAW size - 4", call(edit(RAW, size=int(directory["size"][RAW]) - 4))), ("RUNS n + 1", call(edit(RUN, n=int(directory["n"][RUN]) + 1))),
            ("PAL n - 1, same size", call(edit(PAL4, n=4, bits=2))), ("RUNS n = 0", call(edit(RUN, n=0, size=0))),
            ("SOLID with n", call(edit(SOL, n=1))), ("RAW with a colour", call(edit(RAW, solid=1))), ("SOLID with an offset", call(edit(SOL, offset=16)))]
    # the offset
    bad += [("offset + 4", call(edit(RAW, offset=int(directory["offset"][RAW]) + 4))), ("offset + 8", call(edit(PAL4, offset=int(directory["offset"][PAL4]) + 8))),
            ("offset beyond the payload", call(edit(PAL2, offset=T.ceil16(len(blob))))), ("offset 2^32 - 16", call(edit(RAW, offset=0xFFFFFFF0)))]
    # truncated payloads: the last tile's payload ends the blob
    end = int(directory["offset"][PAL2]) + int(directory["size"][PAL2])
    assert T.ceil16(end) == len(blob)
    for cut in (end - 1, end - 4, 16, 0):
        bad.append((f"payload cut to {cut}", call(nbytes=cut)))
    assert call(nbytes=end) == 0  # (the zeros of the last round-up are not needed)
    store[:] = SENTINEL
    # a palette index >= n
    b = raw.copy()
    at = int(directory["offset"][PAL4]) + 4 * 5
    b[at] |= 0x0F  # pixel 0: index 15 of 5 colours
    bad.append(("palette index 15 of 5", call(b=b)))
    b = raw.copy()
    b[at + 4 * (4096 * 4 // 32) - 1] = 0x50  # the last pixel: index 5 of 5
    bad.append(("palette index 5 of 5 in the last pixel", call(b=b)))
    # run lengths that do not sum to w h
    for delta in (1, -1):
        b = raw.copy()
        at = int(directory["offset"][RUN]) + 4 * int(directory["n"][RUN])
        b[at:at + 2] = np.array([int(np.frombuffer(blob, "<u2", 1, offset=at)[0]) + delta], "<u2").view(np.uint8)
        bad.append((f"run lengths sum to w h {delta:+d}", call(b=b)))
    b = raw.copy()
    at = int(directory["offset"][RUN]) + 4 * int(directory["n"][RUN])
    b[at:at + 2] = 0xFF  # a run of 65536 in a tile of 128 pixels
    bad.append(("a run longer than the tile", call(b=b)))
    for what, rc in bad:
        assert rc == INVALID, f"{what}: returned {rc}"
    assert len(bad) > 45
    assert (store == SENTINEL).all(), "a refused call wrote into the image"
    assert b"fdh_decode_damage" in L.fdh_last_error()
    # nothing to decode needs no arrays
    assert L.fdh_decode_damage(None, pitch, w, h, None, 0, None, 0) == 0
    HipContext.decode_damage(store[:, :w], np.zeros(0, T.ENTRY), b"")
    assert (store == SENTINEL).all()


def test_the_binding_raises_on_a_refused_stream():
    w, h, directory, blob, _ = _stream()
    image = np.full((h, w, 4), SENTINEL, np.uint8)
    with pytest.raises(FigdrawHipError) as e:
        HipContext.decode_damage(image, directory, blob[:100])
    assert e.value.code == INVALID and (image == SENTINEL).all()
    with pytest.raises(ValueError):
        HipContext.decode_damage(image[:, :, :3], directory, blob)


# ------------------------------------------------------------------------------------------------------------------ the kernel's source on a CPU
def test_the_encode_kernel_source_under_a_host_shim(tmp_path):
    """figdraw_amd/csrc/k_damage_codec.hip itself, compiled as C++20 against the threaded shim of tests/emu (threads for lanes, a barrier
    for __syncthreads) with the driver of tests/codec_emu: every entry and payload byte against tilecode_ref.  No device: the GPU tests
    hold the compiled kernel to the same."""
    # the library's own files: the kernel, and the parameter block and device code it shares
    emu_build.build(tmp_path, "codec_emu", ("k_damage_codec.hip", "fdh_damage_read.h"), {"emu": ()}, threads=True)

    def check(what, px, mask=None):
        h, w = px.shape
        px.astype("<u4").tofile(tmp_path / "frame.raw")
        rects, args = T.tiles_of(w, h), ["./emu", str(w), str(h), "frame.raw", "1", "-"]
        if mask is not None:
            np.where(mask.reshape(-1), 7, 3).astype("<u4").tofile(tmp_path / "stamps.raw")
            rects, args = [r for r, m in zip(rects, mask.reshape(-1)) if m], args[:4] + ["0", "stamps.raw"]
        r = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, what + ": " + r.stdout + r.stderr
        n, nbytes = (int(v) for v in r.stdout.split())
        got, blob = np.fromfile(tmp_path / "dir.bin", T.ENTRY), open(tmp_path / "payload.bin", "rb").read()
        want, wblob = T.encode_frame(T.as_rgba(px), rects)
        assert n == len(want) == len(got) and nbytes == len(wblob) == len(blob), what
        used = np.zeros(len(blob), bool)
        for a, b in zip(got, want):
            assert all(a[f] == b[f] for f in ("x", "y", "w", "h", "mode", "bits", "n", "size", "solid")), f"{what}: {a} against {b}"
            size, at, ref = int(a["size"]), int(a["offset"]), int(b["offset"])
            assert at % 16 == 0 and not used[at:at + T.ceil16(size)].any(), what
            used[at:at + T.ceil16(size)] = True
            assert blob[at:at + size] == wblob[ref:ref + size], f"{what}: the payload of {a}"
            assert not any(blob[at + size:at + T.ceil16(size)]), what
        assert used.all(), what
        return np.bincount(got["mode"], minlength=4)

    frame = np.zeros((128, 64 * 8 + 2), np.uint32)  # a 9 x 2 grid whose last column is 2 pixels wide
    for k, kind in enumerate(["pal2", "pal3", "pal4", "pal5", "pal16", "pal17", "pal256", "solid"]):
        frame[:64, 64 * k:64 * k + 64] = _tile(64, 64, kind)
    cols = _colours(257)
    flat = np.concatenate((cols, np.full(4096 - 257, cols[5], np.uint32)))
    np.random.RandomState(5).shuffle(flat)
    frame[64:, 0:64] = flat.reshape(64, 64)
    frame[64:, 64:128], frame[64:, 128:192] = _tile(64, 64, "runs"), _tile(64, 64, "raw")
    frame[64:, 192:256] = np.repeat(np.array([1, 2, 1], np.uint32), [100, 3000, 996]).reshape(64, 64)
    frame[:, 512:] = _tile(2, 128, "pal3")
    assert (check("synthetic", frame) > 0).all(), "every mode occurs"
    mask = np.random.RandomState(1).rand(2, 9) < 0.4
    mask[1, 8] = False
    check("synthetic, some bins pending", frame, mask)
    check("synthetic, the last bin alone", frame, ~np.ones((2, 9), bool) | (np.arange(18).reshape(2, 9) == 17))
    check("gradient 130 x 70", T.as_u32(load_png("ref_render_linear_gradient.png")[100:170, 300:430].copy()))
    check("noise 129 x 65", T.as_u32(load_png("ss_blur_big_noise_r18.png")[:65, :129].copy()))
    check("glyphs", T.as_u32(load_png("ss_glyphs_small.png")))
    for w, h in SIZES:
        for kind in ("solid", "pal3", "raw"):
            check(f"{w} x {h} {kind}", _tile(w, h, kind) if w * h >= 3 or kind != "pal3" else _tile(w, h, "solid"))
