"""Decoded video frames (fdh_put_video_frame, fdh_update_video_frame, fdh_video_coefficients; include_glyphs/figdraw_hip_video_frame.h), what a
CPU can check: the coefficients against their derivation from the standards' constants; known answers of the reference
tests/video_frame_ref.py; the integer rule against float64 within the bound the header derives; the calls' rules on a record-only context
and through C99; and the source of k_video_import.hip under the host shim of tests/emu (tests/video_frame_emu) against the reference, byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_build
import video_frame_cases as VC
import video_frame_ref as REF
from conftest import GOLDEN, ROOT
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext, VideoFrame

INVALID = -1
ROWS = [(fmt, m, r) for fmt in (REF.NV12, REF.P010) for m in (REF.BT601, REF.BT709, REF.BT2020) for r in (REF.LIMITED, REF.FULL)]
TABLE = {  # the header's table: {cY, cRV, cGU, cGV, cBU} per (bits, range) column and matrix row
    (8, 0): [(19077, 26149, 6419, 13320, 33050), (19077, 29372, 3494, 8731, 34610), (19077, 27503, 3069, 10657, 35091)],
    (8, 1): [(16384, 22970, 5638, 11700, 29032), (16384, 25802, 3069, 7670, 30402), (16384, 24160, 2696, 9361, 30825)],
    (10, 0): [(4769, 6537, 1605, 3330, 8263), (4769, 7343, 873, 2183, 8652), (4769, 6876, 767, 2664, 8773)],
    (10, 1): [(4084, 5726, 1405, 2917, 7237), (4084, 6431, 765, 1912, 7578), (4084, 6022, 672, 2333, 7684)],
}


# ------------------------------------------------------------------------------------------------------------------ 1. the rule
def test_coefficients_are_the_derivation_and_the_table():
    assert len(ROWS) == 12
    for fmt, m, r in ROWS:
        got = context.video_coefficients(fmt, m, r)
        assert got == REF.coefficients(fmt, m, r), (fmt, m, r)
        bits = REF.bits_of(fmt)
        s = 1 << (bits - 8)
        assert got[:2] == ((16 * s if r == REF.LIMITED else 0), 128 * s) and got[2:] == TABLE[(bits, r)][m], (fmt, m, r)
    L = context.load()
    out = (C.c_int32 * 7)()
    for bad in ((REF.BGRA8, 0, 0), (3, 0, 0), (REF.NV12, 3, 0), (REF.NV12, 0, 2)):
        assert L.fdh_video_coefficients(*bad, out) == INVALID and L.fdh_last_error().decode().startswith("video_coefficients: ")
    assert L.fdh_video_coefficients(REF.NV12, 0, 0, None) == INVALID


def one(Y, cb, cr, fmt, m, r):
    return REF.yuv_to_rgba(np.array([Y]), np.array([cb]), np.array([cr]), fmt, m, r)[0].tolist()


def test_conversion_known_answers():
    for m in (REF.BT601, REF.BT709, REF.BT2020):
        assert one(16, 128, 128, REF.NV12, m, REF.LIMITED) == [0, 0, 0, 255]
        assert one(235, 128, 128, REF.NV12, m, REF.LIMITED) == [255, 255, 255, 255]
        assert one(0, 128, 128, REF.NV12, m, REF.FULL) == [0, 0, 0, 255]
        assert one(255, 128, 128, REF.NV12, m, REF.FULL) == [255, 255, 255, 255]
        assert one(64, 512, 512, REF.P010, m, REF.LIMITED) == [0, 0, 0, 255] and one(940, 512, 512, REF.P010, m, REF.LIMITED) == [255, 255, 255, 255]
        assert one(1023, 512, 512, REF.P010, m, REF.FULL) == [255, 255, 255, 255]
        for below in (0, 7, 15):  # values below Yoff clamp; above Yoff + Yden too
            assert one(below, 128, 128, REF.NV12, m, REF.LIMITED) == [0, 0, 0, 255]
        assert one(255, 128, 128, REF.NV12, m, REF.LIMITED) == [255, 255, 255, 255]
    # the stored P010 words: the sample sits in the ten high bits, the six low ones are ignored
    black = REF.convert(np.array([[64 << 6, (64 << 6) | 63]], np.uint16), np.array([[[512 << 6, (512 << 6) | 63]]], np.uint16), REF.P010, REF.BT709, REF.LIMITED)
    assert black.tolist() == [[[0, 0, 0, 255], [0, 0, 0, 255]]]
    r, g, b, a = one(63, 102, 240, REF.NV12, REF.BT709, REF.LIMITED)  # the BT709 limited red primary
    assert r == 255 and g <= 1 and b <= 1 and a == 255


def _check_against_float(fmt, m, r, Y, cb, cr):
    """the header's bound: |integer byte - rounded float64 byte| <= 1, and 0 wherever the exact value is more than 0.094 from a half.
    -> the number of bytes that differ"""
    got = REF.yuv_to_rgba(Y, cb, cr, fmt, m, r)[..., :3].astype(np.int64)
    exact = REF.yuv_to_rgb_float(Y, cb, cr, fmt, m, r)
    want = np.clip(np.rint(exact), 0, 255).astype(np.int64)
    d = np.abs(got - want)
    from_half = np.abs(exact - np.floor(exact) - 0.5)
    assert d.max() <= 1, (fmt, m, r, int(d.max()))
    assert not (d[from_half > 0.094]).any(), (fmt, m, r)
    return int((d > 0).sum())


def test_integer_rule_against_float64_on_every_8_bit_triple():
    """all 2^24 triples for BT709 limited and BT601 full.  R depends on (Y, Cr) and B on (Y, Cb) only, so a slab of 16 luma values times
    every chroma pair covers each triple once"""
    cb, cr = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for m, r in ((REF.BT709, REF.LIMITED), (REF.BT601, REF.FULL)):
        differ = 0
        for y0 in range(0, 256, 16):
            Y = np.arange(y0, y0 + 16)[:, None, None] + np.zeros((1, 256, 256), np.int64)
            differ += _check_against_float(REF.NV12, m, r, Y, cb[None] + 0 * Y, cr[None] + 0 * Y)
        print(f"matrix {m} range {r}: {differ} of {3 << 24} bytes differ by 1, each within 0.094 of a tie")


def test_integer_rule_against_float64_on_samples():
    rng = np.random.default_rng(5)
    for fmt, m, r in ROWS:
        top = 1 << REF.bits_of(fmt)
        Y, cb, cr = (rng.integers(0, top, size=400_000) for _ in range(3))
        _check_against_float(fmt, m, r, Y, cb, cr)


def test_upsampling_known_answers():
    const = np.full((3, 4), 77)
    for linear in (False, True):
        assert (REF.upsample(const, 7, 5, linear) == 77).all() and REF.upsample(const, 8, 6, linear).shape == (6, 8)
    c = np.array([[0, 255], [255, 0]])
    assert REF.upsample(c, 4, 4, False).tolist() == [[0, 0, 255, 255], [0, 0, 255, 255], [255, 255, 0, 0], [255, 255, 0, 0]]
    # rows: y = 0 -> 3 c[0] + c[0] (jn clamps to 0); y = 1 -> 3 c[0] + c[1]; y = 2 -> 3 c[1] + c[0]; y = 3 -> 3 c[1] + c[1] (clamps to ch - 1)
    v = [[0, 1020], [255, 765], [765, 255], [1020, 0]]
    want = [[(a + 2) >> 2, (a + b + 4) >> 3, (b + 2) >> 2, (b + b + 4) >> 3] for a, b in v]
    assert want == [[0, 128, 255, 255], [64, 128, 191, 191], [191, 128, 64, 64], [255, 128, 0, 0]]
    assert REF.upsample(c, 4, 4, True).tolist() == want
    # odd extents: the last pair serves one column and one row, and the neighbours clamp
    odd = REF.upsample(c, 3, 3, True)
    assert odd.tolist() == [row[:3] for row in want[:3]]
    assert REF.upsample(np.array([[9]]), 1, 1, True).tolist() == [[9]] and REF.upsample(np.array([[9]]), 2, 2, True).tolist() == [[9, 9], [9, 9]]


def test_bgra_rules():
    t = np.array([[[10, 20, 30, 128], [200, 100, 50, 0]]], np.uint8)  # B, G, R, A
    assert REF.convert(t, None, REF.BGRA8).tolist() == [[[30, 20, 10, 128], [50, 100, 200, 0]]]
    assert REF.convert(t, None, REF.BGRA8, flags=REF.IGNORE_ALPHA).tolist() == [[[30, 20, 10, 255], [50, 100, 200, 255]]]
    assert REF.convert(t, None, REF.BGRA8, flags=REF.STRAIGHT_ALPHA).tolist() == [[[30 * 128 // 255, 20 * 128 // 255, 10 * 128 // 255, 128], [0, 0, 0, 0]]]


# ------------------------------------------------------------------------------------------------------------------ 2. the calls
def packed_area(ctx):
    area = C.c_int64()
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(area)) == 0
    return area.value


def frame(**kw):
    """16 x 9 NV12 at made-up addresses (a record-only context reads nothing)"""
    base = dict(y=0x10000, uv=0x20000, width=16, height=9, pitch_y=16, pitch_uv=16, format=REF.NV12, matrix=REF.BT709, range=REF.LIMITED, flags=0, reserved=(0, 0))
    base.update(kw)
    f = context.video_frame(base["y"], base["uv"], base["width"], base["height"], base["pitch_y"], base["pitch_uv"], base["format"], base["matrix"], base["range"], base["flags"])
    f.reserved[0], f.reserved[1] = base["reserved"]
    return f


def p010(**kw):
    base = dict(format=REF.P010, pitch_y=32, pitch_uv=32)
    base.update(kw)
    return frame(**base)


def bgra(**kw):
    base = dict(format=REF.BGRA8, uv=0, pitch_y=64, pitch_uv=0, matrix=0, range=0)
    base.update(kw)
    return frame(**base)


ELEMENT0 = "planes[0] and pitch_bytes[0] must be multiples of the element size"
ELEMENT1 = "planes[1] and pitch_bytes[1] must be multiples of a pair's size"
REFUSED = [  # (the struct, or None; the text behind the call's name)
    (None, "null frame"),
    (frame(y=0), "null frame"),
    (bgra(y=0), "null frame"),
    (frame(uv=0), "null chroma plane"),
    (p010(uv=0), "null chroma plane"),
    (frame(width=0), "empty frame"),
    (frame(height=-2), "empty frame"),
    (frame(format=3), "unknown format"),
    (frame(matrix=3), "unknown matrix"),
    (frame(range=2), "unknown range"),
    (frame(flags=8), "unknown flag"),
    (frame(flags=1 | 1 << 31), "unknown flag"),
    (frame(reserved=(7, 0)), "reserved must be 0"),
    (frame(reserved=(0, 1)), "reserved must be 0"),
    (bgra(matrix=1), "matrix and range must be 0 for BGRA8"),
    (bgra(range=1), "matrix and range must be 0 for BGRA8"),
    (bgra(uv=0x20000), "BGRA8 has one plane"),
    (bgra(pitch_uv=16), "BGRA8 has one plane"),
    (bgra(flags=REF.CHROMA_LINEAR), "FDH_VIDEO_CHROMA_LINEAR needs a chroma plane"),
    (bgra(flags=REF.STRAIGHT_ALPHA | REF.IGNORE_ALPHA), "FDH_VIDEO_STRAIGHT_ALPHA and FDH_VIDEO_IGNORE_ALPHA exclude each other"),
    (frame(flags=REF.STRAIGHT_ALPHA), "the alpha flags are BGRA8's"),
    (p010(flags=REF.IGNORE_ALPHA | REF.CHROMA_LINEAR), "the alpha flags are BGRA8's"),
    (bgra(y=0x10002), ELEMENT0),
    (bgra(pitch_y=66), ELEMENT0),
    (p010(y=0x10001), ELEMENT0),
    (p010(pitch_y=33), ELEMENT0),
    (frame(uv=0x20001), ELEMENT1),
    (frame(pitch_uv=17), ELEMENT1),
    (p010(uv=0x20002), ELEMENT1),
    (p010(pitch_uv=34), ELEMENT1),
    (frame(pitch_y=15), "pitch_bytes[0] is below a row's bytes"),
    (frame(pitch_y=-16), "pitch_bytes[0] is below a row's bytes"),
    (p010(pitch_y=30), "pitch_bytes[0] is below a row's bytes"),
    (bgra(pitch_y=60), "pitch_bytes[0] is below a row's bytes"),
    (frame(pitch_uv=14), "pitch_bytes[1] is below a row's bytes"),
    (frame(width=15, pitch_uv=14), "pitch_bytes[1] is below a row's bytes"),  # ceil(15 / 2) = 8 pairs
    (p010(pitch_uv=28), "pitch_bytes[1] is below a row's bytes"),
    (frame(pitch_uv=0), "pitch_bytes[1] is below a row's bytes"),
]


def test_refusals_leave_directory_packer_and_epoch_untouched():
    ctx = HipContext(atlas_size=256, record_only=True)
    L = ctx.L
    assert ctx.put_video_frame(7, 0x10000, 0x20000, 16, 9, 16, 16)[2:] == (16, 9)
    out = (C.c_int * 4)()
    before = (ctx.atlas_usage(), packed_area(ctx))
    for i, (f, text) in enumerate(REFUSED):
        ref = C.byref(f) if f is not None else None
        for name, call in (("put_video_frame", lambda: L.fdh_put_video_frame(ctx.h, 9, ref, out)), ("update_video_frame", lambda: L.fdh_update_video_frame(ctx.h, 7, ref))):
            assert call() == INVALID, (i, name)
            assert L.fdh_last_error().decode() == f"{name}: {text}", (i, name)
            assert (ctx.atlas_usage(), packed_area(ctx)) == before and not ctx.has_image(9), (i, name)
    assert L.fdh_update_video_frame(ctx.h, 9, C.byref(frame())) == INVALID and L.fdh_last_error().decode() == "update_video_frame: unknown key"
    for f in (frame(width=15), frame(height=10), bgra(width=8, pitch_y=32)):
        assert L.fdh_update_video_frame(ctx.h, 7, C.byref(f)) == INVALID and L.fdh_last_error().decode() == "update_video_frame: size mismatch"
    assert (ctx.atlas_usage(), packed_area(ctx)) == before
    # fdh_put_image_device keeps to its own formats and flags
    img = context.DeviceImage(0x10000, 16, 9, 64, 0, 3, 4, 0, 0)
    assert L.fdh_put_image_device(ctx.h, 9, C.byref(img), out) == INVALID
    # a call that goes through moves the epoch, and a put the packer too; odd sizes take ceil(w / 2) pairs
    ctx.update_video_frame(7, 0x10000, 0, 16, 9, 64, 0, format=REF.BGRA8, matrix=0, range=0, flags=REF.STRAIGHT_ALPHA)
    after = ctx.atlas_usage()
    assert after["epoch"] == before[0]["epoch"] + 1 and packed_area(ctx) == before[1]
    assert ctx.put_video_frame(9, 0x10002, 0x20004, 15, 9, 30, 32, format=REF.P010, matrix=REF.BT2020, range=REF.FULL, flags=REF.CHROMA_LINEAR)[2:] == (15, 9)
    assert ctx.has_image(9) and packed_area(ctx) > before[1] and ctx.atlas_usage()["epoch"] == after["epoch"] + 1
    ctx.close()


def test_rectangles_pack_like_plain_images():
    """on a record-only context: every put against fdh_put_image of an image of that size on a second context -- the same rectangles, an
    existing key, growth that drops every entry, keep mode -- and a size no atlas takes"""
    for keep in (False, True):
        a, b = HipContext(atlas_size=64, record_only=True), HipContext(atlas_size=64, record_only=True)
        a.set_atlas_keep(keep), b.set_atlas_keep(keep)
        sizes = [(7, 5), (1, 1), (1, 9), (20, 11), (7, 5), (30, 30), (40, 3), (9, 9), (50, 50), (100, 20)]  # the atlas grows on the way
        for key, (w, h) in enumerate(sizes, start=1):
            if key == 5:
                key = 1  # an existing key
            got = a.put_video_frame(key, 0x20000, 0x40000, w, h, w + 3, 2 * ((w + 1) // 2) + 2)
            assert got == b.put_image(key, np.zeros((h, w, 4), np.uint8)) and got[2:] == (w, h)
            assert (a.atlas_usage(), packed_area(a)) == (b.atlas_usage(), packed_area(b))
            assert [a.has_image(k) for k in range(1, 12)] == [b.has_image(k) for k in range(1, 12)]
        assert a.atlas_size() > 64
        codes = []
        for ctx, call in ((a, lambda: a.put_video_frame(30, 0x20000, 0x40000, 16400, 2, 16400, 16400)), (b, lambda: b.put_image(30, np.zeros((2, 16400, 4), np.uint8)))):
            with pytest.raises(FigdrawHipError) as e:
                call()
            codes.append((e.value.code, ctx.atlas_usage(), packed_area(ctx)))
        assert codes[0] == codes[1] and codes[0][0] == -4
        a.close(), b.close()


def test_update_of_a_flippy_entry_on_a_record_only_context():
    a, b = HipContext(atlas_size=512, record_only=True), HipContext(atlas_size=512, record_only=True)
    data = open(os.path.join(GOLDEN, "img1.flippy"), "rb").read()
    r = a.put_flippy(3, data)
    assert r == b.put_flippy(3, data)
    a.update_video_frame(3, 0x10000, 0x80000, r[2], r[3], r[2], 2 * ((r[2] + 1) // 2))
    b.update_image(3, np.zeros((r[3], r[2], 4), np.uint8))
    assert a.atlas_usage() == b.atlas_usage()
    assert a.compact_atlas()["rects_moved"] == b.compact_atlas()["rects_moved"]  # both are chain entries now
    a.close(), b.close()


def test_struct_layout():
    assert C.sizeof(VideoFrame) == 64 and VideoFrame.width.offset == 32 and VideoFrame.format.offset == 40 and VideoFrame.reserved.offset == 56


def test_video_frame_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "video_frame_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_glyphs"),
                           os.path.join(ROOT, "tests", "video_frame_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "video_frame_abi_smoke: OK" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ 3. the kernel's source
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_video_import.hip (and k_image_import.hip, for the tail) compiled as plain C++ under the sequential shim of tests/emu with the driver
    of tests/video_frame_emu -> the directory of ./emu and ./emu_san: the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "video_frame_emu", ("k_video_import.hip", "fdh_video_import.h", "k_image_import.hip", "fdh_image_import.h"),
                           {"emu": (), "emu_san": emu_build.SAN}, opt="-O2")


def place_of(i, w, h):
    """an entry's place for case i: odd coordinates of every residue, and an atlas that just takes it"""
    x, y = 4 + (i * 7) % 13, 4 + (i * 5) % 11
    size = 16
    while size < max(x + w, y + h) + 4:
        size *= 2
    return x, y, size, min(size.bit_length(), 14)  # levels size, size / 2, .. 1


def through_the_shim(tmp, cases, exe="./emu"):
    """-> per case ([the stored levels], the ink block as 64 ints, the level-5 image), what the program printed"""
    places = []
    with open(os.path.join(tmp, "cases.bin"), "wb") as f:
        for i, case in enumerate(cases):
            w, h = VC.size_of(case)
            (ybuf, yalign, ypitch), c = VC.pack(case)
            cbuf, calign, cpitch = c if c else (b"", 0, 0)
            x, y, size, n_levels = place_of(i, w, h)
            places.append((x, y, size, n_levels))
            f.write(np.array([w, h, case[1], case[2], case[3], case[4], ypitch, cpitch, yalign, calign, len(ybuf), len(cbuf), x, y, size, n_levels], np.int32).tobytes())
            f.write(ybuf)
            f.write(cbuf)
    r = subprocess.run([exe, "cases.bin", "out.bin"], cwd=tmp, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (exe, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    raw = np.fromfile(os.path.join(tmp, "out.bin"), np.uint8)
    out, at = [], 0
    for case, (x, y, size, n_levels) in zip(cases, places):
        w, h = VC.size_of(case)
        w5, h5 = (w + 31) // 32, (h + 31) // 32
        levels = []
        while w > 1 and h > 1 and len(levels) < n_levels:
            levels.append(raw[at:at + w * h * 4].reshape(h, w, 4))
            at += w * h * 4
            w, h = (w + 1) // 2, (h + 1) // 2
        block = raw[at:at + 256].view(np.int32)
        at += 256
        out.append((levels, block, raw[at:at + w5 * h5 * 4].reshape(h5, w5, 4)))
        at += w5 * h5 * 4
    assert at == len(raw)
    return out, r.stdout


def check(case, got):
    levels, block, level5 = got
    texels = VC.texels(case)
    want = REF.chain(texels)
    assert len(levels) == len(want), case[0]
    for l, (a, b) in enumerate(zip(levels, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{case[0]}: level {l} differs in {int((a != b).any(axis=2).sum())} texels"
    img = texels
    for _ in range(5):  # the level-5 image is made whether or not the chain reaches it
        img = REF.minify(img)
    assert np.array_equal(level5, img), f"{case[0]}: the level-5 image"
    boxes = REF.ink_boxes(texels)
    if boxes is None:
        assert block.reshape(16, 4).tolist() == [[32767, 32767, 0, 0]] * 16, case[0]  # untouched
    else:
        mine = block.reshape(16, 4).astype(np.int64)
        mine[mine[:, 2] == 0] = 0  # the host's reading: a box whose x1 is still 0 has no texel
        assert np.array_equal(mine, boxes), case[0]


@pytest.fixture(scope="module")
def emulated(shim):
    cases = VC.cases()
    got, said = through_the_shim(shim, cases)
    print(said.strip())
    return cases, got


def test_the_cases_cover_the_ground():
    cases = VC.cases()
    assert 36 <= len(cases) <= 60 and len({c[0] for c in cases}) == len(cases)
    yuv = {(c[1], c[2], c[3], c[4]) for c in cases if c[1] != REF.BGRA8}
    assert len(yuv) == 24  # 2 formats x 3 matrices x 2 ranges x 2 upsamplings
    assert {c[4] for c in cases if c[1] == REF.BGRA8} == {0, REF.STRAIGHT_ALPHA, REF.IGNORE_ALPHA}
    for size in VC.SIZES:
        assert {c[7] for c in cases if VC.size_of(c) == size} >= {"tight", "padded"}, size


def test_the_kernel_source_against_the_reference(emulated):
    """every level of every case, the level-5 image and the ink block, byte for byte; the program itself refuses a texel written outside the
    rectangles"""
    cases, got = emulated
    for case, g in zip(cases, got):
        check(case, g)


def test_nothing_is_stored_of_a_line(emulated):
    cases, got = emulated
    for c, g in zip(cases, got):
        if VC.size_of(c) in ((1, 1), (1, 9)):
            assert g[0] == []  # (its ink boxes are measured all the same: check() has compared them)
        if VC.size_of(c) == VC.LARGEST:
            assert len(g[0]) == 9


def test_the_shim_under_sanitizers(shim, emulated):
    """the stand-alone program built with -fsanitize=address,undefined on every case but the largest: a read past either end of a plane
    that ends with its last element, a store outside a level or the level-5 image, is an error there"""
    cases, _ = emulated
    pick = [i for i, c in enumerate(cases) if VC.size_of(c) != VC.LARGEST]
    assert len(pick) == len(cases) - 2  # (the largest size in its two layouts)
    got, _ = through_the_shim(shim, [cases[i] for i in pick], exe="./emu_san")
    for i, g in zip(pick, got):
        check(cases[i], g)
