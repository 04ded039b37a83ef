"""The rendered frame out as NV12, P010 or BGRA8 (fdh_read_video_frame, fdh_check_video_target, fdh_video_out_coefficients;
include_video/figdraw_hip_video_out.h), what a CPU can check: the coefficients against their derivation from the standards' constants; known
answers of the reference tests/video_out_ref.py; the integer rule against float64 within the bound the header derives; the target's rules
without a device and through C99; the source of k_video_export.hip under the host shim of tests/emu (tests/video_out_emu) against the reference, byte
for byte, padding included; and what a round trip through fdh_put_video_frame's reference loses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_build
import video_frame_ref as IN
import video_out_cases as VC
import video_out_ref as REF
from conftest import ROOT
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext, VideoTarget

INVALID = -1
ROWS = [(fmt, m, r) for fmt in (REF.NV12, REF.P010) for r in (REF.LIMITED, REF.FULL) for m in (REF.BT601, REF.BT709, REF.BT2020)]
TABLE = [  # the header's table, in its order: 8 bit limited, 8 bit full, 10 bit limited, 10 bit full; BT601, BT709, BT2020 in each
    (4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170), (2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660),
    (3696, 9541, 834, -2010, -5186, 7196, 7196, -6617, -579),
    (4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332), (3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751),
    (4304, 11108, 972, -2288, -5904, 8192, 8192, -7533, -659),
    (16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681), (11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639),
    (14786, 38160, 3338, -8038, -20746, 28784, 28784, -26469, -2315),
    (19653, 38583, 7493, -11091, -21773, 32864, 32864, -27519, -5345), (13974, 47009, 4746, -7531, -25333, 32864, 32864, -29851, -3013),
    (17267, 44564, 3898, -9178, -23686, 32864, 32864, -30221, -2643),
]
LUMA_BOUND, CHROMA_BOUND = 0.039, 0.032  # the header: 2.5 * 255 / 16384 and 2 * 255 / 16384


# ------------------------------------------------------------------------------------------------------------------ 1. the rule
def test_coefficients_are_the_derivation_and_the_table():
    assert len(ROWS) == len(TABLE) == 12
    header = open(os.path.join(ROOT, "include_video", "figdraw_hip_video_out.h")).read()
    largest = 0
    for (fmt, m, r), row in zip(ROWS, TABLE):
        got = context.video_out_coefficients(fmt, m, r)
        assert got == REF.coefficients(fmt, m, r), (fmt, m, r)
        yoff, yden, _, coff = REF.ranges(fmt, r)
        assert got[:2] == (yoff, coff) and got[2:] == row, (fmt, m, r)
        assert sum(got[5:8]) == 0 and sum(got[8:11]) == 0, (fmt, m, r)
        assert sum(got[2:5]) == REF.round_half_even(REF.Fraction(yden * 16384, 255)), (fmt, m, r)
        assert all(str(v) in header for v in row), (fmt, m, r)  # the header prints the row
        top = 255 * 8  # the largest operand: a sum of N = 8 bytes
        largest = max(largest, max(sum(abs(k) for k in got[5:8]), sum(abs(k) for k in got[8:11])) * top, sum(got[2:5]) * 255)
    assert largest == 134_085_120  # the header's figure
    assert largest + (8 << 13) + (512 << 17) < 2 ** 31  # ... with the rounding term and, as the kernel adds it, Coff in front of the shift
    L = context.load()
    out = (C.c_int32 * 11)()
    for bad in ((REF.BGRA8, 0, 0), (3, 0, 0), (REF.NV12, 3, 0), (REF.NV12, 0, 2)):
        assert L.fdh_video_out_coefficients(*bad, out) == INVALID and L.fdh_last_error().decode().startswith("video_out_coefficients: ")
    assert L.fdh_video_out_coefficients(REF.NV12, 0, 0, None) == INVALID


def flat(rgb, w=4, h=4):
    img = np.zeros((h, w, 4), np.uint8)
    img[..., :3] = rgb
    img[..., 3] = 77  # (ignored)
    return img


def test_known_answers_for_every_row():
    for fmt, m, r in ROWS:
        yoff, yden, _, coff = REF.ranges(fmt, r)
        shift = 0 if fmt == REF.NV12 else 6
        for linear in (0, REF.CHROMA_LINEAR):
            y, c = REF.export(flat((0, 0, 0)), fmt, m, r, linear)
            assert (y == yoff << shift).all() and (c == coff << shift).all(), (fmt, m, r)
            y, c = REF.export(flat((255, 255, 255)), fmt, m, r, linear)
            assert (y == (yoff + yden) << shift).all() and (c == coff << shift).all(), (fmt, m, r)
            for grey in range(256):  # every grey, and a frame of all of them: chroma is Coff under both rules
                assert (REF.export(flat((grey,) * 3, 3, 3), fmt, m, r, linear)[1] == coff << shift).all(), (fmt, m, r, grey)
            ramp = np.zeros((16, 16, 4), np.uint8)
            ramp[..., :3] = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
            y, c = REF.export(ramp, fmt, m, r, linear)
            assert (c == coff << shift).all() and (np.diff(y.astype(int).ravel()) >= 0).all()
            if fmt == REF.P010:
                noise = np.random.default_rng(3).integers(0, 256, size=(7, 9, 4)).astype(np.uint8)
                y, c = REF.export(noise, fmt, m, r, linear)
                assert y.dtype == c.dtype == np.uint16 and not (y & 63).any() and not (c & 63).any()
    for m in (REF.BT601, REF.BT709, REF.BT2020):  # pure blue in 8-bit full range: Cb reaches 256 in front of the clamp
        k = REF.coefficients(REF.NV12, m, REF.FULL)
        assert k[1] + ((k[7] * 4 * 255 + (4 << 13)) >> 16) == 256
        y, c = REF.export(flat((0, 0, 255)), REF.NV12, m, REF.FULL)
        assert (c[..., 0] == 255).all()
        y, c = REF.export(flat((255, 0, 0)), REF.NV12, m, REF.FULL)
        assert (c[..., 1] == 255).all()
    # one value by hand: a 2 x 2 block of two blue and two black texels, BT601 full range: the average blue is 127.5,
    # Cb = 128 + ((8192 * 510 + 32768) >> 16) = 192 (exactly 191.75), Cr = 128 + ((-1332 * 510 + 32768) >> 16) = 128 - 10 = 118 (117.63)
    img = np.zeros((2, 2, 4), np.uint8)
    img[0, 1, 2] = img[1, 0, 2] = 255
    assert REF.export(img, REF.NV12, REF.BT601, REF.FULL)[1].tolist() == [[[192, 118]]]


def test_bgra_rules():
    t = np.array([[[10, 20, 30, 128], [200, 100, 50, 0]]], np.uint8)  # R, G, B, A
    assert REF.export(t, REF.BGRA8)[0].tolist() == [[[30, 20, 10, 128], [50, 100, 200, 0]]] and REF.export(t, REF.BGRA8)[1] is None
    assert REF.export(t, REF.BGRA8, flags=REF.IGNORE_ALPHA)[0].tolist() == [[[30, 20, 10, 255], [50, 100, 200, 255]]]
    assert np.array_equal(IN.convert(REF.export(t, REF.BGRA8)[0], None, IN.BGRA8), t)  # the way in inverts it


def _luma_against_float(fmt, m, r, rgb):
    got = REF.luma(rgb, fmt, m, r)
    exact = REF.luma_float(rgb, fmt, m, r)
    d = np.abs(got - np.rint(exact).astype(np.int64))
    from_half = np.abs(exact - np.floor(exact) - 0.5)
    assert d.max() <= 1, (fmt, m, r, int(d.max()))
    assert not d[from_half > LUMA_BOUND].any(), (fmt, m, r)
    return int((d > 0).sum()), float(from_half[d > 0].max(initial=0.0))


def test_luma_against_float64_on_every_triple():
    """all 2^24 triples for 8-bit BT709 limited and 10-bit BT601 full, in slabs of 16 red values"""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for fmt, m, r in ((REF.NV12, REF.BT709, REF.LIMITED), (REF.P010, REF.BT601, REF.FULL)):
        differ, far = 0, 0.0
        for r0 in range(0, 256, 16):
            rgb = np.stack(np.broadcast_arrays(np.arange(r0, r0 + 16)[:, None, None], g[None], b[None]), axis=-1)
            n, f = _luma_against_float(fmt, m, r, rgb)
            differ, far = differ + n, max(far, f)
        print(f"format {fmt} matrix {m} range {r}: {differ} of {1 << 24} luma samples differ by 1, each within {far:.4f} of a tie")


def test_luma_and_chroma_against_float64_on_samples():
    rng = np.random.default_rng(5)
    corners = np.array([[(i & 1) * 255, (i >> 1 & 1) * 255, (i >> 2 & 1) * 255] for i in range(8)])
    for fmt, m, r in ROWS:
        _luma_against_float(fmt, m, r, rng.integers(0, 256, size=(400_000, 3)))
        top = (1 << REF.bits_of(fmt)) - 1
        for n in (1, 4, 8):
            s = np.concatenate([rng.integers(0, 255 * n + 1, size=(200_000, 3)), corners * n])
            got = np.stack(REF.chroma_of_sums(s, n, fmt, m, r), axis=-1)
            exact = np.stack(REF.chroma_float(s, n, fmt, m, r), axis=-1)
            d = np.abs(got - np.clip(np.rint(exact), 0, top).astype(np.int64))
            from_half = np.abs(exact - np.floor(exact) - 0.5)
            assert d.max() <= 1, (fmt, m, r, n, int(d.max()))
            assert not d[from_half > CHROMA_BOUND].any(), (fmt, m, r, n)


def sums_of(values, linear):
    """the chroma sums of a one-channel image"""
    img = np.repeat(np.array(values)[..., None], 3, axis=2)
    s, n = REF.chroma_sums(img, linear)
    assert n == (8 if linear else 4) and (s[..., 0] == s[..., 1]).all() and (s[..., 0] == s[..., 2]).all()
    return s[..., 0].tolist()


def test_downsampling_known_answers():
    a = 9
    # 1 x 1: every column and row clamps to the texel: four times it; p(xl) + 2 p(xc) + p(xr) twice: eight times it
    assert sums_of([[a]], False) == [[4 * a]] and sums_of([[a]], True) == [[8 * a]]
    # 2 x 2 checker.  centre: the four texels.  linear: xl = max(-1, 0) = 0, xc = 0, xr = 1: row 0: 0 + 0 + 255, row 1: 255 + 510 + 0
    c2 = [[0, 255], [255, 0]]
    assert sums_of(c2, False) == [[510]] and sums_of(c2, True) == [[255 + 765]]
    # 3 x 3 checker: pair column 1 has xa = 2, xb = min(3, 2) = 2; pair row 1 has ya = 2, yb = min(3, 2) = 2
    c3 = [[0, 255, 0], [255, 0, 255], [0, 255, 0]]
    #   (0, 0): 0 + 255 + 255 + 0; (1, 0): column 2 twice: 0 + 0 + 255 + 255; (0, 1): row 2 twice: 0 + 255 + 0 + 255; (1, 1): texel (2, 2) four times
    assert sums_of(c3, False) == [[510, 510], [510, 0]]
    #   linear, pair column 0: xl = 0, xc = 0, xr = 1; pair column 1: xl = 1, xc = 2, xr = min(3, 2) = 2
    #   (0, 0): row 0: 0 + 0 + 255, row 1: 255 + 510 + 0; (1, 0): row 0: 255 + 0 + 0, row 1: 0 + 510 + 255
    #   (0, 1): row 2 twice: 2 (0 + 0 + 255); (1, 1): row 2 twice: 2 (255 + 0 + 0)
    assert sums_of(c3, True) == [[1020, 1020], [510, 510]]
    # 4 x 4 checker: no clamp but xl of pair column 0.  centre: every block holds two of each.  linear: pair column 0 as in the 2 x 2 case;
    # pair column 1: xl = 1, xc = 2, xr = 3: row 0: 255 + 0 + 255, row 1: 0 + 510 + 0
    c4 = [[255 * ((x + y) & 1) for x in range(4)] for y in range(4)]
    assert sums_of(c4, False) == [[510, 510], [510, 510]] and sums_of(c4, True) == [[1020, 1020], [1020, 1020]]
    # 4 x 4 ramp p = x + 10 y, which tells the columns apart.  centre: (2 i + 2 i + 1) twice + 10 (2 j + 2 j + 1) twice = 8 i + 80 j + 22
    # linear: columns (0, 0, 1) weigh 0 + 0 + 1 = 1 for pair column 0 and (1, 2, 3) weigh 1 + 4 + 3 = 8 for 1, per row; the rows weigh 4 each:
    # 2 (1 or 8) + 40 (2 j) + 40 (2 j + 1)
    ramp = [[x + 10 * y for x in range(4)] for y in range(4)]
    assert sums_of(ramp, False) == [[22, 30], [102, 110]] and sums_of(ramp, True) == [[42, 56], [202, 216]]


# ------------------------------------------------------------------------------------------------------------------ 2. the target's rules
def target(**kw):
    """a valid NV12 target for the whole of a 16 x 9 frame at made-up addresses (nothing is read or written without a device)"""
    base = dict(y=0x10000, uv=0x20000, pitch_y=16, pitch_uv=16, format=REF.NV12, matrix=REF.BT709, range=REF.LIMITED, flags=0, rect=None, reserved=(0, 0))
    base.update(kw)
    t = context.video_target(base["y"], base["uv"], base["pitch_y"], base["pitch_uv"], base["format"], base["matrix"], base["range"], base["flags"], base["rect"])
    t.reserved[0], t.reserved[1] = base["reserved"]
    return t


def p010(**kw):
    base = dict(format=REF.P010, pitch_y=32, pitch_uv=32)
    base.update(kw)
    return target(**base)


def bgra(**kw):
    base = dict(format=REF.BGRA8, uv=0, pitch_y=64, pitch_uv=0, matrix=0, range=0)
    base.update(kw)
    return target(**base)


FW, FH = 16, 9
ELEMENT0 = "planes[0] and pitch_bytes[0] must be multiples of the element size"
ELEMENT1 = "planes[1] and pitch_bytes[1] must be multiples of a pair's size"
OUTSIDE = "rectangle outside the frame"
EVEN = "the rectangle's x and y must be even for NV12 / P010"
REFUSED = [  # (the struct, or None; the text behind the call's name): each one step from a valid target
    (None, "null target"),
    (target(y=0), "null target"),
    (bgra(y=0), "null target"),
    (target(uv=0), "null chroma plane"),
    (p010(uv=0), "null chroma plane"),
    (target(format=3), "unknown format"),
    (target(matrix=3), "unknown matrix"),
    (target(range=2), "unknown range"),
    (target(flags=8), "unknown flag"),
    (target(flags=1 | 1 << 31), "unknown flag"),
    (target(reserved=(7, 0)), "reserved must be 0"),
    (target(reserved=(0, 1)), "reserved must be 0"),
    (bgra(matrix=1), "matrix and range must be 0 for BGRA8"),
    (bgra(range=1), "matrix and range must be 0 for BGRA8"),
    (bgra(uv=0x20000), "BGRA8 has one plane"),
    (bgra(pitch_uv=16), "BGRA8 has one plane"),
    (bgra(flags=REF.CHROMA_LINEAR), "FDH_VIDEO_CHROMA_LINEAR needs a chroma plane"),
    (target(flags=REF.IGNORE_ALPHA), "FDH_VIDEO_IGNORE_ALPHA is BGRA8's"),
    (p010(flags=REF.IGNORE_ALPHA | REF.CHROMA_LINEAR), "FDH_VIDEO_IGNORE_ALPHA is BGRA8's"),
    (target(flags=REF.STRAIGHT_ALPHA), "FDH_VIDEO_STRAIGHT_ALPHA is for the way in: the surface's bytes go out as stored"),
    (p010(flags=REF.STRAIGHT_ALPHA), "FDH_VIDEO_STRAIGHT_ALPHA is for the way in: the surface's bytes go out as stored"),
    (bgra(flags=REF.STRAIGHT_ALPHA), "FDH_VIDEO_STRAIGHT_ALPHA is for the way in: the surface's bytes go out as stored"),
    (target(rect=(2, 0, 15, 9)), OUTSIDE),
    (target(rect=(0, 2, 16, 8)), OUTSIDE),
    (target(rect=(-2, 0, 4, 4)), OUTSIDE),
    (target(rect=(0, -2, 4, 4)), OUTSIDE),
    (target(rect=(16, 0, 1, 1)), OUTSIDE),
    (bgra(rect=(1, 1, 16, 8)), OUTSIDE),
    (target(rect=(2, 2, 2 ** 31 - 1, 2)), OUTSIDE),
    (target(rect=(1, 0, 4, 4)), EVEN),
    (target(rect=(0, 3, 4, 4)), EVEN),
    (p010(rect=(5, 5, 2, 2)), EVEN),
    (bgra(y=0x10002), ELEMENT0),
    (bgra(pitch_y=66), ELEMENT0),
    (p010(y=0x10001), ELEMENT0),
    (p010(pitch_y=33), ELEMENT0),
    (target(uv=0x20001), ELEMENT1),
    (target(pitch_uv=17), ELEMENT1),
    (p010(uv=0x20002), ELEMENT1),
    (p010(pitch_uv=34), ELEMENT1),
    (target(pitch_y=15), "pitch_bytes[0] is below a row's bytes"),
    (target(pitch_y=-16), "pitch_bytes[0] is below a row's bytes"),
    (p010(pitch_y=30), "pitch_bytes[0] is below a row's bytes"),
    (bgra(pitch_y=60), "pitch_bytes[0] is below a row's bytes"),
    (target(pitch_uv=14), "pitch_bytes[1] is below a row's bytes"),
    (target(rect=(0, 0, 15, 9), pitch_uv=14), "pitch_bytes[1] is below a row's bytes"),  # ceil(15 / 2) = 8 pairs
    (p010(pitch_uv=28), "pitch_bytes[1] is below a row's bytes"),
    (target(pitch_uv=0), "pitch_bytes[1] is below a row's bytes"),
    (target(uv=0x10000), "the two planes overlap"),
    (target(uv=0x10000 + 16 * 9 - 2), "the two planes overlap"),      # the chroma plane starts in the luma plane's last two bytes
    (target(y=0x20000 + 16 * 5 - 1), "the two planes overlap"),        # the luma plane starts in the chroma plane's last byte
]
ACCEPTED = [
    target(), p010(), bgra(), bgra(flags=REF.IGNORE_ALPHA), target(flags=REF.CHROMA_LINEAR),
    target(uv=0x10000 + 16 * 9), target(y=0x20000 + 16 * 5),           # the planes touch
    target(rect=(2, 4, 13, 5)), target(rect=(14, 8, 2, 1)), target(rect=(0, 0, 0, 5)), target(rect=(7, 7, -1, 0)),  # (w or h <= 0: the whole frame)
    bgra(rect=(1, 3, 15, 6)), p010(rect=(2, 2, 3, 3), pitch_y=6, pitch_uv=8),
    target(y=0x10001, pitch_y=17), p010(y=0x10002, uv=0x20004, pitch_y=34, pitch_uv=36),
    target(rect=(0, 0, 15, 9), pitch_y=15),
]


def test_check_video_target_applies_every_rule():
    L = context.load()
    for i, t in enumerate(ACCEPTED):
        assert L.fdh_check_video_target(C.byref(t), FW, FH) == 0, (i, L.fdh_last_error().decode())
        context.check_video_target(t, FW, FH)
    for i, (t, text) in enumerate(REFUSED):
        assert L.fdh_check_video_target(C.byref(t) if t is not None else None, FW, FH) == INVALID, (i, text)
        assert L.fdh_last_error().decode() == f"check_video_target: {text}", i
    for fw, fh in ((0, 9), (16, 0), (-1, -1)):
        assert L.fdh_check_video_target(C.byref(target()), fw, fh) == INVALID and L.fdh_last_error().decode() == "check_video_target: empty frame"
    with pytest.raises(FigdrawHipError) as e:
        context.check_video_target(target(format=3), FW, FH)
    assert e.value.code == INVALID and str(e.value).endswith("check_video_target: unknown format")


def test_a_record_only_context_refuses():
    ctx = HipContext(atlas_size=256, record_only=True)
    ctx.begin_frame(FW, FH, True, (0, 0, 0, 1))
    ctx.end_frame()
    assert ctx.L.fdh_read_video_frame(ctx.h, C.byref(target())) == INVALID
    assert ctx.L.fdh_last_error().decode().startswith("read_video_frame: ")
    with pytest.raises(FigdrawHipError):
        ctx.read_video_frame(0x10000, 0x20000, 16, 16)
    assert ctx.L.fdh_read_video_frame(None, C.byref(target())) == INVALID
    ctx.close()


def test_struct_layout():
    assert C.sizeof(VideoTarget) == 72 and VideoTarget.rect.offset == 32 and VideoTarget.format.offset == 48 and VideoTarget.reserved.offset == 64


def test_video_out_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "video_out_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_video"),
                           os.path.join(ROOT, "tests", "video_out_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "video_out_abi_smoke: OK" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ 3. the kernel's source
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_video_export.hip compiled as plain C++ under the sequential shim of tests/emu with the driver of tests/video_out_emu -> the
    directory of ./emu and ./emu_san: the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "video_out_emu", ("k_video_export.hip", "fdh_video_export.h"), {"emu": (), "emu_san": emu_build.SAN}, opt="-O2")


def through_the_shim(tmp, cases, exe):
    """-> per case the planes' bytes as the program left them, and what it printed"""
    with open(os.path.join(tmp, "cases.bin"), "wb") as f:
        for case in cases:
            _, W, H, _, fmt, m, r, flags, _ = case
            lay = VC.layouts(case)
            (ay, py), (ac, pc) = lay[0][:2], (lay[1][:2] if len(lay) > 1 else (0, 0))
            f.write(np.array([W, H, *VC.rect_of(case), fmt, m, r, flags, py, pc, ay, ac, 0, 0], np.int32).tobytes())
            f.write(VC.source(W, H).tobytes())
    r = subprocess.run([exe, "cases.bin", "out.bin"], cwd=tmp, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (exe, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    raw = np.fromfile(os.path.join(tmp, "out.bin"), np.uint8)
    out, at = [], 0
    for case in cases:
        planes = []
        for _, pitch, rows, row_bytes in VC.layouts(case):
            n = VC.plane_bytes(pitch, rows, row_bytes)
            planes.append(raw[at:at + n])
            at += n
        out.append(planes)
    assert at == len(raw)
    return out, r.stdout


def check(case, got):
    want = VC.expected_planes(case)
    assert len(got) == len(want), case[0]
    for p, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (case[0], p)
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{case[0]}: plane {p} differs in {int((a != b).sum())} bytes, the first at {at} (pitch {VC.layouts(case)[p][1]}): {a[at]} != {b[at]}")


def wide(case, p):
    """the host's decision for plane p of a case: one store per run"""
    align, pitch, _, row_bytes = VC.layouts(case)[p]
    es = VC.element_sizes(case[4])[p]
    run = (4, 2)[p] * es
    return align % run == 0 and pitch % run == 0 and row_bytes // es >= (4, 2)[p]


def test_the_cases_cover_the_ground():
    cases = VC.cases()
    assert len({c[0] for c in cases}) == len(cases)
    want_sizes = {(1, 1), (2, 1), (1, 2), (3, 3), (4, 2), (5, 7), (8, 2)} | {(w, h) for w in (127, 128, 129) for h in (15, 16, 17)}
    for fmt, flags in VC.KINDS:
        mine = [c for c in cases if (c[4], c[7]) == (fmt, flags)]
        assert {(c[1], c[2]) for c in mine if c[3] is None} == want_sizes
        for size in want_sizes:
            assert {c[8] for c in mine if (c[1], c[2]) == size} == set(VC.LAYOUTS)
        assert any(c[3] is not None for c in mine)
        planes = (0, 1) if fmt != REF.BGRA8 else (0,)
        for p in planes:  # both the wide and the element path store every kind of plane, at the tile's sizes too
            assert {wide(c, p) for c in mine if c[1] >= 127} == {True, False}, (fmt, flags, p)
        if fmt != REF.BGRA8:
            assert {(c[5], c[6]) for c in mine} == set(VC.MATRIX_RANGE)
    rects = [c for c in cases if c[3] is not None]
    assert all(c[3][0] % 2 == 0 and c[3][1] % 2 == 0 for c in rects if c[4] != REF.BGRA8)
    assert {c[3][0] % 4 for c in rects} >= {0, 2}  # source runs on and off a 16-byte boundary


@pytest.fixture(scope="module")
def emulated(shim):
    cases = VC.cases()
    got, said = through_the_shim(shim, cases, "./emu")
    print(said.strip())
    return cases, got, said


def test_the_kernel_source_against_the_reference(emulated):
    """every plane of every case byte for byte, from the plane's pointer to its last element's end: what lies between a row's end and the
    pitch is still 0xEE; a rectangle's planes are the export of the cropped frame"""
    cases, got, said = emulated
    for case, g in zip(cases, got):
        check(case, g)
    words = said.split()
    counts = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    assert counts["cases"] == len(cases)
    assert counts["wide_y"] == sum(wide(c, 0) for c in cases) and counts["wide_c"] == sum(wide(c, 1) for c in cases if c[4] != REF.BGRA8)
    assert 0 < counts["wide_src"] < len(cases)  # both ways of loading a run


def test_the_shim_under_sanitizers(shim, emulated):
    """the stand-alone program built with -fsanitize=address,undefined on every case: a read past either end of the source, a store outside
    a plane that ends with its last element, a wide access at an address that is no multiple of its size, is an error there"""
    cases, _, _ = emulated
    got, _ = through_the_shim(shim, cases, "./emu_san")
    for case, g in zip(cases, got):
        check(case, g)


# ------------------------------------------------------------------------------------------------------------------ 4. there and back
def test_round_trip_through_the_way_in():
    """video_frame_ref.convert(video_out_ref.export(img)): what 8- or 10-bit coding of either range loses, per format / matrix / range -- a
    property of the coding (profiles/video_out.txt holds the figures), not a tolerance for the device, which is held to the reference byte
    for byte.  Flat colours lose the quantisation alone; noise loses the chroma of three texels in four."""
    rng = np.random.default_rng(11)
    colours = rng.integers(0, 256, size=(4096, 3)).astype(np.uint8)
    noise = np.full((32, 32, 4), 255, np.uint8)
    noise[..., :3] = rng.integers(0, 256, size=(32, 32, 3))
    for fmt, m, r in ROWS:
        worst = 0
        for linear in (0, REF.CHROMA_LINEAR):
            for rgb in colours[:512]:
                img = flat(rgb, 2, 2)
                img[..., 3] = 255
                back = IN.convert(*REF.export(img, fmt, m, r, linear), fmt, m, r, linear)
                worst = max(worst, int(np.abs(back.astype(int) - img).max()))
        back = IN.convert(*REF.export(noise, fmt, m, r), fmt, m, r)
        on_noise = int(np.abs(back.astype(int) - noise).max())
        print(f"round trip {VC.name_of(fmt)} matrix {m} range {r}: flat colours <= {worst}, noise <= {on_noise}")
    assert np.array_equal(IN.convert(REF.export(noise, REF.BGRA8)[0], None, IN.BGRA8), noise)
