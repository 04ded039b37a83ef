"""Three-plane video in and out (fdh_put_video_planes, fdh_update_video_planes, fdh_read_video_planes, fdh_check_video_planes_target;
include_video/figdraw_hip_video_planar.h), what a CPU can check: the reference tests/video_planar_ref.py against the siblings' references on
interleaved and shifted samples; known answers and the float64 bound for 4:4:4; every refusal without a device and through C99; and the
sources of k_video_planar_import.hip and k_video_planar_export.hip under the host shim of tests/emu (tests/video_planar_in_emu,
tests/video_planar_out_emu) against the reference, byte for byte, padding included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_build
import video_frame_ref as SIB_IN
import video_out_ref as SIB_OUT
import video_planar_cases as VC
import video_planar_ref as REF
from conftest import ROOT
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext, VideoPlanes, VideoPlanesTarget

INVALID = -1
ROWS = [(m, r) for m in (REF.BT601, REF.BT709, REF.BT2020) for r in (REF.LIMITED, REF.FULL)]
CHROMA_BOUND = 2 * 255 / 16384  # the header, N = 1


# ------------------------------------------------------------------------------------------------------------------ 1. the reference
def test_the_420_references_equal_the_siblings_on_interleaved_and_shifted_samples():
    rng = np.random.default_rng(31)
    for w, h in ((1, 1), (2, 2), (3, 3), (5, 7), (8, 6), (33, 31)):
        img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        for m, r in ROWS:
            for flags in (0, REF.CHROMA_LINEAR):
                for fmt, sib, shift in ((REF.I420, SIB_IN.NV12, 0), (REF.I010, SIB_IN.P010, 6)):
                    # the way in: the sibling gets the samples interleaved, 10-bit ones at the top of the word, over garbage of its own
                    planes = VC.noise_planes(rng, fmt, w, h)
                    top = (1 << REF.bits_of(fmt)) - 1
                    low = rng.integers(0, 1 << shift, size=(h, w)).astype(planes[0].dtype)
                    luma = (((planes[0] & top) << shift) | low).astype(planes[0].dtype)
                    chroma = ((np.stack([planes[1], planes[2]], axis=2) & top) << shift).astype(planes[0].dtype)
                    assert np.array_equal(REF.convert(planes, fmt, m, r, flags), SIB_IN.convert(luma, chroma, sib, m, r, flags)), (w, h, fmt, m, r, flags)
                    # the way out: the sibling's chroma plane de-interleaved, its 10-bit words >> 6
                    y, cb, cr = REF.export(img, fmt, m, r, flags)
                    sy, sc = SIB_OUT.export(img, sib, m, r, flags)
                    assert np.array_equal(y, sy >> shift) and np.array_equal(cb, sc[..., 0] >> shift) and np.array_equal(cr, sc[..., 1] >> shift), (w, h, fmt, m, r, flags)
                    assert y.dtype == cb.dtype == cr.dtype == REF.dtype_of(fmt) and int(max(y.max(), cb.max(), cr.max())) <= top
    for fmt, sib in ((REF.I420, SIB_IN.NV12), (REF.I010, SIB_IN.P010), (REF.I444, SIB_IN.NV12), (REF.I410, SIB_IN.P010)):
        for m, r in ROWS:  # an 8-bit planar format uses the NV12 row of either table, a 10-bit one the P010 row
            assert REF.in_coefficients(fmt, m, r) == context.video_coefficients(sib, m, r)
            assert REF.out_coefficients(fmt, m, r) == context.video_out_coefficients(sib, m, r)


def flat(rgb, w=3, h=3):
    img = np.zeros((h, w, 4), np.uint8)
    img[..., :3] = rgb
    img[..., 3] = 77  # (ignored)
    return img


def test_444_known_answers():
    for fmt in (REF.I444, REF.I410):
        for m, r in ROWS:
            yoff, yden, _, coff = REF.ranges(fmt, r)
            y, cb, cr = REF.export(flat((0, 0, 0)), fmt, m, r)
            assert y.shape == cb.shape == cr.shape == (3, 3) and (y == yoff).all() and (cb == coff).all() and (cr == coff).all(), (fmt, m, r)
            y, cb, cr = REF.export(flat((255, 255, 255)), fmt, m, r)
            assert (y == yoff + yden).all() and (cb == coff).all() and (cr == coff).all(), (fmt, m, r)
            greys = np.zeros((16, 16, 4), np.uint8)
            greys[..., :3] = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)  # every grey
            y, cb, cr = REF.export(greys, fmt, m, r)
            assert (cb == coff).all() and (cr == coff).all() and (np.diff(y.astype(int).ravel()) >= 0).all(), (fmt, m, r)
    for m in (REF.BT601, REF.BT709, REF.BT2020):  # pure blue and pure red in 8-bit full range: 256 in front of the clamp
        k = REF.out_coefficients(REF.I444, m, REF.FULL)
        assert k[1] + ((k[7] * 255 + 8192) >> 14) == 256 and k[1] + ((k[8] * 255 + 8192) >> 14) == 256
        assert (REF.export(flat((0, 0, 255)), REF.I444, m, REF.FULL)[1] == 255).all()
        assert (REF.export(flat((255, 0, 0)), REF.I444, m, REF.FULL)[2] == 255).all()
    # one value by hand, BT601 full range, 8 bit, the texel (10, 20, 200): kU = (-2765, -5427, 8192), kV = (8192, -6860, -1332)
    #   Cb = 128 + ((-27650 - 108540 + 1638400 + 8192) >> 14) = 128 + (1510402 >> 14) = 128 + 92 = 220   (exactly 220.19)
    #   Cr = 128 + ((81920 - 137200 - 266400 + 8192) >> 14) = 128 + (-313488 >> 14) = 128 - 20 = 108      (exactly 108.87 -> floor of -19.13)
    #   Y  = (4899 * 10 + 9617 * 20 + 1868 * 200 + 8192) >> 14 = 623122 >> 14 = 38
    y, cb, cr = REF.export(flat((10, 20, 200), 1, 1), REF.I444, REF.BT601, REF.FULL)
    assert (int(y[0, 0]), int(cb[0, 0]), int(cr[0, 0])) == (38, 220, 108)
    # the way in takes c[y][x]: a 2 x 2 frame whose four texels differ in chroma only
    Y = np.full((2, 2), 128, np.uint8)
    cb, cr = np.array([[128, 255], [0, 128]], np.uint8), np.array([[128, 128], [128, 0]], np.uint8)
    got = REF.convert((Y, cb, cr), REF.I444, REF.BT601, REF.FULL)
    assert got[0, 0].tolist() == [128, 128, 128, 255] and got[0, 1, 2] == 255 and got[1, 0, 2] == 0 and got[1, 1, 0] == 0
    assert np.array_equal(got, SIB_IN.yuv_to_rgba(Y, cb, cr, SIB_IN.NV12, REF.BT601, REF.FULL))  # the sibling's per-texel rule
    # 10 bit on the way in: the six high bits are ignored
    Y10 = np.array([[64, 64 | 0xFC00]], np.uint16)
    c10 = np.array([[512, 512 | 0xFC00]], np.uint16)
    assert REF.convert((Y10, c10, c10), REF.I410, REF.BT709, REF.LIMITED).tolist() == [[[0, 0, 0, 255]] * 2]
    assert REF.convert((Y10, c10[:, :1], c10[:, 1:]), REF.I010, REF.BT709, REF.LIMITED).tolist() == [[[0, 0, 0, 255]] * 2]


def test_444_chroma_against_float64_within_the_bound():
    """a dense sample of triples -- every (R, B) pair on a green lattice of 16, the cube's corners, and noise --: never more than 1 from the
    rounded float64 value, and equal to it wherever that lies further from a half than 2 * 255 / 16384"""
    rng = np.random.default_rng(7)
    r, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    lattice = np.concatenate([np.stack([r.ravel(), np.full(r.size, g), b.ravel()], axis=1) for g in list(range(0, 256, 16)) + [255]])
    corners = np.array([[(i & 1) * 255, (i >> 1 & 1) * 255, (i >> 2 & 1) * 255] for i in range(8)])
    rgb = np.concatenate([lattice, corners, rng.integers(0, 256, size=(200_000, 3))])
    assert CHROMA_BOUND < 0.032
    for fmt in (REF.I444, REF.I410):
        top = (1 << REF.bits_of(fmt)) - 1
        for m, rg in ROWS:
            s, n = REF.chroma_sums(rgb, fmt, False)
            assert n == 1
            got = np.stack(REF.chroma_of_sums(s, n, fmt, m, rg), axis=-1)
            exact = np.stack(REF.chroma_float(rgb, fmt, m, rg), axis=-1)
            d = np.abs(got - np.clip(np.rint(exact), 0, top).astype(np.int64))
            from_half = np.abs(exact - np.floor(exact) - 0.5)
            assert d.max() <= 1, (fmt, m, rg, int(d.max()))
            assert not d[from_half > CHROMA_BOUND].any(), (fmt, m, rg)


# ------------------------------------------------------------------------------------------------------------------ 2. the rules
FW, FH = 16, 9
Y0, CB0, CR0 = 0x10000, 0x20000, 0x30000


def target(**kw):
    """a valid I420 target for the whole of a 16 x 9 frame at made-up addresses (nothing is read or written without a device)"""
    base = dict(ptrs=(Y0, CB0, CR0), pitches=(16, 8, 8), format=REF.I420, matrix=REF.BT709, range=REF.LIMITED, flags=0, rect=None, reserved=(0, 0))
    base.update(kw)
    t = context.video_planes_target(base["ptrs"], base["pitches"], base["format"], base["matrix"], base["range"], base["flags"], base["rect"])
    t.reserved[0], t.reserved[1] = base["reserved"]
    return t


def frame(**kw):
    """the same as a source: 16 x 9 I420"""
    base = dict(ptrs=(Y0, CB0, CR0), pitches=(16, 8, 8), width=FW, height=FH, format=REF.I420, matrix=REF.BT709, range=REF.LIMITED, flags=0, reserved=(0, 0))
    base.update(kw)
    f = context.video_planes(base["ptrs"], base["width"], base["height"], base["pitches"], base["format"], base["matrix"], base["range"], base["flags"])
    f.reserved[0], f.reserved[1] = base["reserved"]
    return f


I010 = dict(format=REF.I010, pitches=(32, 16, 16))
I444 = dict(format=REF.I444, pitches=(16, 16, 16))
I410 = dict(format=REF.I410, pitches=(32, 32, 32))


def multiple(p):
    return f"planes[{p}] and pitch_bytes[{p}] must be multiples of the sample size"


def below(p):
    return f"pitch_bytes[{p}] is below a row's bytes"


LINEAR_444 = "FDH_VIDEO_CHROMA_LINEAR is for I420 / I010: a 4:4:4 frame has a chroma sample per texel"
ALPHA = "the alpha flags are BGRA8's"
# (keywords one step from a valid struct, the text behind the call's name): the rules both directions share
SHARED = [
    (dict(ptrs=(0, CB0, CR0)), None), (dict(ptrs=(Y0, 0, CR0)), None), (dict(ptrs=(Y0, CB0, 0)), None),
    (dict(format=0), "unknown format"), (dict(format=1), "unknown format"), (dict(format=2), "unknown format"), (dict(format=7), "unknown format"),
    (dict(matrix=3), "unknown matrix"), (dict(range=2), "unknown range"),
    (dict(flags=8), "unknown flag"), (dict(flags=1 | 1 << 31), "unknown flag"),
    (dict(reserved=(7, 0)), "reserved must be 0"), (dict(reserved=(0, 1)), "reserved must be 0"),
    (dict(flags=REF.STRAIGHT_ALPHA), ALPHA), (dict(flags=REF.IGNORE_ALPHA | REF.CHROMA_LINEAR), ALPHA), (dict(I444, flags=REF.IGNORE_ALPHA), ALPHA),
    (dict(I444, flags=REF.CHROMA_LINEAR), LINEAR_444), (dict(I410, flags=REF.CHROMA_LINEAR), LINEAR_444),
    (dict(I010, ptrs=(Y0 + 1, CB0, CR0)), multiple(0)), (dict(I010, ptrs=(Y0, CB0 + 1, CR0)), multiple(1)), (dict(I410, ptrs=(Y0, CB0, CR0 + 1)), multiple(2)),
    (dict(I010, pitches=(33, 16, 16)), multiple(0)), (dict(I010, pitches=(32, 17, 16)), multiple(1)), (dict(I410, pitches=(32, 32, 33)), multiple(2)),
    (dict(pitches=(15, 8, 8)), below(0)), (dict(pitches=(-16, 8, 8)), below(0)), (dict(pitches=(16, 7, 8)), below(1)), (dict(pitches=(16, 8, 0)), below(2)),
    (dict(I010, pitches=(30, 16, 16)), below(0)), (dict(I010, pitches=(32, 16, 14)), below(2)),
    (dict(I444, pitches=(16, 15, 16)), below(1)), (dict(I410, pitches=(32, 32, 30)), below(2)),
]
OUTSIDE = "rectangle outside the frame"
EVEN = "the rectangle's x and y must be even for I420 / I010"
TARGET_ONLY = [
    (dict(rect=(2, 0, 15, 9)), OUTSIDE), (dict(rect=(0, 2, 16, 8)), OUTSIDE), (dict(rect=(-2, 0, 4, 4)), OUTSIDE), (dict(rect=(0, -2, 4, 4)), OUTSIDE),
    (dict(rect=(16, 0, 1, 1)), OUTSIDE), (dict(I444, rect=(1, 1, 16, 8)), OUTSIDE), (dict(rect=(2, 2, 2 ** 31 - 1, 2)), OUTSIDE),
    (dict(rect=(1, 0, 4, 4)), EVEN), (dict(rect=(0, 3, 4, 4)), EVEN), (dict(I010, rect=(5, 5, 2, 2)), EVEN),
    (dict(rect=(0, 0, 15, 9), pitches=(16, 7, 8)), below(1)),  # ceil(15 / 2) = 8 samples
    (dict(ptrs=(Y0, Y0, CR0)), "planes 0 and 1 overlap"), (dict(ptrs=(Y0, CB0, Y0 + 16 * 9 - 1)), "planes 0 and 2 overlap"),
    (dict(ptrs=(Y0, CB0, CB0 + 8 * 5 - 1)), "planes 1 and 2 overlap"), (dict(ptrs=(CB0 + 8 * 5 - 1, CB0, CR0)), "planes 0 and 1 overlap"),
    (dict(I410, ptrs=(Y0, CB0, CB0 + 32 * 9 - 2)), "planes 1 and 2 overlap"),
]
ACCEPTED = [
    dict(), I010, I444, I410, dict(flags=REF.CHROMA_LINEAR), dict(I010, flags=REF.CHROMA_LINEAR),
    dict(ptrs=(Y0, Y0 + 16 * 9, Y0 + 16 * 9 + 8 * 5)), dict(ptrs=(CB0 + 8 * 5, CB0, CR0)),  # the planes touch
    dict(rect=(2, 4, 13, 5)), dict(rect=(14, 8, 2, 1)), dict(rect=(0, 0, 0, 5)), dict(rect=(7, 7, -1, 0)),  # (w or h <= 0: the whole frame)
    dict(I444, rect=(1, 3, 15, 6)), dict(I410, rect=(3, 5, 7, 3), pitches=(14, 14, 14)), dict(I010, rect=(2, 2, 3, 3), pitches=(6, 4, 4)),
    dict(ptrs=(Y0 + 1, CB0 + 3, CR0 + 5), pitches=(17, 9, 11)), dict(I010, ptrs=(Y0 + 2, CB0 + 6, CR0 + 10), pitches=(34, 18, 22)),
    dict(rect=(0, 0, 15, 9), pitches=(15, 8, 8)),
]


def test_check_video_planes_target_applies_every_rule():
    L = context.load()
    for i, kw in enumerate(ACCEPTED):
        t = target(**kw)
        assert L.fdh_check_video_planes_target(C.byref(t), FW, FH) == 0, (i, L.fdh_last_error().decode())
        context.check_video_planes_target(t, FW, FH)
    for i, (kw, text) in enumerate(SHARED + TARGET_ONLY):
        t = target(**kw)
        assert L.fdh_check_video_planes_target(C.byref(t), FW, FH) == INVALID, (i, kw)
        assert L.fdh_last_error().decode() == f"check_video_planes_target: {text or 'null target or plane'}", (i, kw)
    assert L.fdh_check_video_planes_target(None, FW, FH) == INVALID and L.fdh_last_error().decode() == "check_video_planes_target: null target or plane"
    for fw, fh in ((0, 9), (16, 0), (-1, -1)):
        assert L.fdh_check_video_planes_target(C.byref(target()), fw, fh) == INVALID and L.fdh_last_error().decode() == "check_video_planes_target: empty frame"
    with pytest.raises(FigdrawHipError) as e:
        context.check_video_planes_target(target(format=7), FW, FH)
    assert e.value.code == INVALID and str(e.value).endswith("check_video_planes_target: unknown format")


def packed_area(ctx):
    area = C.c_int64()
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(area)) == 0
    return area.value


def test_refusals_on_the_way_in_leave_directory_packer_and_epoch_untouched():
    ctx = HipContext(atlas_size=256, record_only=True)
    L = ctx.L
    assert ctx.put_video_planes(7, (Y0, CB0, CR0), FW, FH, (16, 8, 8))[2:] == (FW, FH)
    out = (C.c_int * 4)()
    before = (ctx.atlas_usage(), packed_area(ctx))
    refused = [(frame(**kw), text or "null frame or plane") for kw, text in SHARED] + [
        (None, "null frame or plane"), (frame(width=0), "empty frame"), (frame(height=-2), "empty frame"), (frame(width=15, pitches=(15, 7, 8)), below(1))]
    for i, (f, text) in enumerate(refused):
        ref = C.byref(f) if f is not None else None
        for name, call in (("put_video_planes", lambda: L.fdh_put_video_planes(ctx.h, 9, ref, out)), ("update_video_planes", lambda: L.fdh_update_video_planes(ctx.h, 7, ref))):
            assert call() == INVALID, (i, name)
            assert L.fdh_last_error().decode() == f"{name}: {text}", (i, name)
            assert (ctx.atlas_usage(), packed_area(ctx)) == before and not ctx.has_image(9), (i, name)
    assert L.fdh_update_video_planes(ctx.h, 9, C.byref(frame())) == INVALID and L.fdh_last_error().decode() == "update_video_planes: unknown key"
    for f in (frame(width=15), frame(height=10), frame(**dict(I444, width=8))):
        assert L.fdh_update_video_planes(ctx.h, 7, C.byref(f)) == INVALID and L.fdh_last_error().decode() == "update_video_planes: size mismatch"
    assert (ctx.atlas_usage(), packed_area(ctx)) == before
    # the siblings keep refusing every format value above 2, and the planar calls the siblings' formats
    old = context.video_frame(Y0, CB0, FW, FH, 16, 16, REF.I420)
    assert L.fdh_put_video_frame(ctx.h, 9, C.byref(old), out) == INVALID and L.fdh_last_error().decode() == "put_video_frame: unknown format"
    assert L.fdh_check_video_target(C.byref(context.video_target(Y0, CB0, 16, 16, format=REF.I444)), FW, FH) == INVALID
    assert (ctx.atlas_usage(), packed_area(ctx)) == before
    # a call that goes through moves the epoch, and a put the packer too; the planes may alias each other on the way in; YV12 is swapped pointers
    ctx.update_video_planes(7, (Y0, CR0, CB0), FW, FH, (16, 8, 8))
    ctx.update_video_planes(7, (Y0, Y0, Y0), FW, FH, (32, 32, 32), format=REF.I410, matrix=REF.BT2020, range=REF.FULL)
    after = ctx.atlas_usage()
    assert after["epoch"] == before[0]["epoch"] + 2 and packed_area(ctx) == before[1]
    assert ctx.put_video_planes(9, (Y0 + 2, CB0 + 2, CR0 + 2), 15, 9, (30, 16, 18), format=REF.I010, flags=REF.CHROMA_LINEAR)[2:] == (15, 9)
    assert ctx.has_image(9) and packed_area(ctx) > before[1] and ctx.atlas_usage()["epoch"] == after["epoch"] + 1
    # and it places like a plain image of that size
    plain = HipContext(atlas_size=256, record_only=True)
    assert plain.put_image(7, np.zeros((FH, FW, 4), np.uint8)) == ctx.image_rect(7) and plain.put_image(9, np.zeros((9, 15, 4), np.uint8)) == ctx.image_rect(9)
    plain.close()
    ctx.close()


def test_a_record_only_context_refuses_the_read():
    ctx = HipContext(atlas_size=256, record_only=True)
    ctx.begin_frame(FW, FH, True, (0, 0, 0, 1))
    ctx.end_frame()
    assert ctx.L.fdh_read_video_planes(ctx.h, C.byref(target())) == INVALID
    assert ctx.L.fdh_last_error().decode().startswith("read_video_planes: ")
    with pytest.raises(FigdrawHipError):
        ctx.read_video_planes((Y0, CB0, CR0), (16, 8, 8))
    assert ctx.L.fdh_read_video_planes(None, C.byref(target())) == INVALID
    ctx.close()


def test_struct_layout():
    assert C.sizeof(VideoPlanes) == 80 and VideoPlanes.pitch_bytes.offset == 24 and VideoPlanes.width.offset == 48 and VideoPlanes.format.offset == 56 and VideoPlanes.reserved.offset == 72
    assert C.sizeof(VideoPlanesTarget) == 88 and VideoPlanesTarget.rect.offset == 48 and VideoPlanesTarget.format.offset == 64 and VideoPlanesTarget.reserved.offset == 80


def test_video_planar_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "video_planar_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_video"),
                           os.path.join(ROOT, "tests", "video_planar_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "video_planar_abi_smoke: OK" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ 3. the way in's source
@pytest.fixture(scope="module")
def shim_in(tmp_path_factory):
    """k_video_planar_import.hip (and k_image_import.hip, for the tail) compiled as plain C++ under the sequential shim of tests/emu with the
    driver of tests/video_planar_in_emu -> the directory of ./emu and ./emu_san: the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "video_planar_in_emu", ("k_video_planar_import.hip", "fdh_video_planar.h", "fdh_video_import.h", "k_image_import.hip", "fdh_image_import.h"),
                           {"emu": (), "emu_san": emu_build.SAN}, opt="-O2")


def place_of(i, w, h):
    """an entry's place for case i: odd coordinates of every residue, and an atlas that just takes it"""
    x, y = 4 + (i * 7) % 13, 4 + (i * 5) % 11
    size = 16
    while size < max(x + w, y + h) + 4:
        size *= 2
    return x, y, size, min(size.bit_length(), 14)  # levels size, size / 2, .. 1


def through_the_shim_in(tmp, cases, exe="./emu"):
    """-> per case ([the stored levels], the ink block as 64 ints, the level-5 image), what the program printed"""
    places = []
    with open(os.path.join(tmp, "cases.bin"), "wb") as f:
        for i, case in enumerate(cases):
            w, h = VC.size_of(case)
            packed = VC.pack(case)
            x, y, size, n_levels = place_of(i, w, h)
            places.append((x, y, size, n_levels))
            f.write(np.array([w, h, case[1], case[2], case[3], case[4], *(p[2] for p in packed), *(p[1] for p in packed), *(len(p[0]) for p in packed), x, y, size, n_levels, 0], np.int32).tobytes())
            for p in packed:
                f.write(p[0])
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


def check_in(case, got):
    levels, block, level5 = got
    texels = VC.texels(case)
    want = SIB_IN.chain(texels)
    assert len(levels) == len(want), case[0]
    for l, (a, b) in enumerate(zip(levels, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{case[0]}: level {l} differs in {int((a != b).any(axis=2).sum())} texels"
    img = texels
    for _ in range(5):  # the level-5 image is made whether or not the chain reaches it
        img = SIB_IN.minify(img)
    assert np.array_equal(level5, img), f"{case[0]}: the level-5 image"
    boxes = SIB_IN.ink_boxes(texels)
    if boxes is None:
        assert block.reshape(16, 4).tolist() == [[32767, 32767, 0, 0]] * 16, case[0]  # untouched
    else:
        mine = block.reshape(16, 4).astype(np.int64)
        mine[mine[:, 2] == 0] = 0  # the host's reading: a box whose x1 is still 0 has no texel
        assert np.array_equal(mine, boxes), case[0]


def counts_of(said):
    words = said.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def wide_in(case, p):
    """the host's decision for plane p of a way-in case: one load per run"""
    data, align, pitch = VC.pack(case)[p]
    es = 1 if REF.bits_of(case[1]) == 8 else 2
    run = VC.run_of(case[1], p) * es
    return align % run == 0 and pitch % run == 0 and case[5][p].shape[1] * es >= run


@pytest.fixture(scope="module")
def emulated_in(shim_in):
    cases = VC.in_cases()
    got, said = through_the_shim_in(shim_in, cases)
    print(said.strip())
    return cases, got, said


def test_the_way_in_cases_cover_the_ground():
    cases = VC.in_cases()
    assert len({c[0] for c in cases}) == len(cases)
    assert {(c[1], c[4], c[2], c[3]) for c in cases} == {(f, fl, m, r) for f, fl in VC.KINDS for m, r in ROWS}  # every build meets every row
    for size in VC.IN_SIZES + [VC.IN_LARGEST]:
        assert {c[6] for c in cases if VC.size_of(c) == size} >= {"tight", "padded"}, size
    assert {(7, 5), (8, 8), (9, 3)} <= set(VC.IN_SIZES)  # the run of eight +- 1
    for kind in VC.KINDS:
        mine = [c for c in cases if (c[1], c[4]) == kind]
        assert any(c[6] == "aligned" and all(wide_in(c, p) for p in range(3)) for c in mine), kind
        assert any(not any(wide_in(c, p) for p in range(3)) for c in mine if VC.size_of(c)[0] >= 16), kind
    ten = [c for c in cases if REF.bits_of(c[1]) == 10]
    assert all((c[5][p] >> 10).any() for c in ten for p in range(3) if c[5][p].size > 8)  # garbage in the six high bits


def test_the_way_in_source_against_the_reference(emulated_in):
    """every level of every case, the level-5 image and the ink block, byte for byte; the program itself refuses a texel written outside the
    rectangles.  For 4:2:0 the reference's texels are also the sibling reference's texels of the interleaved frame"""
    cases, got, said = emulated_in
    for case, g in zip(cases, got):
        check_in(case, g)
        if not REF.full_chroma(case[1]):
            sib, luma, chroma = VC.interleaved(case)
            assert np.array_equal(VC.texels(case), SIB_IN.convert(luma, chroma, sib, case[2], case[3], case[4])), case[0]
    counts = counts_of(said)
    assert counts["cases"] == len(cases)
    for p, key in enumerate(("wide_y", "wide_cb", "wide_cr")):
        assert counts[key] == sum(wide_in(c, p) for c in cases)
    assert 0 < counts["wide_y"] < len(cases)


def test_the_way_in_shim_under_sanitizers(shim_in, emulated_in):
    """the stand-alone program built with -fsanitize=address,undefined on every case but the largest: a read past either end of a plane
    that ends with its last sample, a wide load at an address that is no multiple of its size, a store outside a level or the level-5
    image, is an error there"""
    cases, _, _ = emulated_in
    pick = [i for i, c in enumerate(cases) if VC.size_of(c) != VC.IN_LARGEST]
    assert len(pick) == len(cases) - 2  # (the largest size in its two layouts)
    got, _ = through_the_shim_in(shim_in, [cases[i] for i in pick], exe="./emu_san")
    for i, g in zip(pick, got):
        check_in(cases[i], g)


# ------------------------------------------------------------------------------------------------------------------ 4. the way out's source
@pytest.fixture(scope="module")
def shim_out(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "video_planar_out_emu", ("k_video_planar_export.hip", "fdh_video_planar.h", "fdh_video_export.h", "fdh_image_import.h"),
                           {"emu": (), "emu_san": emu_build.SAN}, opt="-O2")


def through_the_shim_out(tmp, cases, exe):
    """-> per case the planes' bytes as the program left them, and what it printed"""
    with open(os.path.join(tmp, "cases.bin"), "wb") as f:
        for case in cases:
            _, W, H, _, fmt, m, r, flags, _ = case
            lay = VC.layouts(case)
            f.write(np.array([W, H, *VC.rect_of(case), fmt, m, r, flags, *(l[1] for l in lay), *(l[0] for l in lay)], np.int32).tobytes())
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


def check_out(case, got):
    want = VC.expected_planes(case)
    assert len(got) == len(want) == 3, case[0]
    for p, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (case[0], p)
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{case[0]}: plane {p} differs in {int((a != b).sum())} bytes, the first at {at} (pitch {VC.layouts(case)[p][1]}): {a[at]} != {b[at]}")


def wide_out(case, p):
    """the host's decision for plane p of a way-out case: one store per run"""
    align, pitch, _, row_bytes = VC.layouts(case)[p]
    run = VC.run_of(case[4], p) * (1 if REF.bits_of(case[4]) == 8 else 2)
    return align % run == 0 and pitch % run == 0 and row_bytes >= run


def test_the_way_out_cases_cover_the_ground():
    cases = VC.out_cases()
    assert len({c[0] for c in cases}) == len(cases)
    want_sizes = set(VC.OUT_SIZES)
    assert want_sizes >= {(1, 1), (2, 1), (1, 2), (3, 3), (4, 2), (5, 7), (8, 2), (7, 3), (9, 2)} | {(w, h) for w in (127, 128, 129, 255, 256, 257) for h in (15, 16, 17)}
    for kind in VC.KINDS:
        mine = [c for c in cases if (c[4], c[7]) == kind]
        assert {(c[1], c[2]) for c in mine if c[3] is None} == want_sizes
        for size in want_sizes:
            assert {c[8] for c in mine if (c[1], c[2]) == size} == set(VC.LAYOUTS)
        assert {(c[5], c[6]) for c in mine} == set(ROWS)
        for p in range(3):  # both the wide and the sample-by-sample path store every plane, at the tile's sizes too
            assert {wide_out(c, p) for c in mine if c[1] >= 127} == {True, False}, (kind, p)
        rects = {c[3] for c in mine if c[3] is not None}
        assert rects == set(VC.RECTS) | (set(VC.ODD_RECTS) if REF.full_chroma(kind[0]) else set())


@pytest.fixture(scope="module")
def emulated_out(shim_out):
    cases = VC.out_cases()
    got, said = through_the_shim_out(shim_out, cases, "./emu")
    print(said.strip())
    return cases, got, said


def test_the_way_out_source_against_the_reference(emulated_out):
    """every plane of every case byte for byte, from the plane's pointer to its last sample's end: what lies between a row's end and the
    pitch is still 0xEE; a rectangle's planes are the export of the cropped frame; 10-bit words have their six high bits zero"""
    cases, got, said = emulated_out
    for case, g in zip(cases, got):
        check_out(case, g)
        if REF.bits_of(case[4]) == 10:
            assert all(int(p.max()) < 1024 for p in VC.planes_of(g, case)), case[0]
    counts = counts_of(said)
    assert counts["cases"] == len(cases)
    for p, key in enumerate(("wide_y", "wide_cb", "wide_cr")):
        assert counts[key] == sum(wide_out(c, p) for c in cases)
    assert 0 < counts["wide_src"] < len(cases)  # both ways of loading a run


def test_the_way_out_shim_under_sanitizers(shim_out, emulated_out):
    """the stand-alone program built with -fsanitize=address,undefined on every case: a read past either end of the source, a store outside
    a plane that ends with its last sample, a wide access at an address that is no multiple of its size, is an error there"""
    cases, _, _ = emulated_out
    got, _ = through_the_shim_out(shim_out, cases, "./emu_san")
    for case, g in zip(cases, got):
        check_out(case, g)


def test_round_trip_of_the_references():
    """video_planar_ref.convert(video_planar_ref.export(img)): 4:4:4 loses the quantisation alone, on noise too -- the point of the format
    for screen content; 4:2:0 loses the chroma of three texels in four (printed, not a tolerance for the device).  The 4:4:4 bound, from
    the headers' own error terms: a sample is within 0.5 + 0.04 of its exact value, the widest channel (blue, BT2020 limited) scales luma
    by 255 / 219 and Cb by 2 (1 - Kb) 255 / 224, which is 0.54 * 1.164 + 0.54 * 2.142 = 1.79 bytes, and the way in adds its own 0.5 + 0.094:
    under 2.4, so an 8-bit round trip moves a byte by at most 2; 10 bit quarters the first part: 0.45 + 0.6, at most 1"""
    rng = np.random.default_rng(11)
    noise = np.full((32, 32, 4), 255, np.uint8)
    noise[..., :3] = rng.integers(0, 256, size=(32, 32, 3))
    for fmt in REF.FORMATS:
        for m, r in ROWS:
            back = REF.convert(REF.export(noise, fmt, m, r), fmt, m, r)
            d = int(np.abs(back.astype(int) - noise).max())
            print(f"round trip {REF.NAMES[fmt]} matrix {m} range {r}: noise <= {d}")
            if REF.full_chroma(fmt):
                assert d <= (2 if REF.bits_of(fmt) == 8 else 1), (fmt, m, r, d)
