"""4:2:2 video in and out (fdh_put_video_422, fdh_update_video_422, fdh_read_video_422, fdh_check_video_422_target;
include_video/figdraw_hip_video_422.h), what a CPU can check: the reference tests/video_422_ref.py against the 4:2:0 reference on doubled
rows and repeated chroma rows, and its packed layouts against its planar ones; known answers and the float64 bound for N = 2 and N = 4;
every refusal without a device and through C99; and the sources of k_video_422_import.hip and k_video_422_export.hip under the host shim
of tests/emu (tests/video_422_in_emu, tests/video_422_out_emu) against the reference, byte for byte, padding included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_build
import video_frame_ref as SIB_IN
import video_planar_ref as PL
import video_422_cases as VC
import video_422_ref as REF
from conftest import ROOT
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext

INVALID = -1
ROWS = [(m, r) for m in (REF.BT601, REF.BT709, REF.BT2020) for r in (REF.LIMITED, REF.FULL)]
RULES = (0, REF.CHROMA_LINEAR)
CHROMA_BOUND = 2 * 255 / 16384  # the header: the same for N = 2 and N = 4
PLANAR = ((REF.I422, PL.I420), (REF.I210, PL.I010))  # a three-plane 4:2:2 format and the 4:2:0 format of its bit depth


def noise_image(rng, w, h):
    return rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ 1. the reference
def test_the_planar_way_out_is_the_420_export_of_doubled_rows():
    """an image with each row doubled: the 4:2:0 chroma sample averages two equal rows, which is the 4:2:2 sample of either"""
    rng = np.random.default_rng(41)
    for w, h in ((1, 1), (2, 3), (5, 4), (9, 2), (33, 7)):
        img = noise_image(rng, w, h)
        doubled = np.repeat(img, 2, axis=0)
        for m, r in ROWS:
            for flags in RULES:
                for fmt, sib in PLANAR:
                    y, cb, cr = REF.export(img, fmt, m, r, flags)
                    sy, scb, scr = PL.export(doubled, sib, m, r, flags)
                    assert scb.shape == cb.shape == (h, (w + 1) // 2) and np.array_equal(cb, scb) and np.array_equal(cr, scr), (w, h, fmt, m, r, flags)
                    assert np.array_equal(sy[0::2], sy[1::2]) and np.array_equal(sy[0::2], y), (w, h, fmt, m, r, flags)  # the luma rows: pairwise equal
                    dy, dcb, dcr = REF.export(doubled, fmt, m, r, flags)  # and the doubled image's own 4:2:2 planes: every 4:2:0 row twice
                    assert np.array_equal(dcb, np.repeat(scb, 2, axis=0)) and np.array_equal(dcr, np.repeat(scr, 2, axis=0)) and np.array_equal(dy, sy)
                    assert y.dtype == cb.dtype == cr.dtype == REF.dtype_of(fmt) and int(max(y.max(), cb.max(), cr.max())) < 1 << REF.bits_of(fmt)
    for fmt, sib in ((REF.I422, SIB_IN.NV12), (REF.I210, SIB_IN.P010), (REF.YUY2, SIB_IN.NV12), (REF.UYVY, SIB_IN.NV12)):
        for m, r in ROWS:  # an 8-bit format uses the NV12 row of either table, I210 the P010 row
            assert REF.in_coefficients(fmt, m, r) == context.video_coefficients(sib, m, r)
            assert REF.out_coefficients(fmt, m, r) == context.video_out_coefficients(sib, m, r)


def test_the_planar_way_in_is_the_420_convert_where_chroma_is_constant_down_the_columns():
    """one chroma row repeated: the 4:2:0 linear rule's far row equals its near row, and (3 c + c + 2) >> 2 = c"""
    rng = np.random.default_rng(42)
    for w, h in ((1, 1), (2, 3), (5, 4), (9, 2), (33, 7)):
        cw = (w + 1) // 2
        for fmt, sib in PLANAR:
            top = 256 if REF.bits_of(fmt) == 8 else 65536  # (garbage in the six high bits of a 10-bit word)
            y = rng.integers(0, top, size=(h, w)).astype(REF.dtype_of(fmt))
            rows = [rng.integers(0, top, size=(1, cw)).astype(REF.dtype_of(fmt)) for _ in range(2)]
            c422 = [np.repeat(c, h, axis=0) for c in rows]
            c420 = [np.repeat(c, (h + 1) // 2, axis=0) for c in rows]
            for m, r in ROWS:
                for flags in RULES:
                    assert np.array_equal(REF.convert((y, *c422), fmt, m, r, flags), PL.convert((y, *c420), sib, m, r, flags)), (w, h, fmt, m, r, flags)


def test_the_packed_formats_are_the_i422_samples_interleaved():
    rng = np.random.default_rng(43)
    for w, h in ((1, 1), (2, 1), (3, 2), (8, 3), (9, 2), (33, 5)):
        cw = (w + 1) // 2
        img = noise_image(rng, w, h)
        for m, r in ROWS[::2]:
            for flags in RULES:
                y, cb, cr = REF.export(img, REF.I422, m, r, flags)
                for fmt, (iy, ic) in ((REF.YUY2, (0, 1)), (REF.UYVY, (1, 0))):
                    (plane,) = REF.export(img, fmt, m, r, flags)
                    assert plane.shape == (h, 4 * cw) and plane.dtype == np.uint8
                    for x in range(w):  # byte by byte: column x is luma x & 1 of group x >> 1
                        assert np.array_equal(plane[:, 4 * (x >> 1) + iy + 2 * (x & 1)], y[:, x]), (w, h, fmt, x)
                    for i in range(cw):
                        assert np.array_equal(plane[:, 4 * i + ic], cb[:, i]) and np.array_equal(plane[:, 4 * i + ic + 2], cr[:, i]), (w, h, fmt, i)
                    if w & 1:  # the odd width's last group is whole: its second luma is column w - 1's
                        assert np.array_equal(plane[:, 4 * (cw - 1) + iy + 2], y[:, w - 1])
                    # and back: the de-interleaved samples are the planes, and convert to the same texels
                    back = REF.deinterleave(plane, fmt, w)
                    assert all(np.array_equal(a, b) for a, b in zip(back, (y, cb, cr)))
                    assert np.array_equal(REF.convert((plane,), fmt, m, r, flags, w=w), REF.convert((y, cb, cr), REF.I422, m, r, flags))
        # the way in, on noise: a packed frame converts as the I422 frame of its samples
        for fmt in (REF.YUY2, REF.UYVY):
            (plane,) = VC.noise_stored(rng, fmt, w, h)
            assert np.array_equal(REF.convert((plane,), fmt, REF.BT709, REF.FULL, REF.CHROMA_LINEAR, w=w),
                                  REF.convert(REF.deinterleave(plane, fmt, w), REF.I422, REF.BT709, REF.FULL, REF.CHROMA_LINEAR))


def flat(rgb, w=3, h=3):
    img = np.zeros((h, w, 4), np.uint8)
    img[..., :3] = rgb
    img[..., 3] = 77  # (ignored)
    return img


def test_known_answers():
    for fmt in (REF.I422, REF.I210):
        for m, r in ROWS:
            for flags in RULES:
                yoff, yden, _, coff = REF.ranges(fmt, r)
                y, cb, cr = REF.export(flat((0, 0, 0)), fmt, m, r, flags)
                assert y.shape == (3, 3) and cb.shape == cr.shape == (3, 2) and (y == yoff).all() and (cb == coff).all() and (cr == coff).all(), (fmt, m, r)
                y, cb, cr = REF.export(flat((255, 255, 255)), fmt, m, r, flags)
                assert (y == yoff + yden).all() and (cb == coff).all() and (cr == coff).all(), (fmt, m, r)
                greys = np.zeros((16, 16, 4), np.uint8)
                greys[..., :3] = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)  # every grey, beside its neighbours
                y, cb, cr = REF.export(greys, fmt, m, r, flags)
                assert (cb == coff).all() and (cr == coff).all() and (np.diff(y.astype(int).ravel()) >= 0).all(), (fmt, m, r)
    for m in (REF.BT601, REF.BT709, REF.BT2020):  # pure blue and pure red in 8-bit full range: 256 in front of the clamp, under both rules
        k = REF.out_coefficients(REF.I422, m, REF.FULL)
        for n, shift in ((2, 15), (4, 16)):
            assert k[1] + ((k[7] * 255 * n + (n << 13)) >> shift) == 256 and k[1] + ((k[8] * 255 * n + (n << 13)) >> shift) == 256
        for flags in RULES:
            assert (REF.export(flat((0, 0, 255)), REF.I422, m, REF.FULL, flags)[1] == 255).all()
            assert (REF.export(flat((255, 0, 0)), REF.I422, m, REF.FULL, flags)[2] == 255).all()
            assert (REF.export(flat((0, 0, 255)), REF.UYVY, m, REF.FULL, flags)[0][:, 0::4] == 255).all()
    # one pair by hand, BT601 full range, 8 bit, the texels (10, 20, 200) and (30, 40, 100): s = (40, 60, 300), N = 2;
    # kU = (-2765, -5427, 8192), kV = (8192, -6860, -1332)
    #   Cb = 128 + ((-110600 - 325620 + 2457600 + 16384) >> 15) = 128 + (2037764 >> 15) = 128 + 62 = 190   (exactly 189.69)
    #   Cr = 128 + ((327680 - 411600 - 399600 + 16384) >> 15) = 128 + (-467136 >> 15) = 128 - 15 = 113      (exactly 113.24; -14.26 floors to -15)
    #   Y0 = (4899 * 10 + 9617 * 20 + 1868 * 200 + 8192) >> 14 = 623122 >> 14 = 38
    #   Y1 = (4899 * 30 + 9617 * 40 + 1868 * 100 + 8192) >> 14 = 726642 >> 14 = 44
    pair = np.array([[[10, 20, 200, 255], [30, 40, 100, 0]]], np.uint8)
    assert REF.out_coefficients(REF.I422, REF.BT601, REF.FULL)[5:] == (-2765, -5427, 8192, 8192, -6860, -1332)
    y, cb, cr = REF.export(pair, REF.I422, REF.BT601, REF.FULL)
    assert (y.tolist(), cb.tolist(), cr.tolist()) == ([[38, 44]], [[190]], [[113]])
    assert REF.export(pair, REF.YUY2, REF.BT601, REF.FULL)[0].tolist() == [[38, 190, 44, 113]]
    assert REF.export(pair, REF.UYVY, REF.BT601, REF.FULL)[0].tolist() == [[190, 38, 113, 44]]
    #   with FDH_VIDEO_CHROMA_LINEAR: xl = xc = 0, xr = 1: s = 3 * (10, 20, 200) + (30, 40, 100) = (60, 100, 700), N = 4
    #   Cb = 128 + ((-165900 - 542700 + 5734400 + 32768) >> 16) = 128 + (5058568 >> 16) = 128 + 77 = 205
    assert REF.export(pair, REF.I422, REF.BT601, REF.FULL, REF.CHROMA_LINEAR)[1].tolist() == [[205]]
    # the way in: the chroma of a row alone.  Four columns over the samples (128, 128) and (255, 0), mid grey luma, two rows that differ
    Y = np.full((2, 4), 128, np.uint8)
    cb, cr = np.array([[128, 255], [0, 128]], np.uint8), np.array([[128, 0], [128, 128]], np.uint8)
    got = REF.convert((Y, cb, cr), REF.I422, REF.BT601, REF.FULL)
    assert got[0, 0].tolist() == got[0, 1].tolist() == [128, 128, 128, 255] and np.array_equal(got[0, 2], got[0, 3]) and got[0, 2, 2] == 255 and got[0, 2, 0] == 0
    assert np.array_equal(got, SIB_IN.yuv_to_rgba(Y, cb[:, [0, 0, 1, 1]], cr[:, [0, 0, 1, 1]], SIB_IN.NV12, REF.BT601, REF.FULL))  # the sibling's per-texel rule
    lin = REF.convert((Y, cb, cr), REF.I422, REF.BT601, REF.FULL, REF.CHROMA_LINEAR)
    mid_b, mid_r = (128 + 255 + 1) >> 1, (128 + 0 + 1) >> 1  # column 1 lies midway; column 3 has no right neighbour: the last sample again
    assert np.array_equal(lin, SIB_IN.yuv_to_rgba(Y, np.array([[128, mid_b, 255, 255], [0, 64, 128, 128]]), np.array([[128, mid_r, 0, 0], [128, 128, 128, 128]]), SIB_IN.NV12, REF.BT601, REF.FULL))


def test_the_way_in_ignores_the_high_bits_and_the_odd_widths_last_byte():
    Y10 = np.array([[64, 64 | 0xFC00]], np.uint16)
    c10 = np.array([[512 | 0xA400]], np.uint16)
    assert REF.convert((Y10, c10, c10), REF.I210, REF.BT709, REF.LIMITED).tolist() == [[[0, 0, 0, 255]] * 2]
    rng = np.random.default_rng(44)
    for fmt, at in ((REF.YUY2, 2), (REF.UYVY, 3)):
        for w in (1, 5, 9):
            (plane,) = VC.noise_stored(rng, fmt, w, 3)
            other = plane.copy()
            other[:, 4 * ((w + 1) // 2 - 1) + at] ^= 0xFF
            for flags in RULES:
                assert np.array_equal(REF.convert((plane,), fmt, REF.BT601, REF.FULL, flags, w=w), REF.convert((other,), fmt, REF.BT601, REF.FULL, flags, w=w))
            other[:, at - 2] ^= 0xFF  # (the first luma byte of the first group is not ignored)
            assert not np.array_equal(REF.convert((plane,), fmt, REF.BT601, REF.FULL, w=w), REF.convert((other,), fmt, REF.BT601, REF.FULL, w=w))


def test_chroma_against_float64_within_the_bound():
    """a dense sample of colour pairs (N = 2) and triples (N = 4) -- every pair and triple of the cube's corners, pairs along the lattice of
    every (R, B) with its complement, and noise --: never more than 1 from the rounded float64 value of the averaged colour, and equal to
    it wherever that lies further from a half than 2 * 255 / 16384"""
    rng = np.random.default_rng(7)
    corners = np.array([[(i & 1) * 255, (i >> 1 & 1) * 255, (i >> 2 & 1) * 255] for i in range(8)])
    r, b = np.meshgrid(np.arange(0, 256, 3), np.arange(0, 256, 3), indexing="ij")
    lattice = np.concatenate([np.stack([r.ravel(), np.full(r.size, g), b.ravel()], axis=1) for g in (0, 51, 128, 204, 255)])
    assert CHROMA_BOUND < 0.032
    sets = {
        2: (np.concatenate([corners[np.arange(64) // 8], lattice, lattice, rng.integers(0, 256, size=(200_000, 3))]),
            np.concatenate([corners[np.arange(64) % 8], 255 - lattice, np.roll(lattice, 1777, axis=0), rng.integers(0, 256, size=(200_000, 3))])),
        4: (np.concatenate([corners[np.arange(512) // 64], lattice, rng.integers(0, 256, size=(200_000, 3))]),
            np.concatenate([corners[np.arange(512) // 8 % 8], 255 - lattice, rng.integers(0, 256, size=(200_000, 3))]),
            np.concatenate([corners[np.arange(512) % 8], np.roll(lattice, 977, axis=0), rng.integers(0, 256, size=(200_000, 3))])),
    }
    for fmt in (REF.I422, REF.I210):
        top = (1 << REF.bits_of(fmt)) - 1
        for m, rg in ROWS:
            for n, cols in sets.items():
                s = cols[0] + cols[1] if n == 2 else cols[0] + 2 * cols[1] + cols[2]
                got = np.stack(REF.chroma_of_sums(s, n, fmt, m, rg), axis=-1)
                exact = np.stack(REF.chroma_float(s / float(n), fmt, m, rg), axis=-1)
                d = np.abs(got - np.clip(np.rint(exact), 0, top).astype(np.int64))
                from_half = np.abs(exact - np.floor(exact) - 0.5)
                assert d.max() <= 1, (fmt, m, rg, n, int(d.max()))
                assert not d[from_half > CHROMA_BOUND].any(), (fmt, m, rg, n)
    # and the sums of an image are those of its pairs and triples
    img = noise_image(rng, 7, 2)[..., :3].astype(np.int64)
    s2, n2 = REF.chroma_sums(img, False)
    s4, n4 = REF.chroma_sums(img, True)
    assert (n2, n4) == (2, 4) and s2.shape == s4.shape == (2, 4, 3)
    assert np.array_equal(s2[:, 1], img[:, 2] + img[:, 3]) and np.array_equal(s2[:, 3], 2 * img[:, 6])
    assert np.array_equal(s4[:, 0], 3 * img[:, 0] + img[:, 1]) and np.array_equal(s4[:, 2], img[:, 3] + 2 * img[:, 4] + img[:, 5]) and np.array_equal(s4[:, 3], img[:, 5] + 3 * img[:, 6])


# ------------------------------------------------------------------------------------------------------------------ 2. the rules
FW, FH = 16, 9
Y0, CB0, CR0 = 0x10000, 0x20000, 0x30000


def target(**kw):
    """a valid I422 target for the whole of a 16 x 9 frame at made-up addresses (nothing is read or written without a device)"""
    base = dict(ptrs=(Y0, CB0, CR0), pitches=(16, 8, 8), format=REF.I422, matrix=REF.BT709, range=REF.LIMITED, flags=0, rect=None, reserved=(0, 0))
    base.update(kw)
    t = context.video_planes_target(base["ptrs"], base["pitches"], base["format"], base["matrix"], base["range"], base["flags"], base["rect"])
    t.reserved[0], t.reserved[1] = base["reserved"]
    return t


def frame(**kw):
    """the same as a source: 16 x 9 I422"""
    base = dict(ptrs=(Y0, CB0, CR0), pitches=(16, 8, 8), width=FW, height=FH, format=REF.I422, matrix=REF.BT709, range=REF.LIMITED, flags=0, reserved=(0, 0))
    base.update(kw)
    f = context.video_planes(base["ptrs"], base["width"], base["height"], base["pitches"], base["format"], base["matrix"], base["range"], base["flags"])
    f.reserved[0], f.reserved[1] = base["reserved"]
    return f


I210 = dict(format=REF.I210, pitches=(32, 16, 16))
YUY2 = dict(format=REF.YUY2, ptrs=(Y0, 0, 0), pitches=(32, 0, 0))
UYVY = dict(format=REF.UYVY, ptrs=(Y0, 0, 0), pitches=(32, 0, 0))


def multiple(p, unit="sample size"):
    return f"planes[{p}] and pitch_bytes[{p}] must be multiples of the {unit}"


def below(p):
    return f"pitch_bytes[{p}] is below a row's bytes"


ALPHA = "the alpha flags are BGRA8's"
ONE_PLANE = "planes[1], planes[2] and their pitches must be 0 for YUY2 / UYVY: one plane"
GROUP = "group size"
# (keywords one step from a valid struct, the text behind the call's name; None: the null text): the rules both directions share
SHARED = [
    (dict(ptrs=(0, CB0, CR0)), None), (dict(ptrs=(Y0, 0, CR0)), None), (dict(ptrs=(Y0, CB0, 0)), None), (dict(I210, ptrs=(Y0, CB0, 0)), None),
    (dict(YUY2, ptrs=(0, 0, 0)), None), (dict(UYVY, ptrs=(0, 0, 0)), None),
    (dict(YUY2, ptrs=(Y0, CB0, 0)), ONE_PLANE), (dict(YUY2, ptrs=(Y0, 0, CR0)), ONE_PLANE), (dict(UYVY, pitches=(32, 8, 0)), ONE_PLANE), (dict(UYVY, pitches=(32, 0, 8)), ONE_PLANE),
    (dict(YUY2, ptrs=(Y0, CB0, CR0), pitches=(32, 8, 8)), ONE_PLANE),
] + [(dict(format=f), "unknown format") for f in (0, 1, 2, 3, 4, 5, 6, 11, 2 ** 31)] + [
    (dict(matrix=3), "unknown matrix"), (dict(range=2), "unknown range"), (dict(YUY2, matrix=7), "unknown matrix"),
    (dict(flags=8), "unknown flag"), (dict(flags=1 | 1 << 31), "unknown flag"), (dict(UYVY, flags=16), "unknown flag"),
    (dict(reserved=(7, 0)), "reserved must be 0"), (dict(reserved=(0, 1)), "reserved must be 0"), (dict(YUY2, reserved=(0, 1)), "reserved must be 0"),
    (dict(flags=REF.STRAIGHT_ALPHA), ALPHA), (dict(flags=REF.IGNORE_ALPHA | REF.CHROMA_LINEAR), ALPHA), (dict(UYVY, flags=REF.IGNORE_ALPHA), ALPHA),
    (dict(I210, ptrs=(Y0 + 1, CB0, CR0)), multiple(0)), (dict(I210, ptrs=(Y0, CB0 + 1, CR0)), multiple(1)), (dict(I210, ptrs=(Y0, CB0, CR0 + 1)), multiple(2)),
    (dict(I210, pitches=(33, 16, 16)), multiple(0)), (dict(I210, pitches=(32, 17, 16)), multiple(1)), (dict(I210, pitches=(32, 16, 17)), multiple(2)),
    (dict(YUY2, ptrs=(Y0 + 2, 0, 0)), multiple(0, GROUP)), (dict(UYVY, ptrs=(Y0 + 1, 0, 0)), multiple(0, GROUP)), (dict(YUY2, pitches=(34, 0, 0)), multiple(0, GROUP)),
    (dict(UYVY, pitches=(33, 0, 0)), multiple(0, GROUP)),
    (dict(pitches=(15, 8, 8)), below(0)), (dict(pitches=(-16, 8, 8)), below(0)), (dict(pitches=(16, 7, 8)), below(1)), (dict(pitches=(16, 8, 0)), below(2)),
    (dict(I210, pitches=(30, 16, 16)), below(0)), (dict(I210, pitches=(32, 16, 14)), below(2)),
    (dict(YUY2, pitches=(28, 0, 0)), below(0)), (dict(UYVY, pitches=(0, 0, 0)), below(0)), (dict(UYVY, pitches=(-32, 0, 0)), below(0)),
]
OUTSIDE = "rectangle outside the frame"
EVEN = "the rectangle's x must be even for 4:2:2"
CH_BYTES = 8 * (FH - 1) + 8  # a chroma plane of the valid struct: nine rows
TARGET_ONLY = [
    (dict(rect=(2, 0, 15, 9)), OUTSIDE), (dict(rect=(0, 2, 16, 8)), OUTSIDE), (dict(rect=(-2, 0, 4, 4)), OUTSIDE), (dict(rect=(0, -1, 4, 4)), OUTSIDE),
    (dict(rect=(16, 0, 1, 1)), OUTSIDE), (dict(YUY2, rect=(2, 1, 16, 8)), OUTSIDE), (dict(rect=(2, 2, 2 ** 31 - 1, 2)), OUTSIDE),
    (dict(rect=(1, 0, 4, 4)), EVEN), (dict(rect=(3, 3, 4, 4)), EVEN), (dict(I210, rect=(5, 4, 2, 2)), EVEN), (dict(YUY2, rect=(7, 0, 2, 2)), EVEN), (dict(UYVY, rect=(15, 8, 1, 1)), EVEN),
    (dict(rect=(0, 0, 15, 9), pitches=(16, 7, 8)), below(1)),  # ceil(15 / 2) = 8 samples
    (dict(YUY2, rect=(0, 0, 15, 9), pitches=(28, 0, 0)), below(0)),  # ... = 8 groups
    (dict(ptrs=(Y0, Y0, CR0)), "planes 0 and 1 overlap"), (dict(ptrs=(Y0, CB0, Y0 + 16 * 9 - 1)), "planes 0 and 2 overlap"),
    (dict(ptrs=(Y0, CB0, CB0 + CH_BYTES - 1)), "planes 1 and 2 overlap"), (dict(ptrs=(CB0 + CH_BYTES - 1, CB0, CR0)), "planes 0 and 1 overlap"),
    (dict(I210, ptrs=(Y0, CB0, CB0 + 2 * CH_BYTES - 2)), "planes 1 and 2 overlap"),
]
ACCEPTED = [
    dict(), I210, YUY2, UYVY, dict(flags=REF.CHROMA_LINEAR), dict(I210, flags=REF.CHROMA_LINEAR), dict(YUY2, flags=REF.CHROMA_LINEAR), dict(UYVY, flags=REF.CHROMA_LINEAR),
    dict(ptrs=(Y0, Y0 + 16 * 9, Y0 + 16 * 9 + CH_BYTES)), dict(ptrs=(CB0 + CH_BYTES, CB0, CR0)),  # the planes touch
    dict(rect=(2, 4, 13, 5)), dict(rect=(2, 3, 13, 5)), dict(rect=(14, 7, 1, 1)), dict(I210, rect=(0, 1, 3, 3)),  # odd w and h; an odd y
    dict(rect=(0, 0, 0, 5)), dict(rect=(7, 7, -1, 0)), dict(YUY2, rect=(3, 3, 0, 0)),  # (w or h <= 0: the whole frame)
    dict(YUY2, rect=(2, 3, 13, 5), pitches=(28, 0, 0)), dict(UYVY, rect=(14, 8, 1, 1), pitches=(4, 0, 0)), dict(I210, rect=(2, 1, 3, 3), pitches=(6, 4, 4)),
    dict(ptrs=(Y0 + 1, CB0 + 3, CR0 + 5), pitches=(17, 9, 11)), dict(I210, ptrs=(Y0 + 2, CB0 + 6, CR0 + 10), pitches=(34, 18, 22)), dict(YUY2, ptrs=(Y0 + 4, 0, 0), pitches=(36, 0, 0)),
    dict(rect=(0, 0, 15, 9), pitches=(15, 8, 8)),
]


def test_check_video_422_target_applies_every_rule():
    L = context.load()
    for i, kw in enumerate(ACCEPTED):
        t = target(**kw)
        assert L.fdh_check_video_422_target(C.byref(t), FW, FH) == 0, (i, L.fdh_last_error().decode())
        context.check_video_422_target(t, FW, FH)
    for i, (kw, text) in enumerate(SHARED + TARGET_ONLY):
        t = target(**kw)
        assert L.fdh_check_video_422_target(C.byref(t), FW, FH) == INVALID, (i, kw)
        assert L.fdh_last_error().decode() == f"check_video_422_target: {text or 'null target or plane'}", (i, kw)
    assert L.fdh_check_video_422_target(None, FW, FH) == INVALID and L.fdh_last_error().decode() == "check_video_422_target: null target or plane"
    for fw, fh in ((0, 9), (16, 0), (-1, -1)):
        assert L.fdh_check_video_422_target(C.byref(target()), fw, fh) == INVALID and L.fdh_last_error().decode() == "check_video_422_target: empty frame"
    with pytest.raises(FigdrawHipError) as e:
        context.check_video_422_target(target(format=6), FW, FH)
    assert e.value.code == INVALID and str(e.value).endswith("check_video_422_target: unknown format")


def packed_area(ctx):
    area = C.c_int64()
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(area)) == 0
    return area.value


def test_refusals_on_the_way_in_leave_directory_packer_and_epoch_untouched():
    ctx = HipContext(atlas_size=256, record_only=True)
    L = ctx.L
    assert ctx.put_video_422(7, (Y0, CB0, CR0), FW, FH, (16, 8, 8))[2:] == (FW, FH)
    out = (C.c_int * 4)()
    before = (ctx.atlas_usage(), packed_area(ctx))
    refused = [(frame(**kw), text or "null frame or plane") for kw, text in SHARED] + [
        (None, "null frame or plane"), (frame(width=0), "empty frame"), (frame(height=-2), "empty frame"), (frame(**dict(YUY2, width=-1)), "empty frame"),
        (frame(width=15, pitches=(15, 7, 8)), below(1)), (frame(**dict(UYVY, width=15, pitches=(28, 0, 0))), below(0))]
    for i, (f, text) in enumerate(refused):
        ref = C.byref(f) if f is not None else None
        for name, call in (("put_video_422", lambda: L.fdh_put_video_422(ctx.h, 9, ref, out)), ("update_video_422", lambda: L.fdh_update_video_422(ctx.h, 7, ref))):
            assert call() == INVALID, (i, name)
            assert L.fdh_last_error().decode() == f"{name}: {text}", (i, name)
            assert (ctx.atlas_usage(), packed_area(ctx)) == before and not ctx.has_image(9), (i, name)
    assert L.fdh_update_video_422(ctx.h, 9, C.byref(frame())) == INVALID and L.fdh_last_error().decode() == "update_video_422: unknown key"
    for f in (frame(width=15), frame(height=10), frame(**dict(YUY2, width=8))):
        assert L.fdh_update_video_422(ctx.h, 7, C.byref(f)) == INVALID and L.fdh_last_error().decode() == "update_video_422: size mismatch"
    assert (ctx.atlas_usage(), packed_area(ctx)) == before
    # the three sibling families keep refusing every format value from 7 on
    for fmt in REF.FORMATS:
        old = context.video_frame(Y0, CB0, FW, FH, 16, 16, fmt)
        assert L.fdh_put_video_frame(ctx.h, 9, C.byref(old), out) == INVALID and L.fdh_last_error().decode() == "put_video_frame: unknown format"
        assert L.fdh_update_video_frame(ctx.h, 7, C.byref(old)) == INVALID and L.fdh_last_error().decode() == "update_video_frame: unknown format"
        assert L.fdh_check_video_target(C.byref(context.video_target(Y0, CB0, 16, 16, format=fmt)), FW, FH) == INVALID
        assert L.fdh_put_video_planes(ctx.h, 9, C.byref(frame(format=fmt)), out) == INVALID and L.fdh_last_error().decode() == "put_video_planes: unknown format"
        assert L.fdh_update_video_planes(ctx.h, 7, C.byref(frame(format=fmt))) == INVALID and L.fdh_last_error().decode() == "update_video_planes: unknown format"
        assert L.fdh_check_video_planes_target(C.byref(target(format=fmt)), FW, FH) == INVALID and L.fdh_last_error().decode() == "check_video_planes_target: unknown format"
    assert (ctx.atlas_usage(), packed_area(ctx)) == before and not ctx.has_image(9)
    # a call that goes through moves the epoch, and a put the packer too; the planes may alias each other on the way in; the next frame may
    # come in another of the four formats
    ctx.update_video_422(7, (Y0, Y0, Y0), FW, FH, (32, 32, 32), format=REF.I210, matrix=REF.BT2020, range=REF.FULL)
    ctx.update_video_422(7, (Y0, 0, 0), FW, FH, (32, 0, 0), format=REF.UYVY)
    after = ctx.atlas_usage()
    assert after["epoch"] == before[0]["epoch"] + 2 and packed_area(ctx) == before[1]
    assert ctx.put_video_422(9, (Y0 + 4, 0, 0), 15, 9, (36, 0, 0), format=REF.YUY2, flags=REF.CHROMA_LINEAR)[2:] == (15, 9)
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
    assert ctx.L.fdh_read_video_422(ctx.h, C.byref(target())) == INVALID
    assert ctx.L.fdh_last_error().decode().startswith("read_video_422: ")
    with pytest.raises(FigdrawHipError):
        ctx.read_video_422((Y0, 0, 0), (32, 0, 0), format=REF.YUY2)
    assert ctx.L.fdh_read_video_422(None, C.byref(target())) == INVALID
    ctx.close()


def test_the_format_values():
    assert (context.VIDEO_I422, context.VIDEO_I210, context.VIDEO_YUY2, context.VIDEO_UYVY) == (7, 8, 9, 10) == REF.FORMATS


def test_video_422_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "video_422_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_video"),
                           os.path.join(ROOT, "tests", "video_422_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "video_422_abi_smoke: OK" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ 3. the way in's source
@pytest.fixture(scope="module")
def shim_in(tmp_path_factory):
    """k_video_422_import.hip (and k_image_import.hip, for the tail) compiled as plain C++ under the sequential shim of tests/emu with the
    driver of tests/video_422_in_emu -> the directory of ./emu and ./emu_san: the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "video_422_in_emu", ("k_video_422_import.hip", "fdh_video_422.h", "fdh_video_import.h", "k_image_import.hip", "fdh_image_import.h"),
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
            packed += [(b"", 0, 0)] * (3 - len(packed))  # a one-plane format: nothing for the other two
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


def index_of(build):
    """the programs' number of a build (kTen, kPacked, kLinear)"""
    ten, packed, linear = build
    return (4 if packed else 2 * ten) + linear


def check_wide_counts(counts, cases, kind_of, wide, extra=None):
    """what the program counted per build and plane is the host rule's prediction, and every build took both paths on every plane it has"""
    assert counts["cases"] == len(cases)
    for build in VC.BUILDS:
        b, mine = index_of(build), [c for c in cases if VC.build_of(*kind_of(c)) == build]
        assert counts[f"b{b}_cases"] == len(mine) > 0, build
        for p in range(3):
            want = sum(wide(c, p) for c in mine) if p == 0 or not build[1] else 0
            assert counts[f"b{b}_wide_{p}"] == want, (build, p)
            if p == 0 or not build[1]:
                assert 0 < want < len(mine), (build, p)
        if extra:
            assert 0 < counts[f"b{b}_{extra}"] < len(mine), (build, extra)


@pytest.fixture(scope="module")
def emulated_in(shim_in):
    cases = VC.in_cases()
    got, said = through_the_shim_in(shim_in, cases)
    print(said.strip())
    return cases, got, said


def test_the_way_in_cases_cover_the_ground():
    cases = VC.in_cases()
    assert len({c[0] for c in cases}) == len(cases)
    assert {(c[1], c[4], c[2], c[3]) for c in cases} == {(f, fl, m, r) for f, fl in VC.KINDS for m, r in ROWS}  # every kind, so every build, meets every row
    assert {VC.build_of(c[1], c[4]) for c in cases} == set(VC.BUILDS) and len(VC.BUILDS) == 6
    for size in VC.IN_SIZES + [VC.IN_LARGEST]:
        assert {c[6] for c in cases if VC.size_of(c) == size} >= {"tight", "padded"}, size
    assert {c[6] for c in cases} == set(VC.LAYOUTS)
    assert {(7, 5), (8, 8), (9, 3), (31, 33), (33, 31), (1, 1)} <= set(VC.IN_SIZES)  # the run of eight +- 1, the tile +- 1
    import video_frame_cases as FC
    assert set(FC.SIZES) <= set(VC.IN_SIZES) and VC.IN_LARGEST == FC.LARGEST
    for kind in VC.KINDS:
        mine = [c for c in cases if (c[1], c[4]) == kind]
        n = len(mine[0][5])
        assert any(c[6] == "aligned" and all(VC.wide_in(c, p) for p in range(n)) for c in mine), kind
        assert any(not any(VC.wide_in(c, p) for p in range(n)) for c in mine if VC.size_of(c)[0] >= 16), kind
    ten = [c for c in cases if REF.bits_of(c[1]) == 10]
    assert all((c[5][p] >> 10).any() for c in ten for p in range(3) if c[5][p].size > 8)  # garbage in the six high bits
    assert any(VC.size_of(c)[0] & 1 for c in cases if REF.packed(c[1]))  # an odd width's last group, with noise in its second luma byte


def test_the_way_in_source_against_the_reference(emulated_in):
    """every level of every case, the level-5 image and the ink block, byte for byte; the program itself refuses a texel written outside the
    rectangles"""
    cases, got, said = emulated_in
    for case, g in zip(cases, got):
        check_in(case, g)
    check_wide_counts(counts_of(said), cases, lambda c: (c[1], c[4]), VC.wide_in)


def test_the_way_in_shim_under_sanitizers(shim_in, emulated_in):
    """the stand-alone program built with -fsanitize=address,undefined on every case but the largest: a read past either end of a plane
    that ends with its last row's end, a wide load at an address that is no multiple of its size, a store outside a level or the level-5
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
    return emu_build.build(tmp_path_factory, "video_422_out_emu", ("k_video_422_export.hip", "fdh_video_422.h", "fdh_video_export.h", "fdh_image_import.h"),
                           {"emu": (), "emu_san": emu_build.SAN}, opt="-O2")


def through_the_shim_out(tmp, cases, exe):
    """-> per case the planes' bytes as the program left them, and what it printed"""
    with open(os.path.join(tmp, "cases.bin"), "wb") as f:
        for case in cases:
            _, W, H, _, fmt, m, r, flags, _ = case
            lay = VC.layouts(case)
            lay += [(0, 0, 0, 0)] * (3 - len(lay))
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
    assert len(got) == len(want) == (1 if REF.packed(case[4]) else 3), case[0]
    for p, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (case[0], p)
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{case[0]}: plane {p} differs in {int((a != b).sum())} bytes, the first at {at} (pitch {VC.layouts(case)[p][1]}): {a[at]} != {b[at]}")


def test_the_way_out_cases_cover_the_ground():
    cases = VC.out_cases()
    assert len({c[0] for c in cases}) == len(cases)
    want_sizes = set(VC.OUT_SIZES)
    assert want_sizes >= {(1, 1), (2, 1), (1, 2), (3, 3), (7, 3), (8, 2), (9, 2)} | {(w, h) for w in (255, 256, 257) for h in (7, 8, 9)}
    assert (VC.OUT_TILE_W, VC.OUT_TILE_H) == (256, 8)
    for kind in VC.KINDS:
        mine = [c for c in cases if (c[4], c[7]) == kind]
        assert {(c[1], c[2]) for c in mine if c[3] is None} == want_sizes
        for size in want_sizes:
            assert {c[8] for c in mine if (c[1], c[2]) == size} == set(VC.LAYOUTS)
        assert {(c[5], c[6]) for c in mine} == set(ROWS)
        for p in range(len(VC.layouts(mine[0]))):  # both the wide and the element-by-element path store every plane, at the tile's sizes too
            assert {VC.wide_out(c, p) for c in mine if c[1] >= 255} == {True, False}, (kind, p)
        assert {c[3] for c in mine if c[3] is not None} == set(VC.RECTS)
    assert {VC.build_of(c[4], c[7]) for c in cases} == set(VC.BUILDS)
    assert all(not x & 1 for x, _, _, _ in VC.RECTS) and any(y & 1 and w & 1 and h & 1 for _, y, w, h in VC.RECTS)  # an even x; y, w and h odd


@pytest.fixture(scope="module")
def emulated_out(shim_out):
    cases = VC.out_cases()
    got, said = through_the_shim_out(shim_out, cases, "./emu")
    print(said.strip())
    return cases, got, said


def test_the_way_out_source_against_the_reference(emulated_out):
    """every plane of every case byte for byte, from the plane's pointer to its last row's end: what lies between a row's end and the pitch
    is still 0xEE; a rectangle's planes are the export of the cropped frame; 10-bit words have their six high bits zero"""
    cases, got, said = emulated_out
    for case, g in zip(cases, got):
        check_out(case, g)
        if REF.bits_of(case[4]) == 10:
            assert all(int(p.max()) < 1024 for p in VC.stored_of(g, case)), case[0]
    check_wide_counts(counts_of(said), cases, lambda c: (c[4], c[7]), VC.wide_out, extra="wide_src")


def test_the_way_out_shim_under_sanitizers(shim_out, emulated_out):
    """the stand-alone program built with -fsanitize=address,undefined on every case: a read past either end of the source, a store outside
    a plane that ends with its last row's end, a wide access at an address that is no multiple of its size, is an error there"""
    cases, _, _ = emulated_out
    got, _ = through_the_shim_out(shim_out, cases, "./emu_san")
    for case, g in zip(cases, got):
        check_out(case, g)
