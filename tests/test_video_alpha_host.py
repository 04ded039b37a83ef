"""Video with an alpha plane in and out (fdh_put_video_alpha, fdh_update_video_alpha, fdh_read_video_alpha, fdh_check_video_alpha_target;
include_video/figdraw_hip_video_alpha.h), what a CPU can check: the reference tests/video_alpha_ref.py against the siblings' references
and against exact arithmetic (fractions.Fraction), known answers by hand, the float64 bound of the straight way out; every refusal without
a device and through C99; and the sources of k_video_alpha_import.hip and k_video_alpha_export.hip under the host shim of tests/emu
(tests/video_alpha_in_emu, tests/video_alpha_out_emu) against the reference, byte for byte, padding included -- among the way out's
cases a 256 x 256 surface of every (colour, alpha) through every straight build: the exhaustive proof of the quotient."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import emu_build
import video_422_ref as V2
import video_frame_ref as SIB_IN
import video_planar_ref as PL
import video_alpha_cases as VC
import video_alpha_ref as REF
from conftest import ROOT
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext

INVALID = -1
ROWS = [(m, r) for m in (REF.BT601, REF.BT709, REF.BT2020) for r in (REF.LIMITED, REF.FULL)]
L, S = REF.CHROMA_LINEAR, REF.STRAIGHT_ALPHA
SIZES = ((1, 1), (2, 3), (5, 4), (9, 2), (33, 7))


def rules(fmt):
    return (0, L) if REF.linear_allowed(fmt) else (0,)


def noise_image(rng, w, h):
    """any bytes: colour above alpha among them; alpha 0 and 255 a quarter each"""
    img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
    kind = rng.integers(0, 4, size=(h, w))
    img[kind == 0, 3], img[kind == 1, 3] = 0, 255
    return img


def sibling_export(img, fmt, m, r, flags):
    ref, base = REF.BASE[fmt]
    return ref.export(img, base, m, r, flags)


def sibling_convert(stored, fmt, m, r, flags, w):
    ref, base = REF.BASE[fmt]
    return ref.convert(stored[:1], base, m, r, flags, w=w) if REF.packed(fmt) else ref.convert(stored[:3], base, m, r, flags)


# ------------------------------------------------------------------------------------------------------------------ 1. the reference
def test_the_premultiplied_way_out_is_the_sibling_export_and_the_alpha_bytes():
    rng = np.random.default_rng(51)
    for w, h in SIZES:
        img = noise_image(rng, w, h)
        for fmt in REF.FORMATS:
            for m, r in ROWS:
                for flags in rules(fmt):
                    got = REF.export(img, fmt, m, r, flags)
                    want = sibling_export(img, fmt, m, r, flags)
                    assert len(got) == len(want) + 1 and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want)), (w, h, fmt, m, r, flags)
                    assert got[-1].shape == (h, w) and got[-1].dtype == REF.dtype_of(fmt)
                    assert np.array_equal(got[-1], img[..., 3] if REF.bits_of(fmt) == 8 else (1023 * img[..., 3].astype(int) + 127) // 255)
    for fmt, sib in ((REF.A420, SIB_IN.NV12), (REF.A444, SIB_IN.NV12), (REF.A410, SIB_IN.P010), (REF.UYVA, SIB_IN.NV12)):
        for m, r in ROWS:  # an 8-bit format uses the NV12 row of either table, A410 the P010 row
            assert REF.in_coefficients(fmt, m, r) == context.video_coefficients(sib, m, r)
            assert REF.out_coefficients(fmt, m, r) == context.video_out_coefficients(sib, m, r)


def test_an_opaque_alpha_plane_on_the_way_in_is_the_sibling_under_both_flag_settings():
    rng = np.random.default_rng(52)
    for w, h in SIZES:
        for fmt in REF.FORMATS:
            stored = VC.noise_stored(rng, fmt, w, h)
            top = (1 << REF.bits_of(fmt)) - 1
            opaque = stored[:-1] + ((stored[-1] | REF.dtype_of(fmt)(top)),)  # (A410: garbage stays in the six high bits)
            for m, r in ROWS[::2]:
                for flags in rules(fmt):
                    want = sibling_convert(opaque, fmt, m, r, flags, w)
                    assert (want[..., 3] == 255).all()
                    for st in (0, S):
                        assert np.array_equal(REF.convert(opaque, fmt, m, r, flags | st, w=w), want), (w, h, fmt, m, r, flags, st)
                    # and any alpha: the sibling's colour, premultiplied or as converted, under the texel's own alpha byte
                    a = REF.alpha_in(stored[-1], fmt)
                    colour = sibling_convert(stored, fmt, m, r, flags, w)[..., :3]
                    pre, st = REF.convert(stored, fmt, m, r, flags, w=w), REF.convert(stored, fmt, m, r, flags | S, w=w)
                    assert np.array_equal(pre[..., :3], colour) and np.array_equal(pre[..., 3], a) and np.array_equal(st[..., 3], a)
                    assert np.array_equal(st[..., :3], colour.astype(int) * a[..., None].astype(int) // 255)


def test_an_opaque_frames_straight_export_is_its_premultiplied_export():
    rng = np.random.default_rng(53)
    for w, h in SIZES:
        img = noise_image(rng, w, h)
        img[..., 3] = 255
        for fmt in REF.FORMATS:
            for m, r in ROWS:
                for flags in rules(fmt):
                    a, b = REF.export(img, fmt, m, r, flags), REF.export(img, fmt, m, r, flags | S)
                    assert all(np.array_equal(x, y) for x, y in zip(a, b)), (w, h, fmt, m, r, flags)


def nearest(q: Fraction) -> int:
    """round half up"""
    return (2 * q.numerator + q.denominator) // (2 * q.denominator)


def test_the_alpha_depth_conversions_are_exact_and_8_10_8_is_the_identity():
    a8 = np.arange(256)
    a10 = REF.alpha_out(a8, REF.A410).astype(int)
    for a in range(256):
        q = Fraction(1023 * a, 255)
        assert abs(q - nearest(q)) < Fraction(1, 2) and a10[a] == nearest(q)  # to nearest, and no tie
    words = np.arange(1024, dtype=np.uint16)
    back = REF.alpha_in(words, REF.A410).astype(int)
    for a in range(1024):
        q = Fraction(255 * a, 1023)
        assert abs(q - nearest(q)) < Fraction(1, 2) and back[a] == nearest(q)
    assert np.array_equal(REF.alpha_in(REF.alpha_out(a8, REF.A410), REF.A410), a8)
    assert np.array_equal(REF.alpha_in((words | 0xFC00).astype(np.uint16), REF.A410), back)  # the six high bits are ignored
    assert (a10[0], a10[255], back[0], back[1023]) == (0, 1023, 0, 255)
    for fmt in (REF.A420, REF.A444, REF.UYVA):
        assert np.array_equal(REF.alpha_out(a8, fmt), a8) and np.array_equal(REF.alpha_in(a8.astype(np.uint8), fmt), a8)


def test_the_straight_byte_is_255_c_over_a_rounded_half_up_and_clamped_for_every_c_and_a():
    c, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    img = np.stack([c, c, c, a], axis=-1)
    u = REF.unpremultiplied(img, 1)
    assert u.shape == (256, 256, 3)
    want = np.zeros((256, 256), np.int64)
    for ai in range(1, 256):
        for ci in range(256):
            want[ci, ai] = min(255, nearest(Fraction(255 * ci, ai)))
    assert all(np.array_equal(u[..., k], want) for k in range(3))
    assert (u[:, 0] == 0).all() and (u[c > a] == np.where(a[c > a] == 0, 0, 255)[:, None]).all() and np.array_equal(u[:, 255, 0], np.arange(256))


def test_the_straight_sample_against_fractions_on_weighted_sets():
    """s for N = 2, 4, 8 on random weighted sets -- the siblings' weights: (1, 1), (1, 2, 1), 2 x 2 ones, (1, 2, 1) in two rows --, with
    sa = 0, sa = 1 and every c above its a among them"""
    rng = np.random.default_rng(54)
    weights = {2: (1, 1), 4: (1, 2, 1), 8: (1, 2, 1, 1, 2, 1)}
    weights4 = (1, 1, 1, 1)
    for n, wk in list(weights.items()) + [(4, weights4)]:
        assert sum(wk) == n
        texels = rng.integers(0, 256, size=(3000, len(wk), 4))
        texels[:300, :, 3] = 0                                      # sa = 0
        texels[300:600, :, 3] = 0
        texels[300:600, -1 if wk[-1] == 1 else 0, 3] = 1            # sa = 1: one texel of weight 1 with alpha 1
        texels[600:1200, :, 3] = np.minimum(texels[600:1200, :, 3], 254)
        texels[600:1200, :, :3] = np.maximum(texels[600:1200, :, :3], texels[600:1200, :, 3:] + 1).clip(0, 255)  # every c above its a
        texels[1200:1500, :, 3] = 255
        sums = (texels * np.array(wk)[None, :, None]).sum(axis=1)
        assert (sums[:300, 3] == 0).all() and (sums[300:600, 3] == 1).all()
        got = REF.unpremultiplied(sums, n)
        for i in range(len(sums)):
            sa = int(sums[i, 3])
            for k in range(3):
                want = 0 if sa == 0 else min(255 * n, nearest(Fraction(255 * n * int(sums[i, k]), sa)))
                assert got[i, k] == want, (n, i, k)
        assert (got[:300] == 0).all() and np.array_equal(got[1200:1500], sums[1200:1500, :3])
    assert 510 * 8 * 2040 + 2040 < 2 ** 24


def test_the_straight_way_out_against_float64_within_the_bound():
    """noise with every alpha, colour at or below it (a surface's promise where it holds) and above it: no sample of an 8-bit format is
    more than 1 from the rounded float64 value of the exactly un-premultiplied (weighted average) colour.  A410 is held to the same bound
    given the 8-bit straight colour, the header's stated limit: u lies within 1/2 byte of 255 c / a, and a byte is 1023 / 255 = 4.01
    ten-bit samples, so against the exactly un-premultiplied colour its samples lie within 0.5 * 4.01 + 0.032 < 2.04 before rounding --
    at most 3 apart once both are rounded -- which is asserted too."""
    rng = np.random.default_rng(55)
    img = rng.integers(0, 256, size=(64, 96, 4)).astype(np.uint8)
    img[::2, :, :3] = img[::2, :, :3].astype(int) * img[::2, :, 3:].astype(int) // 255
    img[:4, :, 3] = np.arange(96) * 2 % 256
    assert set(np.unique(img[..., 3])) == set(range(256))
    for fmt in REF.FORMATS:
        top = (1 << REF.bits_of(fmt)) - 1
        for m, r in ROWS:
            for flags in rules(fmt):
                y, cb, cr, _ = REF.export_planes(img, fmt, m, r, flags | S)
                ten = REF.bits_of(fmt) == 10
                for got, exact in zip((y, cb, cr), REF.export_float(img, fmt, m, r, flags, eight_bit_colour=ten)):
                    d = np.abs(got.astype(np.int64) - np.clip(np.rint(exact), 0, top).astype(np.int64))
                    assert got.shape == exact.shape and d.max() <= 1, (fmt, m, r, flags, int(d.max()))
                if ten:
                    for got, exact in zip((y, cb, cr), REF.export_float(img, fmt, m, r, flags)):
                        d = np.abs(got.astype(np.int64) - np.clip(np.rint(exact), 0, top).astype(np.int64))
                        assert d.max() <= 3, (fmt, m, r, flags, int(d.max()))


def one(r, g, b, a):
    return np.array([[[r, g, b, a]]], np.uint8)


def test_known_answers_for_one_texel_of_each_format():
    """BT.601 full range by hand.  kY = (4899, 9617, 1868), kU = (-2765, -5427, 8192), kV = (8192, -6860, -1332); N copies of one texel
    average to that texel, so A420 (N = 4) and UYVA (N = 2) give A444's samples.
    opaque white: Y = 255, Cb = Cr = 128, A = 255.
    half-transparent red, stored premultiplied as (128, 0, 0, 128):
      as stored: Y = (4899 * 128 + 8192) >> 14 = 635264 >> 14 = 38; Cb = 128 + ((-353920 + 8192) >> 14) = 128 - 22 = 106;
                 Cr = 128 + ((1048576 + 8192) >> 14) = 128 + 64 = 192
      straight:  u = min(255, (510 * 128 + 128) / 256) = min(255, 255) = 255 (255.5 floors), so pure red:
                 Y = (1249245 + 8192) >> 14 = 76; Cb = 128 + ((-705075 + 8192) >> 14) = 128 - 43 = 85; Cr = 128 + 128 = 256 -> 255
    transparent: Y = 0, Cb = Cr = 128, A = 0 in both modes, whatever colour bytes lie under alpha 0 in the straight one."""
    assert REF.out_coefficients(REF.A444, REF.BT601, REF.FULL) == (0, 128, 4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332)
    for fmt in (REF.A420, REF.A444, REF.UYVA):
        for flags in rules(fmt):
            def samples(img, st):
                return tuple(int(p[0, 0]) for p in REF.export_planes(img, fmt, REF.BT601, REF.FULL, flags | st))
            for st in (0, S):
                assert samples(one(255, 255, 255, 255), st) == (255, 128, 128, 255), (fmt, flags, st)
                assert samples(one(0, 0, 0, 0), st) == (0, 128, 128, 0), (fmt, flags, st)
            assert samples(one(128, 0, 0, 128), 0) == (38, 106, 192, 128), (fmt, flags)
            assert samples(one(128, 0, 0, 128), S) == (76, 85, 255, 128), (fmt, flags)
            assert samples(one(50, 60, 70, 0), S) == (0, 128, 128, 0), (fmt, flags)
            assert samples(one(50, 60, 70, 0), 0)[0] == (4899 * 50 + 9617 * 60 + 1868 * 70 + 8192) >> 14
    assert [p.tolist() for p in REF.export(one(128, 0, 0, 128), REF.UYVA, REF.BT601, REF.FULL, S)] == [[[85, 76, 255, 76]], [[128]]]
    assert [p.tolist() for p in REF.export(one(128, 0, 0, 128), REF.UYVA, REF.BT601, REF.FULL)] == [[[106, 38, 192, 38]], [[128]]]
    # A410: ten bits.  White: 1023, 512, 512, 1023; transparent: 0, 512, 512, 0; half-transparent red: a10 = (1023 * 128 + 127) / 255 = 514,
    # straight Y is 1023 * 0.299 = 305.9 and Cr clamps at 1023, as stored Y is 1023 * 0.299 * 128 / 255 = 153.5, each within 1
    for st in (0, S):
        assert [int(p[0, 0]) for p in REF.export(one(255, 255, 255, 255), REF.A410, REF.BT601, REF.FULL, st)] == [1023, 512, 512, 1023]
        assert [int(p[0, 0]) for p in REF.export(one(0, 0, 0, 0), REF.A410, REF.BT601, REF.FULL, st)] == [0, 512, 512, 0]
    y, cb, cr, a = (int(p[0, 0]) for p in REF.export(one(128, 0, 0, 128), REF.A410, REF.BT601, REF.FULL, S))
    assert abs(y - 305.9) <= 1 and cr == 1023 and a == 514 and abs(cb - (512 - 1023 * 0.299 / 1.772)) <= 1
    y, cb, cr, a = (int(p[0, 0]) for p in REF.export(one(128, 0, 0, 128), REF.A410, REF.BT601, REF.FULL))
    assert abs(y - 153.5) <= 1 and a == 514 and abs(cr - (512 + 1023 * 0.5 * 128 / 255)) <= 1
    # the way in, BT.601 full range: Y = 76, Cb = 85, Cr = 255 is red; under alpha 128 it is stored as converted, or premultiplied
    Y, cb, cr = (np.array([[v]], np.uint8) for v in (76, 85, 255))
    red = SIB_IN.yuv_to_rgba(Y, cb, cr, SIB_IN.NV12, REF.BT601, REF.FULL)[0, 0, :3].astype(int)
    assert red[0] >= 253 and red[1] <= 1 and red[2] <= 1
    for fmt, stored in ((REF.A444, (Y, cb, cr)), (REF.A420, (Y, cb, cr)), (REF.UYVA, (np.array([[85, 76, 255, 9]], np.uint8),))):
        a = np.array([[128]], np.uint8)
        assert REF.convert(stored + (a,), fmt, REF.BT601, REF.FULL, 0, w=1)[0, 0].tolist() == red.tolist() + [128]
        assert REF.convert(stored + (a,), fmt, REF.BT601, REF.FULL, S, w=1)[0, 0].tolist() == (red * 128 // 255).tolist() + [128]
        assert REF.convert(stored + (a * 0,), fmt, REF.BT601, REF.FULL, S, w=1)[0, 0].tolist() == [0, 0, 0, 0]
    a10 = np.array([[514 | 0xFC00]], np.uint16)
    grey = tuple(np.array([[512]], np.uint16) for _ in range(3))
    assert REF.convert(grey + (a10,), REF.A410, REF.BT601, REF.FULL, S)[0, 0, 3] == 128


# ------------------------------------------------------------------------------------------------------------------ 2. the rules
FW, FH = 16, 9
Y0, CB0, CR0, A0 = 0x10000, 0x20000, 0x30000, 0x40000


def target(**kw):
    """a valid A444 target for the whole of a 16 x 9 frame at made-up addresses (nothing is read or written without a device)"""
    base = dict(ptrs=(Y0, CB0, CR0, A0), pitches=(16, 16, 16, 16), format=REF.A444, matrix=REF.BT709, range=REF.LIMITED, flags=0, rect=None, reserved=(0, 0))
    base.update(kw)
    t = context.video_alpha_planes_target(base["ptrs"], base["pitches"], base["format"], base["matrix"], base["range"], base["flags"], base["rect"])
    t.reserved[0], t.reserved[1] = base["reserved"]
    return t


def frame(**kw):
    """the same as a source: 16 x 9 A444"""
    base = dict(ptrs=(Y0, CB0, CR0, A0), pitches=(16, 16, 16, 16), width=FW, height=FH, format=REF.A444, matrix=REF.BT709, range=REF.LIMITED, flags=0, reserved=(0, 0))
    base.update(kw)
    f = context.video_alpha_planes(base["ptrs"], base["width"], base["height"], base["pitches"], base["format"], base["matrix"], base["range"], base["flags"])
    f.reserved[0], f.reserved[1] = base["reserved"]
    return f


A420 = dict(format=REF.A420, pitches=(16, 8, 8, 16))
A410 = dict(format=REF.A410, pitches=(32, 32, 32, 32))
UYVA = dict(format=REF.UYVA, ptrs=(Y0, 0, 0, A0), pitches=(32, 0, 0, 16))


def multiple(p, unit="sample size"):
    return f"planes[{p}] and pitch_bytes[{p}] must be multiples of the {unit}"


def below(p):
    return f"pitch_bytes[{p}] is below a row's bytes"


IGNORE = "FDH_VIDEO_IGNORE_ALPHA is the sibling call: these formats carry an alpha plane"
LINEAR = "FDH_VIDEO_CHROMA_LINEAR is for A420 / UYVA: a 4:4:4 frame has a chroma sample per texel"
TWO_PLANES = "planes[1], planes[2] and their pitches must be 0 for UYVA: a UYVY plane and an alpha plane"
GROUP = "group size"
# (keywords one step from a valid struct, the text behind the call's name; None: the null text): the rules both directions share
SHARED = [
    (dict(ptrs=(0, CB0, CR0, A0)), None), (dict(ptrs=(Y0, 0, CR0, A0)), None), (dict(ptrs=(Y0, CB0, 0, A0)), None), (dict(ptrs=(Y0, CB0, CR0, 0)), None),
    (dict(A420, ptrs=(Y0, CB0, 0, A0)), None), (dict(A410, ptrs=(Y0, CB0, CR0, 0)), None),
    (dict(UYVA, ptrs=(0, 0, 0, A0)), None), (dict(UYVA, ptrs=(Y0, 0, 0, 0)), None),
    (dict(UYVA, ptrs=(Y0, CB0, 0, A0)), TWO_PLANES), (dict(UYVA, ptrs=(Y0, 0, CR0, A0)), TWO_PLANES), (dict(UYVA, pitches=(32, 8, 0, 16)), TWO_PLANES),
    (dict(UYVA, pitches=(32, 0, 8, 16)), TWO_PLANES),
] + [(dict(format=f), "unknown format") for f in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 15, 2 ** 31)] + [
    (dict(matrix=3), "unknown matrix"), (dict(range=2), "unknown range"), (dict(UYVA, matrix=7), "unknown matrix"),
    (dict(flags=8), "unknown flag"), (dict(flags=2 | 1 << 31), "unknown flag"), (dict(UYVA, flags=16), "unknown flag"),
    (dict(reserved=(7, 0)), "reserved must be 0"), (dict(reserved=(0, 1)), "reserved must be 0"), (dict(UYVA, reserved=(0, 1)), "reserved must be 0"),
    (dict(flags=REF.IGNORE_ALPHA), IGNORE), (dict(A420, flags=REF.IGNORE_ALPHA | L), IGNORE), (dict(UYVA, flags=REF.IGNORE_ALPHA | S), IGNORE),
    (dict(flags=L), LINEAR), (dict(A410, flags=L | S), LINEAR),
    (dict(A410, ptrs=(Y0 + 1, CB0, CR0, A0)), multiple(0)), (dict(A410, ptrs=(Y0, CB0 + 1, CR0, A0)), multiple(1)), (dict(A410, ptrs=(Y0, CB0, CR0 + 1, A0)), multiple(2)),
    (dict(A410, ptrs=(Y0, CB0, CR0, A0 + 1)), multiple(3)),
    (dict(A410, pitches=(33, 32, 32, 32)), multiple(0)), (dict(A410, pitches=(32, 32, 33, 32)), multiple(2)), (dict(A410, pitches=(32, 32, 32, 33)), multiple(3)),
    (dict(UYVA, ptrs=(Y0 + 2, 0, 0, A0)), multiple(0, GROUP)), (dict(UYVA, ptrs=(Y0 + 1, 0, 0, A0)), multiple(0, GROUP)), (dict(UYVA, pitches=(34, 0, 0, 16)), multiple(0, GROUP)),
    (dict(pitches=(15, 16, 16, 16)), below(0)), (dict(pitches=(-16, 16, 16, 16)), below(0)), (dict(pitches=(16, 15, 16, 16)), below(1)), (dict(pitches=(16, 16, 0, 16)), below(2)),
    (dict(pitches=(16, 16, 16, 15)), below(3)), (dict(A420, pitches=(16, 7, 8, 16)), below(1)), (dict(A420, pitches=(16, 8, 8, 8)), below(3)),
    (dict(A410, pitches=(30, 32, 32, 32)), below(0)), (dict(A410, pitches=(32, 32, 32, 30)), below(3)),
    (dict(UYVA, pitches=(28, 0, 0, 16)), below(0)), (dict(UYVA, pitches=(32, 0, 0, 15)), below(3)), (dict(UYVA, pitches=(0, 0, 0, 16)), below(0)),
]
OUTSIDE = "rectangle outside the frame"
EVEN_XY = "the rectangle's x and y must be even for A420"
EVEN_X = "the rectangle's x must be even for UYVA"
PLANE = 16 * (FH - 1) + 16  # a plane of the valid struct
TARGET_ONLY = [
    (dict(rect=(2, 0, 15, 9)), OUTSIDE), (dict(rect=(0, 2, 16, 8)), OUTSIDE), (dict(rect=(-2, 0, 4, 4)), OUTSIDE), (dict(rect=(0, -1, 4, 4)), OUTSIDE),
    (dict(rect=(16, 0, 1, 1)), OUTSIDE), (dict(UYVA, rect=(2, 1, 16, 8)), OUTSIDE), (dict(rect=(2, 2, 2 ** 31 - 1, 2)), OUTSIDE),
    (dict(A420, rect=(1, 0, 4, 4)), EVEN_XY), (dict(A420, rect=(0, 1, 4, 4)), EVEN_XY), (dict(A420, rect=(3, 3, 4, 4)), EVEN_XY),
    (dict(UYVA, rect=(7, 0, 2, 2)), EVEN_X), (dict(UYVA, rect=(15, 8, 1, 1)), EVEN_X),
    (dict(A420, rect=(0, 0, 15, 9), pitches=(16, 7, 8, 16)), below(1)),  # ceil(15 / 2) = 8 samples
    (dict(UYVA, rect=(0, 0, 15, 9), pitches=(28, 0, 0, 16)), below(0)),  # ... = 8 groups
    (dict(ptrs=(Y0, Y0, CR0, A0)), "planes 0 and 1 overlap"), (dict(ptrs=(Y0, CB0, Y0 + PLANE - 1, A0)), "planes 0 and 2 overlap"),
    (dict(ptrs=(Y0, CB0, CB0 + PLANE - 1, A0)), "planes 1 and 2 overlap"), (dict(ptrs=(Y0, CB0, CR0, Y0 + PLANE - 1)), "planes 0 and 3 overlap"),
    (dict(ptrs=(Y0, CB0, CR0, CB0)), "planes 1 and 3 overlap"), (dict(ptrs=(Y0, CB0, A0 + 1, A0)), "planes 2 and 3 overlap"),
    (dict(UYVA, ptrs=(Y0, 0, 0, Y0 + 32 * 9 - 1)), "planes 0 and 3 overlap"), (dict(A410, ptrs=(Y0, CB0, CR0, CR0 + 2 * PLANE - 2)), "planes 2 and 3 overlap"),
]
ACCEPTED = [
    dict(), A420, A410, UYVA, dict(flags=S), dict(A420, flags=L), dict(A420, flags=L | S), dict(A410, flags=S), dict(UYVA, flags=L), dict(UYVA, flags=L | S),
    dict(ptrs=(Y0, Y0 + PLANE, Y0 + 2 * PLANE, Y0 + 3 * PLANE)),  # the planes touch
    dict(UYVA, ptrs=(Y0, 0, 0, Y0 + 32 * 9)),                      # NDI's one block: the alpha plane right behind the UYVY plane
    dict(rect=(3, 3, 13, 5)), dict(A410, rect=(1, 1, 3, 3)), dict(A420, rect=(2, 4, 13, 5)), dict(UYVA, rect=(2, 3, 13, 5)),  # odd w and h; odd x and y where allowed
    dict(rect=(0, 0, 0, 5)), dict(A420, rect=(7, 7, -1, 0)), dict(UYVA, rect=(3, 3, 0, 0)),  # (w or h <= 0: the whole frame)
    dict(UYVA, rect=(2, 3, 13, 5), pitches=(28, 0, 0, 13)), dict(A420, rect=(14, 8, 1, 1), pitches=(1, 1, 1, 1)), dict(A410, rect=(2, 1, 3, 3), pitches=(6, 6, 6, 6)),
    dict(ptrs=(Y0 + 1, CB0 + 3, CR0 + 5, A0 + 7), pitches=(17, 19, 21, 23)), dict(A410, ptrs=(Y0 + 2, CB0 + 6, CR0 + 10, A0 + 14), pitches=(34, 38, 42, 46)),
    dict(UYVA, ptrs=(Y0 + 4, 0, 0, A0 + 1), pitches=(36, 0, 0, 17)),
]


def test_check_video_alpha_target_applies_every_rule():
    Lb = context.load()
    for i, kw in enumerate(ACCEPTED):
        t = target(**kw)
        assert Lb.fdh_check_video_alpha_target(C.byref(t), FW, FH) == 0, (i, Lb.fdh_last_error().decode())
        context.check_video_alpha_target(t, FW, FH)
    for i, (kw, text) in enumerate(SHARED + TARGET_ONLY):
        t = target(**kw)
        assert Lb.fdh_check_video_alpha_target(C.byref(t), FW, FH) == INVALID, (i, kw)
        assert Lb.fdh_last_error().decode() == f"check_video_alpha_target: {text or 'null target or plane'}", (i, kw)
    assert Lb.fdh_check_video_alpha_target(None, FW, FH) == INVALID and Lb.fdh_last_error().decode() == "check_video_alpha_target: null target or plane"
    for fw, fh in ((0, 9), (16, 0), (-1, -1)):
        assert Lb.fdh_check_video_alpha_target(C.byref(target()), fw, fh) == INVALID and Lb.fdh_last_error().decode() == "check_video_alpha_target: empty frame"
    with pytest.raises(FigdrawHipError) as e:
        context.check_video_alpha_target(target(format=6), FW, FH)
    assert e.value.code == INVALID and str(e.value).endswith("check_video_alpha_target: unknown format")


def packed_area(ctx):
    area = C.c_int64()
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(area)) == 0
    return area.value


def test_refusals_on_the_way_in_leave_directory_packer_and_epoch_untouched():
    ctx = HipContext(atlas_size=256, record_only=True)
    Lb = ctx.L
    assert ctx.put_video_alpha(7, (Y0, CB0, CR0, A0), FW, FH, (16, 16, 16, 16), format=REF.A444)[2:] == (FW, FH)
    out = (C.c_int * 4)()
    before = (ctx.atlas_usage(), packed_area(ctx))
    refused = [(frame(**kw), text or "null frame or plane") for kw, text in SHARED] + [
        (None, "null frame or plane"), (frame(width=0), "empty frame"), (frame(height=-2), "empty frame"), (frame(**dict(UYVA, width=-1)), "empty frame"),
        (frame(**dict(A420, width=15, pitches=(15, 7, 8, 15))), below(1)), (frame(**dict(UYVA, width=15, pitches=(28, 0, 0, 15))), below(0))]
    for i, (f, text) in enumerate(refused):
        ref = C.byref(f) if f is not None else None
        for name, call in (("put_video_alpha", lambda: Lb.fdh_put_video_alpha(ctx.h, 9, ref, out)), ("update_video_alpha", lambda: Lb.fdh_update_video_alpha(ctx.h, 7, ref))):
            assert call() == INVALID, (i, name)
            assert Lb.fdh_last_error().decode() == f"{name}: {text}", (i, name)
            assert (ctx.atlas_usage(), packed_area(ctx)) == before and not ctx.has_image(9), (i, name)
    assert Lb.fdh_update_video_alpha(ctx.h, 9, C.byref(frame())) == INVALID and Lb.fdh_last_error().decode() == "update_video_alpha: unknown key"
    for f in (frame(width=15), frame(height=10), frame(**dict(UYVA, width=8))):
        assert Lb.fdh_update_video_alpha(ctx.h, 7, C.byref(f)) == INVALID and Lb.fdh_last_error().decode() == "update_video_alpha: size mismatch"
    assert (ctx.atlas_usage(), packed_area(ctx)) == before
    # the four older families keep refusing every format value from 11 on
    for fmt in REF.FORMATS:
        old = context.video_frame(Y0, CB0, FW, FH, 16, 16, fmt)
        planes = context.video_planes((Y0, CB0, CR0), FW, FH, (16, 16, 16), fmt)
        planes_target = context.video_planes_target((Y0, CB0, CR0), (16, 16, 16), fmt)
        assert Lb.fdh_put_video_frame(ctx.h, 9, C.byref(old), out) == INVALID and Lb.fdh_last_error().decode() == "put_video_frame: unknown format"
        assert Lb.fdh_update_video_frame(ctx.h, 7, C.byref(old)) == INVALID and Lb.fdh_last_error().decode() == "update_video_frame: unknown format"
        assert Lb.fdh_check_video_target(C.byref(context.video_target(Y0, CB0, 16, 16, format=fmt)), FW, FH) == INVALID
        assert Lb.fdh_put_video_planes(ctx.h, 9, C.byref(planes), out) == INVALID and Lb.fdh_last_error().decode() == "put_video_planes: unknown format"
        assert Lb.fdh_update_video_planes(ctx.h, 7, C.byref(planes)) == INVALID and Lb.fdh_last_error().decode() == "update_video_planes: unknown format"
        assert Lb.fdh_check_video_planes_target(C.byref(planes_target), FW, FH) == INVALID and Lb.fdh_last_error().decode() == "check_video_planes_target: unknown format"
        assert Lb.fdh_put_video_422(ctx.h, 9, C.byref(planes), out) == INVALID and Lb.fdh_last_error().decode() == "put_video_422: unknown format"
        assert Lb.fdh_update_video_422(ctx.h, 7, C.byref(planes)) == INVALID and Lb.fdh_last_error().decode() == "update_video_422: unknown format"
        assert Lb.fdh_check_video_422_target(C.byref(planes_target), FW, FH) == INVALID and Lb.fdh_last_error().decode() == "check_video_422_target: unknown format"
    assert (ctx.atlas_usage(), packed_area(ctx)) == before and not ctx.has_image(9)
    # a call that goes through moves the epoch, and a put the packer too; the planes may alias each other on the way in; the next frame may
    # come in another of the four formats
    ctx.update_video_alpha(7, (Y0, Y0, Y0, Y0), FW, FH, (32, 32, 32, 32), format=REF.A410, matrix=REF.BT2020, range=REF.FULL, flags=S)
    ctx.update_video_alpha(7, (Y0, 0, 0, Y0), FW, FH, (32, 0, 0, 16), format=REF.UYVA)
    after = ctx.atlas_usage()
    assert after["epoch"] == before[0]["epoch"] + 2 and packed_area(ctx) == before[1]
    assert ctx.put_video_alpha(9, (Y0 + 4, 0, 0, A0 + 1), 15, 9, (36, 0, 0, 17), format=REF.UYVA, flags=L | S)[2:] == (15, 9)
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
    assert ctx.L.fdh_read_video_alpha(ctx.h, C.byref(target())) == INVALID
    assert ctx.L.fdh_last_error().decode().startswith("read_video_alpha: ")
    with pytest.raises(FigdrawHipError):
        ctx.read_video_alpha((Y0, 0, 0, A0), (32, 0, 0, 16), format=REF.UYVA)
    assert ctx.L.fdh_read_video_alpha(None, C.byref(target())) == INVALID
    ctx.close()


def test_the_format_values():
    assert (context.VIDEO_A420, context.VIDEO_A444, context.VIDEO_A410, context.VIDEO_UYVA) == (11, 12, 13, 14) == REF.FORMATS
    assert C.sizeof(context.VideoAlphaPlanes) == 96 and C.sizeof(context.VideoAlphaPlanesTarget) == 104


def test_video_alpha_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "video_alpha_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_video"),
                           os.path.join(ROOT, "tests", "video_alpha_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "video_alpha_abi_smoke: OK" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ 3. the way in's source
@pytest.fixture(scope="module")
def shim_in(tmp_path_factory):
    """k_video_alpha_import.hip (and k_image_import.hip, for the tail) compiled as plain C++ under the sequential shim of tests/emu with the
    driver of tests/video_alpha_in_emu -> the directory of ./emu and ./emu_san: the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "video_alpha_in_emu", ("k_video_alpha_import.hip", "fdh_video_alpha.h", "fdh_video_import.h", "k_image_import.hip", "fdh_image_import.h"),
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
            packed = VC.four_of(case[1], VC.pack(case), nothing=(b"", 0, 0))
            x, y, size, n_levels = place_of(i, w, h)
            places.append((x, y, size, n_levels))
            f.write(np.array([w, h, case[1], case[2], case[3], case[4], *(p[2] for p in packed), *(p[1] for p in packed), *(len(p[0]) for p in packed), x, y, size, n_levels, 0, 0], np.int32).tobytes())
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


def check_wide_counts(counts, cases, kind_of, wide, extra=None):
    """what the program counted per build and plane is the host rule's prediction, and every build took both paths on every plane it has"""
    assert counts["cases"] == len(cases)
    for build in VC.BUILDS:
        b, mine = VC.build_index(*build), [c for c in cases if kind_of(c) == build]
        assert counts[f"b{b}_cases"] == len(mine) > 0, build
        for p in range(4):
            has = p in VC.plane_ids(build[0])
            want = sum(wide(c, p) for c in mine) if has else 0
            assert counts[f"b{b}_wide_{p}"] == want, (build, p)
            if has:
                assert 0 < want < len(mine), (build, p)
        if extra:
            assert 0 < counts[f"b{b}_{extra}"] < len(mine), (build, extra)
    assert sorted(VC.build_index(*b) for b in VC.BUILDS) == list(range(12))


@pytest.fixture(scope="module")
def emulated_in(shim_in):
    cases = VC.in_cases()
    got, said = through_the_shim_in(shim_in, cases)
    print(said.strip())
    return cases, got, said


def test_the_cases_cover_the_ground():
    """every one of the 24 builds -- twelve each way -- is met by a case with a cut run, by one with a whole wide run, and by one in an
    element-by-element layout; every straight case of three texels or more holds alpha 0, alpha 255 and alphas in between"""
    assert len(VC.KINDS) == len(set(VC.KINDS)) == 12
    assert {k for k in VC.KINDS} == {(f, fl | st) for f in (REF.A420, REF.UYVA) for fl in (0, L) for st in (0, S)} | {(f, st) for f in (REF.A444, REF.A410) for st in (0, S)}
    cases = VC.in_cases()
    assert len({c[0] for c in cases}) == len(cases)
    assert {(c[1], c[4], c[2], c[3]) for c in cases} == {(f, fl, m, r) for f, fl in VC.KINDS for m, r in ROWS}  # every build meets every row
    for size in VC.IN_SIZES + [VC.IN_LARGEST]:
        assert {c[6] for c in cases if VC.size_of(c) == size} >= {"tight", "padded"}, size
    assert {(7, 5), (8, 8), (9, 3), (31, 33), (33, 31), (1, 1)} <= set(VC.IN_SIZES)  # the run of eight +- 1, the tile +- 1
    for kind in VC.KINDS:
        mine = [c for c in cases if (c[1], c[4]) == kind]
        ids = VC.plane_ids(kind[0])
        assert any(VC.size_of(c)[0] % VC.RUN for c in mine), kind                                                             # a cut run
        assert any(c[6] == "aligned" and all(VC.wide_in(c, p) for p in ids) for c in mine), kind                               # a whole wide run
        assert any(not any(VC.wide_in(c, p) for p in ids) for c in mine if VC.size_of(c)[0] >= 16), kind                       # element by element
        for c in mine:
            a = REF.alpha_in(c[5][-1], c[1])
            if a.size >= 16:
                assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any(), c[0]
    ten = [c for c in cases if REF.bits_of(c[1]) == 10]
    assert ten and all((c[5][p] >> 10).any() for c in ten for p in range(4) if c[5][p].size > 8)  # garbage in the six high bits, alpha too
    assert any(VC.size_of(c)[0] & 1 for c in cases if REF.packed(c[1]))  # an odd width's last group, with noise in its second luma byte
    out = VC.out_cases()
    assert len({c[0] for c in out}) == len(out)
    for kind in VC.KINDS:
        fmt = kind[0]
        mine = [c for c in out if (c[4], c[7]) == kind]
        want_sizes = set(VC.out_sizes(fmt))
        t = VC.out_tile_h(fmt)
        assert want_sizes >= {(1, 1), (2, 1), (1, 2), (3, 3), (7, 3), (8, 2), (9, 2)} | {(w, h) for w in (255, 256, 257) for h in (t - 1, t, t + 1)}
        assert {(c[1], c[2]) for c in mine if c[3] is None} == want_sizes
        for size in want_sizes:
            assert {c[8] for c in mine if (c[1], c[2]) == size} == set(VC.LAYOUTS)
        assert {(c[5], c[6]) for c in mine} == set(ROWS)
        for p in VC.plane_ids(fmt):  # both the wide and the element-by-element path store every plane, at the tile's sizes too
            assert {VC.wide_out(c, p) for c in mine if c[1] >= 255} == {True, False}, (kind, p)
        assert any(VC.rect_of(c)[2] % VC.RUN for c in mine)  # a cut run
        assert {c[3] for c in mine if c[3] is not None} == set(VC.rects(fmt))
        if kind[1] & S:
            for c in mine:
                a = VC.cropped(VC.source(c[1], c[2]), VC.rect_of(c))[..., 3]
                if c[3] is None and a.size >= 3:
                    assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any(), c[0]
    assert (VC.OUT_TILE_W, VC.out_tile_h(REF.A420), VC.out_tile_h(REF.UYVA)) == (256, 16, 8)
    assert all(not (x | y) & 1 for x, y, _, _ in VC.rects(REF.A420)) and all(not x & 1 for x, _, _, _ in VC.rects(REF.UYVA))
    assert any(y & 1 for _, y, _, _ in VC.rects(REF.UYVA)) and any(x & 1 and y & 1 for x, y, _, _ in VC.rects(REF.A444))
    src = VC.source(9, 2)
    assert (src[..., :3].max(axis=2) > src[..., 3]).any()  # a colour byte above its alpha: what a rendered frame cannot promise


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


def test_the_way_in_of_opaque_frames_is_the_siblings_texels():
    """the cases with their alpha planes all 255 / 1023: the reference's texels are the sibling reference's, under the case's flags"""
    for case in VC.in_cases(largest=False):
        o = VC.opaque(case)
        want = sibling_convert(o[5], o[1], o[2], o[3], o[4] & L, o[7])
        assert np.array_equal(REF.convert(o[5], o[1], o[2], o[3], o[4], w=o[7]), want), o[0]


# ------------------------------------------------------------------------------------------------------------------ 4. the way out's source
@pytest.fixture(scope="module")
def shim_out(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "video_alpha_out_emu", ("k_video_alpha_export.hip", "fdh_video_alpha.h", "fdh_video_export.h", "fdh_image_import.h"),
                           {"emu": (), "emu_san": emu_build.SAN}, opt="-O2")


def through_the_shim_out(tmp, cases, exe, frames=None):
    """-> per case the planes' bytes as the program left them, and what it printed.  frames: per case its source, VC.source by default"""
    with open(os.path.join(tmp, "cases.bin"), "wb") as f:
        for i, case in enumerate(cases):
            _, W, H, _, fmt, m, r, flags, _ = case
            lay = VC.four_of(fmt, VC.layouts(case), nothing=(0, 0, 0, 0))
            f.write(np.array([W, H, *VC.rect_of(case), fmt, m, r, flags, *(l[1] for l in lay), *(l[0] for l in lay)], np.int32).tobytes())
            f.write((VC.source(W, H) if frames is None else frames[i]).tobytes())
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


def check_out(case, got, frame=None):
    want = VC.expected_planes(case, frame)
    assert len(got) == len(want) == len(VC.plane_ids(case[4])), case[0]
    for p, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (case[0], p)
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{case[0]}: plane {VC.plane_ids(case[4])[p]} differs in {int((a != b).sum())} bytes, the first at {at} (pitch {VC.layouts(case)[p][1]}): {a[at]} != {b[at]}")


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


def test_every_colour_and_alpha_through_every_straight_build(shim_out):
    """the exhaustive proof of the quotient: the 256 x 256 surface whose texel (c, a) holds colour c and alpha a -- c above a included --
    through the six straight builds, byte for byte against the reference, whose own quotient the tests above hold to Fraction; under the
    sanitizers too.  Luma is strictly increasing in the straight byte in the full range, so every u shows in a sample."""
    surface = VC.quotient_surface()
    cases = [(f"every (c, a) {REF.NAMES[fmt]} f{flags} {layout}", 256, 256, None, fmt, REF.BT709, REF.FULL, flags, layout)
             for fmt, flags in VC.KINDS if flags & S for layout in ("tight", "padded")]
    assert len(cases) == 12
    k = REF.out_coefficients(REF.A444, REF.BT709, REF.FULL)
    grey = (sum(k[2:5]) * np.arange(256) + 8192) >> 14
    assert (np.diff(grey) > 0).all()
    for exe in ("./emu", "./emu_san"):
        got, _ = through_the_shim_out(shim_out, cases, exe, frames=[surface] * len(cases))
        for case, g in zip(cases, got):
            check_out(case, g, frame=surface)
    # and what that export holds: row a, column c of the A444 luma plane is the luma of grey min(255, round(255 c / a))
    y = REF.export(surface, REF.A444, REF.BT709, REF.FULL, S)[0].astype(int)
    for a in (1, 2, 127, 128, 254, 255):
        u = np.minimum(255, (510 * np.arange(256) + a) // (2 * a))
        assert np.array_equal(y[a], grey[u]), a
    assert (y[0] == 0).all()
