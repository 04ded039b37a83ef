"""The order of the refusals of the four video export calls, without a device (fdh_check_video_target, fdh_check_video_planes_target,
fdh_check_video_422_target, fdh_check_video_alpha_target; figdraw_amd/csrc/fdh_video_out.cpp): targets that break TWO rules at once, and
which of the two is reported.  The tables of test_video_out_host.py, test_video_planar_host.py, test_video_422_host.py and
test_video_alpha_host.py pin every text one step from a valid target; this pins the order the steps are asked in:

  1 null target or plane, 2 format, 3 matrix, 4 range, 5 unknown flag, 6 reserved, 7 the family's flag rules, 8 its plane-count rules
  (BGRA8's "one plane", a packed format's zero planes, a planar format's null planes behind them), 9 "empty frame", 10 the rectangle
  outside, 11 evenness, 12 per plane in plane order the element multiple, then the pitch, 13 the overlaps, lowest pair first.

The 16 x 9 frame and the made-up addresses of those tests: nothing is read or written."""
import ctypes as C

from figdraw_amd import context
from figdraw_amd.context import (VIDEO_A410, VIDEO_A420, VIDEO_A444, VIDEO_BGRA8, VIDEO_BT709, VIDEO_CHROMA_LINEAR, VIDEO_I010, VIDEO_I420, VIDEO_I444,
                                 VIDEO_I210, VIDEO_I422, VIDEO_IGNORE_ALPHA, VIDEO_LIMITED, VIDEO_NV12, VIDEO_P010, VIDEO_STRAIGHT_ALPHA, VIDEO_UYVA, VIDEO_YUY2)

INVALID = -1
FW, FH = 16, 9
Y0, CB0, CR0, A0 = 0x10000, 0x20000, 0x30000, 0x40000
LUMA = 16 * 9  # the bytes of an 8-bit luma (or alpha, or 4:4:4 chroma) plane of the frame, rows packed

OUTSIDE = "rectangle outside the frame"
EMPTY = "empty frame"
NULL = "null target or plane"
RESERVED = "reserved must be 0"
ALPHA_FLAGS = "the alpha flags are BGRA8's"


def multiple(p, unit="the sample size"):
    return f"planes[{p}] and pitch_bytes[{p}] must be multiples of {unit}"


def below(p):
    return f"pitch_bytes[{p}] is below a row's bytes"


def overlap(p, q):
    return f"planes {p} and {q} overlap"


def filled(t, kw):
    t.reserved[0], t.reserved[1] = kw["reserved"]
    return t


def frame_target(kw):
    return filled(context.video_target(kw["y"], kw["uv"], kw["pitch_y"], kw["pitch_uv"], kw["format"], kw["matrix"], kw["range"], kw["flags"], kw["rect"]), kw)


def planes_target(kw):
    return filled(context.video_planes_target(kw["ptrs"], kw["pitches"], kw["format"], kw["matrix"], kw["range"], kw["flags"], kw["rect"]), kw)


def alpha_target(kw):
    return filled(context.video_alpha_planes_target(kw["ptrs"], kw["pitches"], kw["format"], kw["matrix"], kw["range"], kw["flags"], kw["rect"]), kw)


COMMON = dict(matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0, rect=None, reserved=(0, 0), frame=(FW, FH))


def run(call, make, valid, cases):
    """every case is keywords over `valid` that break two rules (frame=: the frame's size, for "empty frame") and the text that wins"""
    L = context.load()
    check = getattr(L, "fdh_" + call)
    assert check(C.byref(make(dict(COMMON, **valid))), FW, FH) == 0, L.fdh_last_error().decode()
    for i, (kw, text) in enumerate(cases):
        kw = dict(COMMON, **dict(valid, **kw))
        assert check(C.byref(make(kw)), *kw["frame"]) == INVALID, (i, kw)
        assert L.fdh_last_error().decode() == f"{call}: {text}", (i, kw)


# ------------------------------------------------------------------------------------------------------------------ NV12, P010, BGRA8
NV12 = dict(y=Y0, uv=CB0, pitch_y=16, pitch_uv=16, format=VIDEO_NV12)
P010 = dict(format=VIDEO_P010, pitch_y=32, pitch_uv=32)
BGRA = dict(format=VIDEO_BGRA8, uv=0, pitch_y=64, pitch_uv=0, matrix=0, range=0)
STRAIGHT = "FDH_VIDEO_STRAIGHT_ALPHA is for the way in: the surface's bytes go out as stored"
IGNORE_IS_BGRAS = "FDH_VIDEO_IGNORE_ALPHA is BGRA8's"
ONE_PLANE = "BGRA8 has one plane"
NEEDS_CHROMA = "FDH_VIDEO_CHROMA_LINEAR needs a chroma plane"
EVEN = "the rectangle's x and y must be even for NV12 / P010"
ELEMENT0 = "planes[0] and pitch_bytes[0] must be multiples of the element size"
ELEMENT1 = "planes[1] and pitch_bytes[1] must be multiples of a pair's size"
FRAME_CASES = [
    (dict(y=0, format=99), "null target"),                                        # 1 | 2
    (dict(format=99, matrix=3), "unknown format"),                                # 2 | 3
    (dict(matrix=3, range=2), "unknown matrix"),                                  # 3 | 4
    (dict(range=2, flags=8), "unknown range"),                                    # 4 | 5
    (dict(flags=8, reserved=(1, 0)), "unknown flag"),                             # 5 | 6
    (dict(reserved=(0, 1), flags=VIDEO_STRAIGHT_ALPHA), RESERVED),                # 6 | 7
    (dict(flags=VIDEO_STRAIGHT_ALPHA, uv=0), STRAIGHT),                           # 7 | 8
    (dict(BGRA, flags=VIDEO_STRAIGHT_ALPHA, uv=CB0), STRAIGHT),
    (dict(BGRA, flags=VIDEO_STRAIGHT_ALPHA, matrix=1), STRAIGHT),
    (dict(BGRA, matrix=1, uv=CB0), "matrix and range must be 0 for BGRA8"),       # BGRA8's rules among themselves: matrix and range,
    (dict(BGRA, uv=CB0, flags=VIDEO_CHROMA_LINEAR), ONE_PLANE),                   # ... one plane, the chroma flag
    (dict(uv=0, flags=VIDEO_IGNORE_ALPHA), "null chroma plane"),                  # NV12's: the chroma plane, the alpha flag
    (dict(uv=0, frame=(0, 9)), "null chroma plane"),                              # 8 | 9
    (dict(flags=VIDEO_IGNORE_ALPHA, frame=(16, 0)), IGNORE_IS_BGRAS),
    (dict(BGRA, pitch_uv=16, frame=(0, 0)), ONE_PLANE),
    (dict(BGRA, flags=VIDEO_CHROMA_LINEAR, frame=(-1, 9)), NEEDS_CHROMA),
    (dict(frame=(0, 9), rect=(0, 0, 4, 4)), EMPTY),                               # 9 | 10
    (dict(rect=(1, 0, 16, 9)), OUTSIDE),                                          # 10 | 11
    (dict(rect=(2, 3, 15, 6)), OUTSIDE),
    (dict(rect=(1, 0, 4, 4), pitch_y=3), EVEN),                                   # 11 | 12
    (dict(P010, rect=(0, 1, 4, 4), y=Y0 + 1), EVEN),
    (dict(P010, pitch_y=31), ELEMENT0),                                           # 12: the multiple before the pitch
    (dict(BGRA, pitch_y=62), ELEMENT0),
    (dict(pitch_uv=13), ELEMENT1),
    (dict(pitch_y=15, uv=CB0 + 1), below(0)),                                     # 12: plane 0's pitch before plane 1's multiple
    (dict(P010, pitch_y=30, uv=CB0 + 2), below(0)),
    (dict(P010, y=Y0 + 1, pitch_uv=28), ELEMENT0),
    (dict(uv=Y0, pitch_uv=14), below(1)),                                         # 12 | 13
    (dict(P010, uv=Y0 + 2), ELEMENT1),
]


def test_the_order_of_check_video_target():
    run("check_video_target", frame_target, NV12, FRAME_CASES)


# ------------------------------------------------------------------------------------------------------------------ I420, I010, I444, I410
I420 = dict(ptrs=(Y0, CB0, CR0), pitches=(16, 8, 8), format=VIDEO_I420)
I010 = dict(format=VIDEO_I010, pitches=(32, 16, 16))
I444 = dict(format=VIDEO_I444, pitches=(16, 16, 16))
LINEAR_IS_420S = "FDH_VIDEO_CHROMA_LINEAR is for I420 / I010: a 4:4:4 frame has a chroma sample per texel"
EVEN_420 = "the rectangle's x and y must be even for I420 / I010"
PLANAR_CASES = [
    (dict(ptrs=(Y0, CB0, 0), format=0), NULL),                                    # 1 | 2
    (dict(ptrs=(Y0, 0, CR0), matrix=3), NULL),
    (dict(format=7, matrix=3), "unknown format"),                                 # 2 | 3
    (dict(matrix=3, range=2), "unknown matrix"),                                  # 3 | 4
    (dict(range=2, flags=8), "unknown range"),                                    # 4 | 5
    (dict(flags=8, reserved=(1, 0)), "unknown flag"),                             # 5 | 6
    (dict(reserved=(0, 1), flags=VIDEO_STRAIGHT_ALPHA), RESERVED),                # 6 | 7
    (dict(I444, flags=VIDEO_IGNORE_ALPHA | VIDEO_CHROMA_LINEAR), ALPHA_FLAGS),    # 7: the alpha flags before the chroma flag
    (dict(flags=VIDEO_STRAIGHT_ALPHA, frame=(0, 9)), ALPHA_FLAGS),                # 7 | 9 (the family has no plane-count rule)
    (dict(I444, flags=VIDEO_CHROMA_LINEAR, frame=(16, 0)), LINEAR_IS_420S),
    (dict(frame=(0, 9), rect=(0, 0, 4, 4)), EMPTY),                               # 9 | 10
    (dict(rect=(1, 0, 16, 9)), OUTSIDE),                                          # 10 | 11
    (dict(rect=(1, 0, 4, 4), pitches=(3, 8, 8)), EVEN_420),                       # 11 | 12
    (dict(I010, rect=(0, 1, 4, 4), ptrs=(Y0 + 1, CB0, CR0)), EVEN_420),
    (dict(I010, pitches=(31, 16, 16)), multiple(0)),                              # 12: the multiple before the pitch
    (dict(I010, pitches=(32, 16, 13)), multiple(2)),
    (dict(I010, pitches=(30, 16, 16), ptrs=(Y0, CB0 + 1, CR0)), below(0)),        # 12: plane 0's pitch before plane 1's multiple
    (dict(I010, pitches=(32, 14, 16), ptrs=(Y0, CB0, CR0 + 1)), below(1)),
    (dict(I010, pitches=(32, 16, 14), ptrs=(Y0, CB0 + 1, CR0)), multiple(1)),
    (dict(ptrs=(Y0, Y0, CR0), pitches=(16, 8, 7)), below(2)),                     # 12 | 13
    (dict(ptrs=(Y0, Y0, Y0)), overlap(0, 1)),                                     # 13: the lowest pair first
    (dict(ptrs=(Y0, Y0 + LUMA, Y0 + LUMA - 4)), overlap(0, 2)),                   # (planes 0 and 1 touch; plane 2 lies over both)
]


def test_the_order_of_check_video_planes_target():
    run("check_video_planes_target", planes_target, I420, PLANAR_CASES)


# ------------------------------------------------------------------------------------------------------------------ I422, I210, YUY2, UYVY
I422 = dict(ptrs=(Y0, CB0, CR0), pitches=(16, 8, 8), format=VIDEO_I422)
I210 = dict(format=VIDEO_I210, pitches=(32, 16, 16))
YUY2 = dict(format=VIDEO_YUY2, ptrs=(Y0, 0, 0), pitches=(32, 0, 0))
ONE_PLANE_422 = "planes[1], planes[2] and their pitches must be 0 for YUY2 / UYVY: one plane"
EVEN_422 = "the rectangle's x must be even for 4:2:2"
GROUP = "the group size"
CASES_422 = [
    (dict(ptrs=(0, CB0, CR0), format=0), NULL),                                   # 1 | 2
    (dict(ptrs=(Y0, 0, CR0), format=0), "unknown format"),                        # (planes 1 and 2 are step 8's: the format says whether they are there)
    (dict(format=6, matrix=3), "unknown format"),                                 # 2 | 3
    (dict(matrix=3, range=2), "unknown matrix"),                                  # 3 | 4
    (dict(range=2, flags=8), "unknown range"),                                    # 4 | 5
    (dict(flags=8, reserved=(1, 0)), "unknown flag"),                             # 5 | 6
    (dict(reserved=(0, 1), flags=VIDEO_STRAIGHT_ALPHA), RESERVED),                # 6 | 7
    (dict(YUY2, flags=VIDEO_IGNORE_ALPHA, ptrs=(Y0, CB0, 0)), ALPHA_FLAGS),       # 7 | 8
    (dict(flags=VIDEO_STRAIGHT_ALPHA, ptrs=(Y0, 0, CR0)), ALPHA_FLAGS),
    (dict(YUY2, pitches=(32, 0, 8), frame=(0, 9)), ONE_PLANE_422),                # 8 | 9
    (dict(ptrs=(Y0, CB0, 0), frame=(16, 0)), NULL),
    (dict(frame=(0, 9), rect=(0, 0, 4, 4)), EMPTY),                               # 9 | 10
    (dict(rect=(1, 0, 16, 9)), OUTSIDE),                                          # 10 | 11
    (dict(YUY2, rect=(3, 2, 14, 8)), OUTSIDE),
    (dict(rect=(1, 0, 4, 4), pitches=(3, 8, 8)), EVEN_422),                       # 11 | 12
    (dict(YUY2, rect=(1, 0, 4, 4), ptrs=(Y0 + 2, 0, 0)), EVEN_422),
    (dict(I210, pitches=(31, 16, 16)), multiple(0)),                              # 12: the multiple before the pitch
    (dict(YUY2, pitches=(30, 0, 0)), multiple(0, GROUP)),
    (dict(I210, pitches=(30, 16, 16), ptrs=(Y0, CB0 + 1, CR0)), below(0)),        # 12: plane 0's pitch before plane 1's multiple
    (dict(I210, pitches=(32, 14, 16), ptrs=(Y0, CB0, CR0 + 1)), below(1)),
    (dict(I210, pitches=(32, 16, 14), ptrs=(Y0, CB0 + 1, CR0)), multiple(1)),
    (dict(ptrs=(Y0, Y0, CR0), pitches=(16, 8, 7)), below(2)),                     # 12 | 13
    (dict(ptrs=(Y0, Y0, Y0)), overlap(0, 1)),                                     # 13: the lowest pair first
    (dict(ptrs=(Y0, Y0 + LUMA, Y0 + LUMA - 4)), overlap(0, 2)),
]


def test_the_order_of_check_video_422_target():
    run("check_video_422_target", planes_target, I422, CASES_422)


# ------------------------------------------------------------------------------------------------------------------ A420, A444, A410, UYVA
A444 = dict(ptrs=(Y0, CB0, CR0, A0), pitches=(16, 16, 16, 16), format=VIDEO_A444)
A420 = dict(format=VIDEO_A420, pitches=(16, 8, 8, 16))
A410 = dict(format=VIDEO_A410, pitches=(32, 32, 32, 32))
UYVA = dict(format=VIDEO_UYVA, ptrs=(Y0, 0, 0, A0), pitches=(32, 0, 0, 16))
IGNORE_IS_THE_SIBLINGS = "FDH_VIDEO_IGNORE_ALPHA is the sibling call: these formats carry an alpha plane"
LINEAR_IS_A420S = "FDH_VIDEO_CHROMA_LINEAR is for A420 / UYVA: a 4:4:4 frame has a chroma sample per texel"
ONE_PLANE_UYVA = "planes[1], planes[2] and their pitches must be 0 for UYVA: a UYVY plane and an alpha plane"
EVEN_A420 = "the rectangle's x and y must be even for A420"
EVEN_UYVA = "the rectangle's x must be even for UYVA"
ALPHA_CASES = [
    (dict(ptrs=(Y0, CB0, CR0, 0), format=0), NULL),                               # 1 | 2
    (dict(ptrs=(0, CB0, CR0, A0), matrix=3), NULL),
    (dict(ptrs=(Y0, 0, CR0, A0), format=0), "unknown format"),                    # (planes 1 and 2 are step 8's)
    (dict(format=10, matrix=3), "unknown format"),                                # 2 | 3
    (dict(matrix=3, range=2), "unknown matrix"),                                  # 3 | 4
    (dict(range=2, flags=8), "unknown range"),                                    # 4 | 5
    (dict(flags=8, reserved=(1, 0)), "unknown flag"),                             # 5 | 6
    (dict(reserved=(0, 1), flags=VIDEO_IGNORE_ALPHA), RESERVED),                  # 6 | 7
    (dict(flags=VIDEO_IGNORE_ALPHA | VIDEO_CHROMA_LINEAR), IGNORE_IS_THE_SIBLINGS),  # 7: the alpha flag before the chroma flag
    (dict(flags=VIDEO_CHROMA_LINEAR, ptrs=(Y0, 0, CR0, A0)), LINEAR_IS_A420S),    # 7 | 8
    (dict(UYVA, flags=VIDEO_IGNORE_ALPHA, ptrs=(Y0, CB0, 0, A0)), IGNORE_IS_THE_SIBLINGS),
    (dict(UYVA, pitches=(32, 0, 8, 16), frame=(0, 9)), ONE_PLANE_UYVA),           # 8 | 9
    (dict(ptrs=(Y0, CB0, 0, A0), frame=(16, 0)), NULL),
    (dict(frame=(0, 9), rect=(0, 0, 4, 4)), EMPTY),                               # 9 | 10
    (dict(A420, rect=(1, 0, 16, 9)), OUTSIDE),                                    # 10 | 11
    (dict(UYVA, rect=(3, 2, 14, 8)), OUTSIDE),
    (dict(A420, rect=(0, 1, 4, 4), pitches=(3, 8, 8, 16)), EVEN_A420),            # 11 | 12
    (dict(UYVA, rect=(1, 0, 4, 4), ptrs=(Y0 + 2, 0, 0, A0)), EVEN_UYVA),
    (dict(A410, pitches=(31, 32, 32, 32)), multiple(0)),                          # 12: the multiple before the pitch
    (dict(UYVA, pitches=(30, 0, 0, 16)), multiple(0, GROUP)),
    (dict(A410, pitches=(30, 32, 32, 32), ptrs=(Y0, CB0 + 1, CR0, A0)), below(0)),  # 12: plane 0's pitch before plane 1's multiple
    (dict(A410, pitches=(32, 32, 30, 32), ptrs=(Y0, CB0, CR0, A0 + 1)), below(2)),
    (dict(A410, pitches=(32, 32, 32, 30), ptrs=(Y0, CB0 + 1, CR0, A0)), multiple(1)),
    (dict(UYVA, pitches=(28, 0, 0, 15)), below(0)),
    (dict(UYVA, ptrs=(Y0, 0, 0, Y0), pitches=(32, 0, 0, 15)), below(3)),          # 12 | 13; planes 1 and 2 are absent: their zero pitch is not asked
    (dict(ptrs=(Y0, Y0, CR0, A0), pitches=(16, 16, 16, 15)), below(3)),
    (dict(ptrs=(Y0, Y0, Y0, Y0)), overlap(0, 1)),                                 # 13: the lowest pair first
    (dict(ptrs=(Y0, CB0, Y0 + 100, CB0 + 100)), overlap(0, 2)),
    (dict(ptrs=(Y0, CB0, CR0, CB0 + LUMA - 1)), overlap(1, 3)),
    (dict(UYVA, ptrs=(Y0, 0, 0, Y0)), overlap(0, 3)),                             # ... and no pair with an absent plane
]


def test_the_order_of_check_video_alpha_target():
    run("check_video_alpha_target", alpha_target, A444, ALPHA_CASES)
