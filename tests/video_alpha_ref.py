"""Video with an alpha plane in and out (fdh_put_video_alpha, fdh_update_video_alpha, fdh_read_video_alpha): the text of
include_video/figdraw_hip_video_alpha.h in numpy.  A420, A444, A410 (I420's, I444's, I410's three planes and A) and UYVA (a UYVY plane and
A).  Everything a base format already specifies is asked of its own reference and not restated: the coefficients, the conversion, the
chroma rules, the weights of a chroma sample and the packed layout come from tests/video_planar_ref.py (A420, A444, A410) and
tests/video_422_ref.py (UYVA), the premultiply rule of FDH_VIDEO_STRAIGHT_ALPHA on the way in from tests/video_frame_ref.py.  What is
written here from the header's comment is the alpha sample and the un-premultiplied sample of the straight way out.  The level chain and
the ink boxes behind the way in's RGBA8 are tests/device_image_ref.py's."""
import numpy as np

import video_422_ref as V2
import video_frame_ref as VF
import video_planar_ref as PL

A420, A444, A410, UYVA = 11, 12, 13, 14
FORMATS = (A420, A444, A410, UYVA)
BT601, BT709, BT2020 = PL.BT601, PL.BT709, PL.BT2020
LIMITED, FULL = PL.LIMITED, PL.FULL
CHROMA_LINEAR, STRAIGHT_ALPHA, IGNORE_ALPHA = 1, 2, 4
NAMES = {A420: "A420", A444: "A444", A410: "A410", UYVA: "UYVA"}
BASE = {A420: (PL, PL.I420), A444: (PL, PL.I444), A410: (PL, PL.I410), UYVA: (V2, V2.UYVY)}  # the reference and the format of planes 0 .. 2


def bits_of(fmt):
    return 10 if fmt == A410 else 8


def packed(fmt):
    """planes[0] is a UYVY plane; there are no planes[1], planes[2]"""
    return fmt == UYVA


def full_chroma(fmt):
    return fmt in (A444, A410)


def linear_allowed(fmt):
    return fmt in (A420, UYVA)


def dtype_of(fmt):
    return np.uint8 if bits_of(fmt) == 8 else np.uint16


def n_of(fmt, flags):
    """the sum of a chroma sample's weights"""
    return {A420: 4, A444: 1, A410: 1, UYVA: 2}[fmt] * (2 if flags & CHROMA_LINEAR else 1)


def in_coefficients(fmt, matrix, rng):
    ref, base = BASE[fmt]
    return ref.in_coefficients(base, matrix, rng)


def out_coefficients(fmt, matrix, rng):
    ref, base = BASE[fmt]
    return ref.out_coefficients(base, matrix, rng)


def ranges(fmt, rng):
    ref, base = BASE[fmt]
    return ref.ranges(base, rng)


# ---------------------------------------------------------------------------------------------------------------------- the alpha sample
def alpha_out(a, fmt):
    """alpha bytes -> the samples as stored"""
    a = np.asarray(a).astype(np.int64)
    return ((1023 * a + 127) // 255 if bits_of(fmt) == 10 else a).astype(dtype_of(fmt))


def alpha_in(plane, fmt):
    """the stored bytes or words -> alpha bytes; a 10-bit sample is word & 1023"""
    assert plane.dtype == dtype_of(fmt)
    a = plane.astype(np.int64)
    return ((255 * (a & 1023) + 511) // 1023 if bits_of(fmt) == 10 else a).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------- the way in
def convert(stored, fmt, matrix=0, rng=0, flags=0, w=None):
    """stored: (Y, Cb, Cr, A) for A420 / A444 / A410, (the UYVY plane (h, 4 cw) uint8, A) and the width `w` for UYVA -> the (h, w, 4) uint8
    RGBA texels"""
    assert not flags & ~(CHROMA_LINEAR | STRAIGHT_ALPHA) and (linear_allowed(fmt) or not flags & CHROMA_LINEAR)
    ref, base = BASE[fmt]
    if packed(fmt):
        assert len(stored) == 2 and w is not None
        out = ref.convert(stored[:1], base, matrix, rng, flags & CHROMA_LINEAR, w=w)
    else:
        assert len(stored) == 4
        out = ref.convert(stored[:3], base, matrix, rng, flags & CHROMA_LINEAR)
    out = out.copy()
    a = alpha_in(stored[-1], fmt)
    assert a.shape == out.shape[:2]
    out[..., 3] = a
    return VF.premultiply(out) if flags & STRAIGHT_ALPHA else out


# ---------------------------------------------------------------------------------------------------------------------- the way out
def unpremultiplied(sums, n):
    """(..., 4) weighted sums sc (three channels) and sa of a sample whose weights sum to n -> (..., 3): per channel
    (sa == 0) ? 0 : min(255 n, (510 n sc + sa) / (2 sa))"""
    s = np.asarray(sums).astype(np.int64)
    sc, sa = s[..., :3], s[..., 3:]
    assert (510 * n * sc + sa).max(initial=0) < 2 ** 24
    q = np.minimum(255 * n, (510 * n * sc + sa) // np.maximum(2 * sa, 1))
    return np.where(sa == 0, 0, q)


def weighted_sums(img, fmt, flags):
    """(h, w, k) bytes -> the base format's weighted sums of every chroma sample, channel by channel, and N"""
    ref, base = BASE[fmt]
    linear = bool(flags & CHROMA_LINEAR)
    return ref.chroma_sums(img, linear) if packed(fmt) else ref.chroma_sums(img, base, linear)


def export_planes(img, fmt, matrix=0, rng=0, flags=0):
    """(h, w, 4) uint8 premultiplied RGBA as fdh_read_pixels returns it -> the samples (Y, Cb, Cr, A), whatever the layout"""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4
    assert not flags & ~(CHROMA_LINEAR | STRAIGHT_ALPHA) and (linear_allowed(fmt) or not flags & CHROMA_LINEAR)
    ref, base = BASE[fmt]
    a = alpha_out(img[..., 3], fmt)
    if not flags & STRAIGHT_ALPHA:  # the colour bytes as stored: the sibling's export
        y, cb, cr = ref.export_planes(img, base, matrix, rng, flags) if packed(fmt) else ref.export(img, base, matrix, rng, flags)
        return y, cb, cr, a
    y = ref.luma(unpremultiplied(img, 1), base, matrix, rng)
    sums, n = weighted_sums(img, fmt, flags)
    assert n == n_of(fmt, flags)
    cb, cr = ref.chroma_of_sums(unpremultiplied(sums, n), n, base, matrix, rng)
    assert y.min() >= 0 and y.max() < 1 << bits_of(fmt)
    return tuple(np.ascontiguousarray(p.astype(dtype_of(fmt))) for p in (y, cb, cr)) + (a,)


def export(img, fmt, matrix=0, rng=0, flags=0):
    """... -> what the call stores: (Y, Cb, Cr, A), uint8 or uint16 words with the value in the low bits, or (the UYVY plane, A)"""
    y, cb, cr, a = export_planes(img, fmt, matrix, rng, flags)
    return (V2.interleave((y, cb, cr), V2.UYVY), a) if packed(fmt) else (y, cb, cr, a)


def export_float(img, fmt, matrix, rng, flags, eight_bit_colour=False):
    """the exact straight export in float64, unrounded and unclamped: (Y, Cb, Cr) of the exactly un-premultiplied texel and of the exactly
    un-premultiplied weighted average (0 where the weights' alpha is 0).  eight_bit_colour (N = 1 alone): of the texel's 8-bit straight
    colour u instead -- the header's stated limit of the straight path, what a 10-bit sample is made of"""
    ref, base = BASE[fmt]
    p = img.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(p[..., 3:] > 0, np.minimum(255.0, 255.0 * p[..., :3] / p[..., 3:]), 0.0)
        sums, n = weighted_sums(img, fmt, flags)
        s = sums.astype(np.float64)
        avg = np.where(s[..., 3:] > 0, np.minimum(255.0, 255.0 * s[..., :3] / s[..., 3:]), 0.0)
    if eight_bit_colour:
        assert n == 1
        u = avg = unpremultiplied(img, 1).astype(np.float64)
    yoff, yden, _, _ = ranges(fmt, rng)
    kr, kb = (float(v) for v in PL.KR_KB[matrix])
    y = yoff + yden * (kr * u[..., 0] + (1 - kr - kb) * u[..., 1] + kb * u[..., 2]) / 255.0
    cb, cr = ref.chroma_float(avg, base, matrix, rng)
    return y, cb, cr
