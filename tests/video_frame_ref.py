"""Decoded video frames (fdh_put_video_frame, fdh_update_video_frame): the text of include_glyphs/figdraw_hip_video_frame.h in numpy -- the
samples, the chroma upsampling, the integer conversion with coefficients derived here from the standards' Kr / Kb as exact rationals (not
from the header's table), and the BGRA8 rules.  The result is RGBA8 bytes; the level chain and the ink boxes behind them are
tests/device_image_ref.py's.  Written from the header's comment, not from the C++."""
from fractions import Fraction

import numpy as np

from device_image_ref import chain, ink_boxes, minify, premultiply  # noqa: F401  (what is stored of the converted bytes)

BGRA8, NV12, P010 = 0, 1, 2
BT601, BT709, BT2020 = 0, 1, 2
LIMITED, FULL = 0, 1
CHROMA_LINEAR, STRAIGHT_ALPHA, IGNORE_ALPHA = 1, 2, 4
KR_KB = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000)),
         BT2020: (Fraction(2627, 10000), Fraction(593, 10000))}


def bits_of(fmt):
    return {NV12: 8, P010: 10}[fmt]


def round_half_even(q: Fraction) -> int:
    lo = q.numerator // q.denominator
    rest = q - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2):
        return lo + 1
    return lo


def terms(fmt, matrix, rng):
    """Yoff, Coff and the five exact terms (Fractions) that the coefficients are 255 * 2^14 times of"""
    b = bits_of(fmt)
    s = 1 << (b - 8)
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    if rng == LIMITED:
        yoff, yden, cden = 16 * s, 219 * s, 224 * s
    else:
        yoff, yden, cden = 0, (1 << b) - 1, (1 << b) - 1
    t = (Fraction(1, yden), 2 * (1 - kr) / cden, 2 * kb * (1 - kb) / (kg * cden), 2 * kr * (1 - kr) / (kg * cden), 2 * (1 - kb) / cden)
    return yoff, 128 * s, t


def coefficients(fmt, matrix, rng):
    """(Yoff, Coff, cY, cRV, cGU, cGV, cBU)"""
    yoff, coff, t = terms(fmt, matrix, rng)
    return (yoff, coff) + tuple(round_half_even(255 * 16384 * q) for q in t)


def samples(plane, fmt):
    """the stored words -> the samples: NV12 bytes; P010 word >> 6"""
    if fmt == NV12:
        assert plane.dtype == np.uint8
        return plane.astype(np.int64)
    assert plane.dtype == np.uint16
    return (plane >> 6).astype(np.int64)


def upsample(c, w, h, linear):
    """one chroma component (ch, cw) -> its value at every luma texel (h, w)"""
    ch, cw = c.shape
    assert (cw, ch) == ((w + 1) // 2, (h + 1) // 2)
    c = c.astype(np.int64)
    y, x = np.arange(h), np.arange(w)
    j, i = y >> 1, x >> 1
    if not linear:
        return c[j][:, i]
    jn = np.where(y & 1, np.minimum(j + 1, ch - 1), np.maximum(j - 1, 0))
    v = 3 * c[j] + c[jn]  # (h, cw)
    even = (v[:, i] + 2) >> 2
    odd = (v[:, i] + v[:, np.minimum(i + 1, cw - 1)] + 4) >> 3
    return np.where((x & 1)[None, :], odd, even)


def yuv_to_rgba(Y, cb, cr, fmt, matrix, rng):
    """samples (int arrays of one shape) -> RGBA8, the integer rule"""
    yoff, coff, cy, crv, cgu, cgv, cbu = coefficients(fmt, matrix, rng)
    y, u, v = Y.astype(np.int64) - yoff, cb.astype(np.int64) - coff, cr.astype(np.int64) - coff
    sums = (cy * y + crv * v + 8192, cy * y - cgu * u - cgv * v + 8192, cy * y + cbu * u + 8192)
    for s in sums:
        assert np.abs(s).max(initial=0) < 2 ** 31
    out = np.full(Y.shape + (4,), 255, np.uint8)
    for k, s in enumerate(sums):
        out[..., k] = np.clip(s >> 14, 0, 255)  # (>> of a negative int64 floors)
    return out


def yuv_to_rgb_float(Y, cb, cr, fmt, matrix, rng):
    """the exact conversion in float64, unrounded and unclamped, in byte units: (..., 3)"""
    yoff, coff, t = terms(fmt, matrix, rng)
    ty, trv, tgu, tgv, tbu = (float(255 * q) for q in t)
    y, u, v = Y.astype(np.float64) - yoff, cb.astype(np.float64) - coff, cr.astype(np.float64) - coff
    return np.stack([ty * y + trv * v, ty * y - tgu * u - tgv * v, ty * y + tbu * u], axis=-1)


def convert(luma, chroma, fmt, matrix=0, rng=0, flags=0):
    """the (h, w, 4) uint8 texels of a frame.  NV12: luma (h, w) uint8, chroma (ch, cw, 2) uint8; P010: the same of uint16 words; BGRA8: luma
    (h, w, 4) uint8 and chroma None"""
    if fmt == BGRA8:
        assert luma.dtype == np.uint8 and luma.ndim == 3 and luma.shape[2] == 4 and chroma is None and matrix == 0 and rng == 0
        assert not flags & CHROMA_LINEAR and flags & (STRAIGHT_ALPHA | IGNORE_ALPHA) != (STRAIGHT_ALPHA | IGNORE_ALPHA)
        rgba = luma[..., [2, 1, 0, 3]].copy()
        if flags & IGNORE_ALPHA:
            rgba[..., 3] = 255
        return premultiply(rgba) if flags & STRAIGHT_ALPHA else rgba
    assert not flags & (STRAIGHT_ALPHA | IGNORE_ALPHA)
    h, w = luma.shape
    Y, c = samples(luma, fmt), samples(chroma, fmt)
    linear = bool(flags & CHROMA_LINEAR)
    return yuv_to_rgba(Y, upsample(c[..., 0], w, h, linear), upsample(c[..., 1], w, h, linear), fmt, matrix, rng)
