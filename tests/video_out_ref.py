"""The rendered frame out as NV12, P010 or BGRA8 (fdh_read_video_frame): the text of include_video/figdraw_hip_video_out.h in numpy -- the
coefficients derived here from the standards' Kr / Kb as exact rationals (not from the header's table), the luma rule, the two chroma
sitings with their clamps to the rectangle, the stored words, and the BGRA8 rules.  Written from the header's comment, not from the C++."""
from fractions import Fraction

import numpy as np

from video_frame_ref import (BGRA8, BT601, BT709, BT2020, CHROMA_LINEAR, FULL, IGNORE_ALPHA, KR_KB, LIMITED, NV12, P010,  # noqa: F401
                             STRAIGHT_ALPHA, bits_of, round_half_even)


def ranges(fmt, rng):
    """Yoff, Yden, Cden, Coff"""
    b = bits_of(fmt)
    s = 1 << (b - 8)
    if rng == LIMITED:
        return 16 * s, 219 * s, 224 * s, 128 * s
    return 0, (1 << b) - 1, (1 << b) - 1, 128 * s


def coefficients(fmt, matrix, rng):
    """(Yoff, Coff, kYR, kYG, kYB, kUR, kUG, kUB, kVR, kVG, kVB)"""
    yoff, yden, cden, coff = ranges(fmt, rng)
    kr, kb = KR_KB[matrix]
    ty, tc = Fraction(yden * 16384, 255), Fraction(cden * 16384, 255)
    rne = round_half_even
    kyr, kyb = rne(kr * ty), rne(kb * ty)
    kyg = rne(ty) - kyr - kyb
    kub = kvr = rne(tc / 2)
    kur = -rne(kr * tc / (2 * (1 - kb)))
    kvb = -rne(kb * tc / (2 * (1 - kr)))
    return (yoff, coff, kyr, kyg, kyb, kur, -(kub + kur), kub, kvr, -(kvr + kvb), kvb)


def _dot(k, c):
    c = c.astype(np.int64)
    s = k[0] * c[..., 0] + k[1] * c[..., 1] + k[2] * c[..., 2]
    assert (abs(k[0]) * c[..., 0] + abs(k[1]) * c[..., 1] + abs(k[2]) * c[..., 2]).max(initial=0) < 2 ** 31 - (8 << 13)
    return s


def luma(rgb, fmt, matrix, rng):
    """(..., 3) colour bytes -> the luma samples"""
    k = coefficients(fmt, matrix, rng)
    return k[0] + ((_dot(k[2:5], rgb) + 8192) >> 14)  # (>> of a negative int64 floors)


def chroma_of_sums(s, n, fmt, matrix, rng):
    """(..., 3) component-wise sums of n = 1, 4 or 8 texels -> Cb, Cr samples"""
    k = coefficients(fmt, matrix, rng)
    shift, top = 14 + {1: 0, 4: 2, 8: 3}[n], (1 << bits_of(fmt)) - 1
    cb = np.clip(k[1] + ((_dot(k[5:8], s) + (n << 13)) >> shift), 0, top)
    cr = np.clip(k[1] + ((_dot(k[8:11], s) + (n << 13)) >> shift), 0, top)
    return cb, cr


def chroma_sums(rgb, linear):
    """(h, w, 3) -> the sums s of every pair, (ch, cw, 3), and N"""
    h, w = rgb.shape[:2]
    p = rgb.astype(np.int64)
    j, i = np.arange((h + 1) // 2), np.arange((w + 1) // 2)
    rows = p[2 * j] + p[np.minimum(2 * j + 1, h - 1)]  # (ch, w, 3): both rows of every pair
    if not linear:
        return rows[:, 2 * i] + rows[:, np.minimum(2 * i + 1, w - 1)], 4
    return rows[:, np.maximum(2 * i - 1, 0)] + 2 * rows[:, 2 * i] + rows[:, np.minimum(2 * i + 1, w - 1)], 8


def luma_float(rgb, fmt, matrix, rng):
    """the exact luma in float64, unrounded"""
    yoff, yden, _, _ = ranges(fmt, rng)
    kr, kb = (float(v) for v in KR_KB[matrix])
    c = rgb.astype(np.float64)
    return yoff + yden * (kr * c[..., 0] + (1 - kr - kb) * c[..., 1] + kb * c[..., 2]) / 255.0


def chroma_float(s, n, fmt, matrix, rng):
    """the exact Cb, Cr of the exactly averaged colour s / n in float64, unrounded and unclamped"""
    _, _, cden, coff = ranges(fmt, rng)
    kr, kb = (float(v) for v in KR_KB[matrix])
    c = s.astype(np.float64) / n
    y = kr * c[..., 0] + (1 - kr - kb) * c[..., 1] + kb * c[..., 2]
    return coff + cden * (c[..., 2] - y) / (2 * (1 - kb)) / 255.0, coff + cden * (c[..., 0] - y) / (2 * (1 - kr)) / 255.0


def export(img, fmt, matrix=0, rng=0, flags=0):
    """(h, w, 4) uint8 RGBA as fdh_read_pixels returns it -> (planes[0], planes[1]) as stored: NV12 (h, w) uint8 and (ch, cw, 2) uint8; P010
    the same of uint16 words value << 6; BGRA8 (h, w, 4) uint8 and None"""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4 and not flags & STRAIGHT_ALPHA
    if fmt == BGRA8:
        assert matrix == 0 and rng == 0 and not flags & CHROMA_LINEAR
        out = img[..., [2, 1, 0, 3]].copy()
        if flags & IGNORE_ALPHA:
            out[..., 3] = 255
        return out, None
    assert not flags & IGNORE_ALPHA
    rgb = img[..., :3]
    y = luma(rgb, fmt, matrix, rng)
    s, n = chroma_sums(rgb, bool(flags & CHROMA_LINEAR))
    c = np.stack(chroma_of_sums(s, n, fmt, matrix, rng), axis=2)
    assert y.min() >= 0 and y.max() < 1 << bits_of(fmt)
    if fmt == NV12:
        return y.astype(np.uint8), c.astype(np.uint8)
    return (y << 6).astype(np.uint16), (c << 6).astype(np.uint16)
