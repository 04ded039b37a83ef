"""Three-plane video in and out (fdh_put_video_planes, fdh_update_video_planes, fdh_read_video_planes): the text of
include_video/figdraw_hip_video_planar.h -- and of the two headers it points to for the arithmetic -- in numpy.  I420, I010 (4:2:0) and
I444, I410 (4:4:4); the coefficients derived here from the standards' Kr / Kb as exact rationals.  Written from the headers' comments: it
calls neither tests/video_frame_ref.py nor tests/video_out_ref.py, so that its equality with them on interleaved and shifted samples
(tests/test_video_planar_host.py) is a test.  The level chain and the ink boxes behind the way in's RGBA8 are tests/device_image_ref.py's."""
from fractions import Fraction

import numpy as np

I420, I010, I444, I410 = 3, 4, 5, 6
FORMATS = (I420, I010, I444, I410)
BT601, BT709, BT2020 = 0, 1, 2
LIMITED, FULL = 0, 1
CHROMA_LINEAR, STRAIGHT_ALPHA, IGNORE_ALPHA = 1, 2, 4
KR_KB = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000)),
         BT2020: (Fraction(2627, 10000), Fraction(593, 10000))}
NAMES = {I420: "I420", I010: "I010", I444: "I444", I410: "I410"}


def bits_of(fmt):
    return {I420: 8, I010: 10, I444: 8, I410: 10}[fmt]


def full_chroma(fmt):
    """4:4:4: a chroma sample per texel"""
    return fmt in (I444, I410)


def dtype_of(fmt):
    return np.uint8 if bits_of(fmt) == 8 else np.uint16


def chroma_size(fmt, w, h):
    return (w, h) if full_chroma(fmt) else ((w + 1) // 2, (h + 1) // 2)


def rne(q: Fraction) -> int:
    """an exact rational to the nearest integer, ties to even"""
    lo = q.numerator // q.denominator
    rest = q - lo
    return lo + 1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2) else lo


def ranges(fmt, rng):
    """Yoff, Yden, Cden, Coff"""
    b = bits_of(fmt)
    s = 1 << (b - 8)
    if rng == LIMITED:
        return 16 * s, 219 * s, 224 * s, 128 * s
    return 0, (1 << b) - 1, (1 << b) - 1, 128 * s


# ---------------------------------------------------------------------------------------------------------------------- the way in
def in_coefficients(fmt, matrix, rng):
    """(Yoff, Coff, cY, cRV, cGU, cGV, cBU): 255 * 2^14 times the terms of figdraw_hip_video_frame.h, rounded to nearest even"""
    yoff, yden, cden, coff = ranges(fmt, rng)
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    t = (Fraction(1, yden), 2 * (1 - kr) / cden, 2 * kb * (1 - kb) / (kg * cden), 2 * kr * (1 - kr) / (kg * cden), 2 * (1 - kb) / cden)
    return (yoff, coff) + tuple(rne(255 * 16384 * q) for q in t)


def samples(plane, fmt):
    """the stored bytes or words -> the samples: a 10-bit sample is word & 1023"""
    assert plane.dtype == dtype_of(fmt)
    return plane.astype(np.int64) & ((1 << bits_of(fmt)) - 1)


def chroma_at_texels(c, fmt, w, h, linear):
    """one chroma plane's samples (ch, cw) -> C for every luma texel (h, w)"""
    ch, cw = c.shape
    assert (cw, ch) == chroma_size(fmt, w, h)
    if full_chroma(fmt):
        assert not linear
        return c
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    j, i = y >> 1, x >> 1
    if not linear:
        return c[j, i]
    jn = np.where(y & 1, np.minimum(j + 1, ch - 1), np.maximum(j - 1, 0))
    i1 = np.minimum(i + 1, cw - 1)
    v0, v1 = 3 * c[j, i] + c[jn, i], 3 * c[j, i1] + c[jn, i1]
    return np.where(x & 1, (v0 + v1 + 4) >> 3, (v0 + 2) >> 2)


def convert(planes, fmt, matrix=0, rng=0, flags=0):
    """planes: Y (h, w), Cb and Cr (ch, cw) each, uint8 or uint16 as stored -> the (h, w, 4) uint8 RGBA texels"""
    assert not flags & ~CHROMA_LINEAR
    Y, cb, cr = (samples(p, fmt) for p in planes)
    h, w = Y.shape
    linear = bool(flags & CHROMA_LINEAR)
    yoff, coff, cy, crv, cgu, cgv, cbu = in_coefficients(fmt, matrix, rng)
    y, u, v = Y - yoff, chroma_at_texels(cb, fmt, w, h, linear) - coff, chroma_at_texels(cr, fmt, w, h, linear) - coff
    sums = (cy * y + crv * v + 8192, cy * y - cgu * u - cgv * v + 8192, cy * y + cbu * u + 8192)
    out = np.full((h, w, 4), 255, np.uint8)
    for k, s in enumerate(sums):
        assert np.abs(s).max(initial=0) < 2 ** 31
        out[..., k] = np.clip(s >> 14, 0, 255)  # (>> of a negative int64 floors)
    return out


# ---------------------------------------------------------------------------------------------------------------------- the way out
def out_coefficients(fmt, matrix, rng):
    """(Yoff, Coff, kYR, kYG, kYB, kUR, kUG, kUB, kVR, kVG, kVB) of figdraw_hip_video_out.h"""
    yoff, yden, cden, coff = ranges(fmt, rng)
    kr, kb = KR_KB[matrix]
    ty, tc = Fraction(yden * 16384, 255), Fraction(cden * 16384, 255)
    kyr, kyb = rne(kr * ty), rne(kb * ty)
    kyg = rne(ty) - kyr - kyb
    kub = kvr = rne(tc / 2)
    kur = -rne(kr * tc / (2 * (1 - kb)))
    kvb = -rne(kb * tc / (2 * (1 - kr)))
    return (yoff, coff, kyr, kyg, kyb, kur, -(kub + kur), kub, kvr, -(kvr + kvb), kvb)


def _dot(k, c):
    s = k[0] * c[..., 0] + k[1] * c[..., 1] + k[2] * c[..., 2]
    assert (abs(k[0]) * c[..., 0] + abs(k[1]) * c[..., 1] + abs(k[2]) * c[..., 2]).max(initial=0) < 2 ** 31 - (8 << 13)
    return s


def luma(rgb, fmt, matrix, rng):
    k = out_coefficients(fmt, matrix, rng)
    return k[0] + ((_dot(k[2:5], rgb.astype(np.int64)) + 8192) >> 14)


def chroma_of_sums(s, n, fmt, matrix, rng):
    """(..., 3) component-wise sums of n = 1, 4 or 8 texels -> Cb, Cr"""
    k = out_coefficients(fmt, matrix, rng)
    shift, top = 14 + {1: 0, 4: 2, 8: 3}[n], (1 << bits_of(fmt)) - 1
    s = s.astype(np.int64)
    return tuple(np.clip(k[1] + ((_dot(row, s) + (n << 13)) >> shift), 0, top) for row in (k[5:8], k[8:11]))


def chroma_sums(rgb, fmt, linear):
    """(h, w, 3) colour bytes -> the sums s of every chroma sample, and N"""
    p = rgb.astype(np.int64)
    if full_chroma(fmt):
        assert not linear
        return p, 1
    h, w = p.shape[:2]
    j, i = np.arange((h + 1) // 2), np.arange((w + 1) // 2)
    rows = p[2 * j] + p[np.minimum(2 * j + 1, h - 1)]
    if not linear:
        return rows[:, 2 * i] + rows[:, np.minimum(2 * i + 1, w - 1)], 4
    return rows[:, np.maximum(2 * i - 1, 0)] + 2 * rows[:, 2 * i] + rows[:, np.minimum(2 * i + 1, w - 1)], 8


def chroma_float(rgb, fmt, matrix, rng):
    """the exact Cb, Cr of a colour in float64, unrounded and unclamped"""
    _, _, cden, coff = ranges(fmt, rng)
    kr, kb = (float(v) for v in KR_KB[matrix])
    c = rgb.astype(np.float64)
    y = kr * c[..., 0] + (1 - kr - kb) * c[..., 1] + kb * c[..., 2]
    return coff + cden * (c[..., 2] - y) / (2 * (1 - kb)) / 255.0, coff + cden * (c[..., 0] - y) / (2 * (1 - kr)) / 255.0


def export(img, fmt, matrix=0, rng=0, flags=0):
    """(h, w, 4) uint8 RGBA as fdh_read_pixels returns it -> (Y, Cb, Cr) as stored: uint8, or uint16 words with the value in the low bits"""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4 and not flags & ~CHROMA_LINEAR
    rgb = img[..., :3]
    y = luma(rgb, fmt, matrix, rng)
    s, n = chroma_sums(rgb, fmt, bool(flags & CHROMA_LINEAR))
    cb, cr = chroma_of_sums(s, n, fmt, matrix, rng)
    assert y.min() >= 0 and y.max() < 1 << bits_of(fmt)
    return tuple(np.ascontiguousarray(p.astype(dtype_of(fmt))) for p in (y, cb, cr))
