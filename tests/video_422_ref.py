"""4:2:2 video in and out (fdh_put_video_422, fdh_update_video_422, fdh_read_video_422): the text of include_video/figdraw_hip_video_422.h
in numpy.  I422, I210 (three planes) and YUY2, UYVY (one plane of four-byte groups).  The coefficients, the ranges and the float64 values
are tests/video_planar_ref.py's functions, asked for I420 (8 bit) or I010 (10 bit): the header takes its rows from the same tables.  The
chroma rules are written here from the header's comment and call no 4:2:0 code, so that their equality with the 4:2:0 references on
doubled rows (tests/test_video_422_host.py) is a test.  The level chain and the ink boxes behind the way in's RGBA8 are
tests/device_image_ref.py's."""
import numpy as np

import video_planar_ref as PL

I422, I210, YUY2, UYVY = 7, 8, 9, 10
FORMATS = (I422, I210, YUY2, UYVY)
BT601, BT709, BT2020 = PL.BT601, PL.BT709, PL.BT2020
LIMITED, FULL = PL.LIMITED, PL.FULL
CHROMA_LINEAR, STRAIGHT_ALPHA, IGNORE_ALPHA = 1, 2, 4
NAMES = {I422: "I422", I210: "I210", YUY2: "YUY2", UYVY: "UYVY"}


def bits_of(fmt):
    return {I422: 8, I210: 10, YUY2: 8, UYVY: 8}[fmt]


def packed(fmt):
    """one plane of four-byte groups"""
    return fmt in (YUY2, UYVY)


def sibling(fmt):
    """the 4:2:0 format with the same bit depth: its rows of the coefficient tables are this format's"""
    return PL.I420 if bits_of(fmt) == 8 else PL.I010


def dtype_of(fmt):
    return np.uint8 if bits_of(fmt) == 8 else np.uint16


def chroma_width(w):
    return (w + 1) // 2


def ranges(fmt, rng):
    """Yoff, Yden, Cden, Coff"""
    return PL.ranges(sibling(fmt), rng)


def in_coefficients(fmt, matrix, rng):
    return PL.in_coefficients(sibling(fmt), matrix, rng)


def out_coefficients(fmt, matrix, rng):
    return PL.out_coefficients(sibling(fmt), matrix, rng)


# ---------------------------------------------------------------------------------------------------------------------- the packed layouts
def interleave(planes, fmt):
    """(Y (h, w), Cb (h, cw), Cr (h, cw)) uint8 -> the packed plane (h, 4 cw) uint8.  An odd w: the last group's second luma byte is the
    luma of column w - 1 (what the way out writes there)"""
    y, cb, cr = planes
    h, w = y.shape
    cw = chroma_width(w)
    assert packed(fmt) and cb.shape == cr.shape == (h, cw) and y.dtype == np.uint8
    y2 = np.concatenate([y, y[:, -1:]], axis=1) if w & 1 else y
    out = np.empty((h, cw, 4), np.uint8)
    a, c = (0, 1) if fmt == YUY2 else (1, 0)  # where a group's first luma and its Cb lie
    out[..., a], out[..., a + 2], out[..., c], out[..., c + 2] = y2[:, 0::2], y2[:, 1::2], cb, cr
    return out.reshape(h, 4 * cw)


def deinterleave(plane, fmt, w):
    """the packed plane (h, >= 4 cw) uint8 -> (Y (h, w), Cb (h, cw), Cr (h, cw)).  An odd w: the last group's second luma byte is ignored"""
    cw = chroma_width(w)
    g = plane[:, :4 * cw].reshape(plane.shape[0], cw, 4)
    a, c = (0, 1) if fmt == YUY2 else (1, 0)
    y = np.stack([g[..., a], g[..., a + 2]], axis=2).reshape(plane.shape[0], 2 * cw)[:, :w]
    return np.ascontiguousarray(y), np.ascontiguousarray(g[..., c]), np.ascontiguousarray(g[..., c + 2])


def as_planes(stored, fmt, w):
    """what a call takes or leaves -> (Y, Cb, Cr): the three planes themselves, or the one packed plane's samples"""
    return deinterleave(stored[0], fmt, w) if packed(fmt) else tuple(stored)


# ---------------------------------------------------------------------------------------------------------------------- the way in
def samples(plane, fmt):
    """the stored bytes or words -> the samples: a 10-bit sample is word & 1023"""
    assert plane.dtype == dtype_of(fmt)
    return plane.astype(np.int64) & ((1 << bits_of(fmt)) - 1)


def chroma_at_texels(c, w, linear):
    """one chroma plane's samples (h, cw) -> C for every luma texel (h, w): the header's two rules, along the row alone"""
    h, cw = c.shape
    assert cw == chroma_width(w)
    x = np.arange(w)
    i = x >> 1
    if not linear:
        return c[:, i]
    i1 = np.minimum(i + 1, cw - 1)
    return np.where(x & 1, (c[:, i] + c[:, i1] + 1) >> 1, c[:, i])


def convert(stored, fmt, matrix=0, rng=0, flags=0, w=None):
    """stored: (Y (h, w), Cb, Cr (h, cw)) uint8 or uint16 for I422 / I210; (the packed plane (h, 4 cw) uint8,) and the width `w` for
    YUY2 / UYVY -> the (h, w, 4) uint8 RGBA texels"""
    assert not flags & ~CHROMA_LINEAR
    if packed(fmt):
        assert w is not None
    else:
        w = stored[0].shape[1]
    Y, cb, cr = (samples(p, fmt) for p in as_planes(stored, fmt, w))
    h = Y.shape[0]
    assert Y.shape == (h, w)
    linear = bool(flags & CHROMA_LINEAR)
    yoff, coff, cy, crv, cgu, cgv, cbu = in_coefficients(fmt, matrix, rng)
    y, u, v = Y - yoff, chroma_at_texels(cb, w, linear) - coff, chroma_at_texels(cr, w, linear) - coff
    sums = (cy * y + crv * v + 8192, cy * y - cgu * u - cgv * v + 8192, cy * y + cbu * u + 8192)
    out = np.full((h, w, 4), 255, np.uint8)
    for k, s in enumerate(sums):
        assert np.abs(s).max(initial=0) < 2 ** 31
        out[..., k] = np.clip(s >> 14, 0, 255)  # (>> of a negative int64 floors)
    return out


# ---------------------------------------------------------------------------------------------------------------------- the way out
def _dot(k, c):
    s = k[0] * c[..., 0] + k[1] * c[..., 1] + k[2] * c[..., 2]
    assert (abs(k[0]) * c[..., 0] + abs(k[1]) * c[..., 1] + abs(k[2]) * c[..., 2]).max(initial=0) < 2 ** 31 - (8 << 13)
    return s


def luma(rgb, fmt, matrix, rng):
    k = out_coefficients(fmt, matrix, rng)
    return k[0] + ((_dot(k[2:5], rgb.astype(np.int64)) + 8192) >> 14)


def chroma_of_sums(s, n, fmt, matrix, rng):
    """(..., 3) component-wise sums of n = 2 or 4 colours -> Cb, Cr"""
    k = out_coefficients(fmt, matrix, rng)
    shift, top = 14 + {2: 1, 4: 2}[n], (1 << bits_of(fmt)) - 1
    s = s.astype(np.int64)
    return tuple(np.clip(k[1] + ((_dot(row, s) + (n << 13)) >> shift), 0, top) for row in (k[5:8], k[8:11]))


def chroma_sums(rgb, linear):
    """(h, w, 3) colour bytes -> the sums s of every chroma sample (h, cw, 3), and N"""
    p = rgb.astype(np.int64)
    w = p.shape[1]
    i = np.arange(chroma_width(w))
    if not linear:
        return p[:, 2 * i] + p[:, np.minimum(2 * i + 1, w - 1)], 2
    return p[:, np.maximum(2 * i - 1, 0)] + 2 * p[:, 2 * i] + p[:, np.minimum(2 * i + 1, w - 1)], 4


def chroma_float(rgb, fmt, matrix, rng):
    """the exact Cb, Cr of a colour in float64, unrounded and unclamped"""
    return PL.chroma_float(rgb, sibling(fmt), matrix, rng)


def export_planes(img, fmt, matrix=0, rng=0, flags=0):
    """(h, w, 4) uint8 RGBA -> the samples (Y (h, w), Cb (h, cw), Cr (h, cw)) in the format's sample type, whatever its layout"""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4 and not flags & ~CHROMA_LINEAR
    rgb = img[..., :3]
    y = luma(rgb, fmt, matrix, rng)
    s, n = chroma_sums(rgb, bool(flags & CHROMA_LINEAR))
    cb, cr = chroma_of_sums(s, n, fmt, matrix, rng)
    assert y.min() >= 0 and y.max() < 1 << bits_of(fmt)
    return tuple(np.ascontiguousarray(p.astype(dtype_of(fmt))) for p in (y, cb, cr))


def export(img, fmt, matrix=0, rng=0, flags=0):
    """(h, w, 4) uint8 RGBA as fdh_read_pixels returns it -> what the call stores: (Y, Cb, Cr), uint8 or uint16 words with the value in the
    low bits, or (the packed plane (h, 4 cw) uint8,)"""
    planes = export_planes(img, fmt, matrix, rng, flags)
    return (interleave(planes, fmt),) if packed(fmt) else planes
