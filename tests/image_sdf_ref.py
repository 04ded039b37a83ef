"""The rule of include_glyphs/figdraw_hip_image_sdf.h in float64 numpy, written from that header alone: a brute force over the search window,
and over the whole plane for small images.  Nothing is shared with the device code."""
import math

import numpy as np


def reach(R):
    """how far the bounded search looks along each axis"""
    return int(math.floor(R / 2.0 + 0.5)) + 1


def distances(cov, pad, R=None):
    """cov: (h, w) uint8 coverage bytes -> d: (h + 2 pad, w + 2 pad) float64, +-inf where no candidate exists.  R: the search stops at
    |dx|, |dy| <= reach(R); None: every texel of the plane takes part"""
    cov = np.asarray(cov, np.uint8)
    h, w = cov.shape
    oh, ow = h + 2 * pad, w + 2 * pad
    # unbounded: the source and one ring of the plane outside it, from every texel of the output.  (A texel of the plane farther out is
    # farther from p than the ring's texel on the way to it, and has the same e.)
    r = reach(R) if R is not None else max(oh, ow) + 1
    m = pad + r
    plane = np.zeros((h + 2 * m, w + 2 * m))
    plane[m:m + h, m:m + w] = cov.astype(np.float64) / 255.0
    c_p = plane[r:r + oh, r:r + ow]
    best_in = np.full((oh, ow), np.inf)   # min over c_q < 1 of |p - q| + e_q
    best_out = np.full((oh, ow), np.inf)  # min over c_q > 0 of |p - q| - e_q
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            c_q = plane[r + dy:r + dy + oh, r + dx:r + dx + ow]
            apart = math.sqrt(dx * dx + dy * dy)
            e_q = c_q - 0.5
            np.minimum(best_in, np.where(c_q < 1.0, apart + e_q, np.inf), out=best_in)
            np.minimum(best_out, np.where(c_q > 0.0, apart - e_q, np.inf), out=best_out)
    return np.where(2.0 * c_p >= 1.0, best_in, -best_out)


def encode(d, R):
    """the byte of every texel"""
    with np.errstate(invalid="ignore"):
        v = np.clip(0.5 + d / float(R), 0.0, 1.0)
    return np.floor(255.0 * v + 0.5).astype(np.uint8)


def field(cov, pad, R, bounded=True):
    """-> (h + 2 pad, w + 2 pad) uint8: what every one of the four bytes of a texel holds"""
    return encode(distances(cov, pad, R if bounded else None), R)
