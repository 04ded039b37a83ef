"""Inputs of the image distance-field tests (test_image_sdf_host.py, test_image_sdf.py; tools/image_sdf_bench.py uses the glyphs): the 94
coverage glyphs of the font fixture at four (range, pad) pairs, and the small and hostile images at which the kernel can go wrong.  The
reference (image_sdf_ref.py) runs once per case and process: reference(case)."""
import os

import numpy as np

import image_sdf_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLYPH_SETTINGS = ((1, 1), (4, 2), (8, 4), (7, 3))  # (R, pad)


def white(cov):
    """(h, w) coverage bytes -> premultiplied white RGBA8, every channel the coverage"""
    cov = np.asarray(cov, np.uint8)
    return np.ascontiguousarray(np.repeat(cov[..., None], 4, axis=2))


def glyph_images():
    """-> {code: (h, w, 4) uint8}: cov_33 .. cov_126 of tests/golden/glyphs_ubuntu20.npz"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "glyphs_ubuntu20.npz"))
    return {code: np.ascontiguousarray(z[f"cov_{code}"], np.uint8) for code in range(33, 127)}


def glyphs():
    """-> [(name, rgba, channel, pad, R)]: every glyph's alpha channel at every setting"""
    imgs = glyph_images()
    return [(f"glyph {code} R={R} pad={pad}", imgs[code], 3, pad, R) for R, pad in GLYPH_SETTINGS for code in range(33, 127)]


def disc(w, h, cx, cy, radius, ss=16):
    """an antialiased disc, ss x ss samples per texel -> (h, w) uint8"""
    s = (np.arange(ss) + 0.5) / ss
    xs = (np.arange(w)[:, None] + s[None, :]).reshape(-1)
    ys = (np.arange(h)[:, None] + s[None, :]).reshape(-1)
    inside = (xs[None, :] - cx) ** 2 + (ys[:, None] - cy) ** 2 <= radius * radius
    frac = inside.reshape(h, ss, w, ss).mean(axis=(1, 3))
    return np.floor(255.0 * frac + 0.5).astype(np.uint8)


DISC = dict(w=40, h=40, cx=20.2, cy=19.7, radius=10.3)  # the disc of the header's table
HALF_PLANE_EDGE = 5.3


def half_plane(w=24, h=21):
    """covered where x < 5.3: columns 0 .. 4 full, column 5 by 0.3"""
    cov = np.zeros((h, w), np.uint8)
    cov[:, :5] = 255
    cov[:, 5] = int(np.floor(255.0 * 0.3 + 0.5))
    return cov


def hostile():
    """-> [(name, rgba, channel, pad, R)]"""
    rng = np.random.default_rng(20240607)

    def blobs(w, h):  # bytes with runs of 0 and of 255 among them
        v = rng.integers(-200, 456, size=(h, w))
        return np.clip(v, 0, 255).astype(np.uint8)

    out = [(f"1 x 1 at {v}", white(np.full((1, 1), v)), 3, 3, 4) for v in (0, 1, 127, 128, 255)]
    out += [
        ("1 x 37", white(blobs(1, 37)), 3, 0, 4),   # 1 texel wide, no pad: the field that only level 0 holds
        ("37 x 1", white(blobs(37, 1)), 3, 0, 4),
        ("3 x 70", white(blobs(3, 70)), 3, 1, 4),   # crosses tile edges downward
        ("65 x 9", white(blobs(65, 9)), 3, 1, 7),   # ... and across
        ("covered 17 x 17", white(np.full((17, 17), 255)), 3, 0, 32),  # only the plane outside is an edge
        ("empty 9 x 9", white(np.zeros((9, 9))), 3, 2, 4),
        ("byte noise", white(rng.integers(0, 256, size=(40, 40))), 3, 2, 4),
        ("binary noise", white(rng.integers(0, 2, size=(40, 40)) * 255), 3, 4, 8),
        ("half plane", white(half_plane()), 3, 0, 16),
        ("disc", white(disc(**DISC)), 3, 0, 16),
        ("wide disc", white(disc(200, 150, 99.3, 74.6, 70.4, ss=4)), 3, 32, 64),  # the widest window; tiles that take each shortcut
    ]
    odd = rng.integers(0, 256, size=(23, 31, 4)).astype(np.uint8)  # the chosen channel differs from the other three
    odd[..., 1] = disc(31, 23, 14.6, 11.2, 7.7)
    out.append(("channel 1 of 4", np.ascontiguousarray(odd), 1, 3, 6))
    return out


_REFERENCE = {}


def reference(case):
    """the reference's bytes of a case, (h + 2 pad, w + 2 pad) uint8; computed once"""
    name, rgba, channel, pad, R = case
    if name not in _REFERENCE:
        _REFERENCE[name] = REF.field(rgba[..., channel], pad, R)
    return _REFERENCE[name]


def compare(got, want):
    """got: (oh, ow, 4) uint8 texels, want: (oh, ow) bytes -> (texels that differ at all, texels beyond 1 LSB)"""
    d = np.abs(got.astype(int) - want[..., None].astype(int)).max(axis=2)
    return int((d > 0).sum()), int((d > 1).sum())
