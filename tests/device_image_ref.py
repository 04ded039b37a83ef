"""Images from device memory (fdh_put_image_device, fdh_update_image_device): the text of include_glyphs/figdraw_hip_device_image.h in numpy --
the conversion to the RGBA8 texel, the premultiplication, the level chain and the ink boxes.  Written from that comment, not from the C++;
the chain is pinned on the stored levels of tests/golden/img1.flippy (tests/test_device_image_host.py)."""
import numpy as np

RGBA8, PLANAR_F32, PLANAR_F16 = 0, 1, 2
STRAIGHT_ALPHA = 1
INK_MAX = 128


def to_byte(v):
    """a planar value (float32, or float16: widened first, which is exact) -> the byte: NaN gives 0, any other value
    rint(min(max(v, 0), 1) * 255) in float32, ties to even"""
    v = np.asarray(v)
    assert v.dtype in (np.float32, np.float16)
    v = v.astype(np.float32)
    nan = np.isnan(v)
    c = np.minimum(np.maximum(np.where(nan, np.float32(0), v), np.float32(0)), np.float32(1))
    scaled = c * np.float32(255.0)
    assert scaled.dtype == np.float32
    return np.rint(scaled).astype(np.uint8)  # (np.rint: to the nearest, ties to even)


def premultiply(rgba):
    """each colour byte becomes (c * a) / 255, an integer division"""
    out = rgba.copy()
    a = rgba[..., 3].astype(np.uint32)
    for k in range(3):
        out[..., k] = (rgba[..., k].astype(np.uint32) * a // 255).astype(np.uint8)
    return out


def convert(src, fmt, flags=0):
    """the (h, w, 4) uint8 texels of a source: (h, w, 4) uint8 for RGBA8, (channels, h, w) float32 / float16 for the planar formats"""
    if fmt == RGBA8:
        assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 4
        rgba = src.copy()
    else:
        assert src.dtype == (np.float32 if fmt == PLANAR_F32 else np.float16) and src.ndim == 3 and src.shape[0] in (1, 3, 4)
        b = to_byte(src)
        c, h, w = b.shape
        rgba = np.full((h, w, 4), 255, np.uint8)
        if c == 1:
            rgba[..., 0] = rgba[..., 1] = rgba[..., 2] = b[0]
        else:
            for k in range(c):
                rgba[..., k] = b[k]
    return premultiply(rgba) if flags & STRAIGHT_ALPHA else rgba


def minify(img):
    """one level from the one before: the sum of a 2 x 2 block div 4; the extra column, row and corner of odd extents"""
    h, w = img.shape[:2]
    nh, nw, fh, fw = (h + 1) // 2, (w + 1) // 2, h // 2, w // 2
    s = img.astype(np.uint32)
    out = np.zeros((nh, nw, 4), np.uint32)
    out[:fh, :fw] = (s[0:2 * fh:2, 0:2 * fw:2] + s[0:2 * fh:2, 1:2 * fw:2] + s[1:2 * fh:2, 0:2 * fw:2] + s[1:2 * fh:2, 1:2 * fw:2]) // 4
    if w % 2:
        a, b = s[0:2 * fh:2, w - 1], s[1:2 * fh:2, w - 1]
        out[:fh, nw - 1] = ((127 * a + 128 * b) // 255) * 128 // 255
    if h % 2:
        a, b = s[h - 1, 0:2 * fw:2], s[h - 1, 1:2 * fw:2]
        out[nh - 1, :fw] = ((127 * a + 128 * b) // 255) * 128 // 255
    if w % 2 and h % 2:
        out[nh - 1, nw - 1] = 64 * s[h - 1, w - 1] // 255
    return out.astype(np.uint8)


def chain(img, n_levels=14):
    """the stored levels: level l is ceil(w / 2^l) x ceil(h / 2^l) while both extents exceed 1 -- none at all of an image 1 texel wide or high"""
    levels = []
    while img.shape[0] > 1 and img.shape[1] > 1 and len(levels) < n_levels:
        levels.append(img)
        img = minify(img)
    return levels


def ink_boxes(img):
    """(16, 4) ints {x0, y0, x1, y1}: for k = 0 .. 7 the bounding box of texels whose alpha exceeds 16 k, then of those whose largest colour
    channel does; an empty box is {0, 0, 0, 0}.  None for an image wider or higher than 128."""
    h, w = img.shape[:2]
    if w > INK_MAX or h > INK_MAX:
        return None
    boxes = np.zeros((16, 4), np.int64)
    for kind, value in enumerate((img[..., 3], img[..., :3].max(axis=2))):
        for k in range(8):
            ys, xs = np.nonzero(value > 16 * k)
            if len(xs):
                boxes[kind * 8 + k] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return boxes
