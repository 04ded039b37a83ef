"""The sources that the device-image tests share (tests/test_device_image_host.py: the kernel's source under the host shim;
tests/test_device_image.py: the device): sizes at which the tile, the chain and the ink limit change their way, contents, memory layouts,
and every format with and without FDH_IMAGE_STRAIGHT_ALPHA.  A case is (name, format, flags, source, layout); `source` is what
device_image_ref.convert takes."""
import numpy as np

import device_image_ref as REF

SIZES = [(1, 1), (1, 40), (40, 1), (2, 2), (3, 3), (2, 3), (31, 33), (32, 32), (33, 31), (65, 65), (100, 100), (128, 128), (129, 127), (257, 63)]
LARGE = (1025, 1023)  # in an atlas of 2048: the tail goes beyond level 5
LAYOUTS = ("tight", "pitch 16", "pitch 4", "data + 4", "sub-rectangle")


def noise_rgba(rng, w, h):
    """premultiplied-looking noise with translucent, opaque and empty texels"""
    img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
    kind = rng.integers(0, 4, size=(h, w))
    img[kind == 0, 3] = 255
    img[kind == 1] = 0
    return img


def hostile_floats(dtype):
    """0, 1, -0.0, denormals, +-inf, NaN in several spellings, values out of range, and both neighbours of every k + 0.5 product"""
    one = np.array([1.0], dtype)
    special = [0.0, 1.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 2.0, -1.0, 1e-3, 0.5, 255.0, 0.5 / 255.0, 1.5 / 255.0, 254.5 / 255.0]
    v = [np.array(special, dtype)]
    tiny = np.finfo(dtype).tiny
    v.append(np.array([tiny, -tiny, tiny / 2, -tiny / 4, np.finfo(dtype).max, -np.finfo(dtype).max, np.nextafter(one[0], dtype(0)), np.nextafter(one[0], dtype(2))], dtype))
    if dtype == np.float32:
        v.append(np.array([0x7F800001, 0x7FFFFFFF, 0xFF800001, 0xFFC00000, 0x7FC00001, 0x00000001, 0x80000001, 0x007FFFFF], np.uint32).view(np.float32))
    else:
        v.append(np.array([0x7C01, 0x7FFF, 0xFC01, 0xFE00, 0x7E01, 0x0001, 0x8001, 0x03FF], np.uint16).view(np.float16))
    ties = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(dtype)
    v += [ties, np.nextafter(ties, dtype(0)), np.nextafter(ties, dtype(1))]
    return np.concatenate(v)


def float_planes(rng, dtype, channels, w, h):
    """seeded values in [-0.2, 1.2] with the hostile ones strewn among them"""
    v = rng.uniform(-0.2, 1.2, size=(channels, h, w)).astype(dtype)
    hostile = hostile_floats(dtype)
    assert v.size > len(hostile)
    if v.size >= 4 * len(hostile):
        hostile = np.concatenate([hostile, hostile])
    v.reshape(-1)[rng.permutation(v.size)[:len(hostile)]] = hostile
    return v


def all_halves(channels):
    """256 x 256 halves holding all 65 536 bit patterns, plane k the patterns rotated by 12345 k"""
    bits = np.arange(65536, dtype=np.uint32)
    return np.stack([((bits + 12345 * k) & 0xFFFF).astype(np.uint16).view(np.float16).reshape(256, 256) for k in range(channels)])


def all_pairs():
    """256 x 256 RGBA8 holding every (c, a) pair: R = c, G = 255 - c, B = c ^ 0x55, A = a"""
    a, c = np.meshgrid(np.arange(256), np.arange(256))
    return np.stack([c, 255 - c, c ^ 0x55, a], axis=2).astype(np.uint8)


def cases(large=True):
    rng = np.random.default_rng(20261020)
    out = []
    for i, (w, h) in enumerate(SIZES + ([LARGE] if large else [])):
        out.append((f"noise {w} x {h}", REF.RGBA8, i & 1, noise_rgba(rng, w, h), LAYOUTS[i % 5]))
    zero = np.zeros((100, 100, 4), np.uint8)
    corner = zero.copy()
    corner[99, 99] = (3, 200, 17, 129)
    out.append(("all zero", REF.RGBA8, 0, zero, "tight"))
    out.append(("ink in a corner", REF.RGBA8, 0, corner, "pitch 16"))
    fzero = np.zeros((4, 100, 100), np.float32)
    fcorner = fzero.copy()
    fcorner[:, 0, 99] = (0.1, 0.9, 0.3, 0.6)
    out.append(("all zero float32", REF.PLANAR_F32, 0, fzero, "tight"))
    out.append(("ink in a corner float32", REF.PLANAR_F32, 1, fcorner, "data + 4"))
    for j, layout in enumerate(LAYOUTS):
        out.append((f"rgba8 33 x 31 {layout}", REF.RGBA8, j & 1, noise_rgba(rng, 33, 31), layout))
        out.append((f"float32 33 x 31 {layout}", REF.PLANAR_F32, ~j & 1, float_planes(rng, np.float32, (4, 3, 1)[j % 3], 33, 31), layout))
        out.append((f"float16 33 x 31 {layout}", REF.PLANAR_F16, j & 1, float_planes(rng, np.float16, (3, 4, 1)[j % 3], 33, 31), layout))
        out.append((f"rgba8 100 x 36 {layout}", REF.RGBA8, ~j & 1, noise_rgba(rng, 100, 36), layout))
    for flags in (0, 1):
        out.append((f"every half, flags {flags}", REF.PLANAR_F16, flags, all_halves(1), "tight"))
        out.append((f"every half in four planes, flags {flags}", REF.PLANAR_F16, flags, all_halves(4), "pitch 16"))
        out.append((f"every (c, a) pair, flags {flags}", REF.RGBA8, flags, all_pairs(), "tight"))
        for channels in (1, 3, 4):
            out.append((f"float32 {channels} planes 65 x 65, flags {flags}", REF.PLANAR_F32, flags, float_planes(rng, np.float32, channels, 65, 65), LAYOUTS[(channels + flags) % 5]))
            out.append((f"float16 {channels} planes 67 x 34, flags {flags}", REF.PLANAR_F16, flags, float_planes(rng, np.float16, channels, 67, 34), LAYOUTS[(channels + 2 + flags) % 5]))
    return out


def size_of(case):
    src = case[3]
    return (src.shape[1], src.shape[0]) if case[1] == REF.RGBA8 else (src.shape[2], src.shape[1])


def texels(case):
    """the (h, w, 4) uint8 texels the reference makes of the case's source: what fdh_put_image gets on the host path"""
    return REF.convert(case[3], case[1], case[2])


def pack(case):
    """the source in memory -> (bytes from the data pointer to the last element's end, the data pointer's remainder mod 16, pitch_bytes,
    plane_bytes, channels).  What lies between the rows and the planes is seeded garbage."""
    name, fmt, flags, src, layout = case
    planes = src.view(np.uint32).reshape(1, src.shape[0], src.shape[1]) if fmt == REF.RGBA8 else src
    raw = planes.view({4: np.uint32, 2: np.uint16}[planes.dtype.itemsize])
    c, h, w = raw.shape
    es = raw.dtype.itemsize
    row = w * es
    first, align = 0, 0
    if layout == "tight":
        pitch, plane = row, row * h
    elif layout == "pitch 16":
        pitch = (row + 15) // 16 * 16 + 16
        plane = pitch * h + 32
    elif layout == "pitch 4":
        pitch = row + 4
        if pitch % 16 == 0:
            pitch += 4
        plane = pitch * h + 4
    elif layout == "data + 4":
        pitch, plane, align = row, row * h, 4
    else:  # a sub-rectangle at (7, 3) of an image (w + 11) x (h + 5)
        pitch = (w + 11) * es
        plane = pitch * (h + 5)
        first = 3 * pitch + 7 * es
        align = first % 16
    total = (c - 1) * plane + (h - 1) * pitch + row
    rng = np.random.default_rng(len(name) * 7919 + w * 31 + h)
    buf = rng.integers(0, 256, size=total, dtype=np.uint8)
    for k in range(c):
        for y in range(h):
            at = k * plane + y * pitch
            buf[at:at + row] = raw[k, y].view(np.uint8)
    return buf.tobytes(), align, pitch, (plane if fmt != REF.RGBA8 else 0), (c if fmt != REF.RGBA8 else 4)
