"""Images from device memory (fdh_put_image_device, fdh_update_image_device; include_glyphs/figdraw_hip_device_image.h), what a CPU can
check: known answers for the reference tests/device_image_ref.py itself, its chain pinned on the stored levels of img1.flippy; the calls'
rules on a record-only context and through C99; the tensor convenience's layouts; and the source of k_image_import.hip under the host shim
of tests/emu (tests/device_image_emu) against that reference, byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import device_image_cases as DC
import device_image_ref as REF
import emu_build
from conftest import ROOT, load_flippy_levels
from figdraw_amd import context
from figdraw_amd.context import DeviceImage, FigdrawHipError, HipContext

INVALID = -1


# ------------------------------------------------------------------------------------------------------------------ 1. the reference
def test_conversion_known_answers():
    f = np.float32
    assert REF.to_byte(np.array([0.0, 1.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 2.0, -3.0, 0.5], f)).tolist() == [0, 255, 0, 255, 0, 0, 0, 255, 0, 128]
    tiny = np.array([0x00000001, 0x80000001, 0x007FFFFF, 0x00800000], np.uint32).view(f)  # denormals and the smallest normal
    assert not REF.to_byte(tiny).any()
    nans = np.array([0x7F800001, 0x7FFFFFFF, 0xFF800001, 0xFFC00000, 0x7FC00000], np.uint32).view(f)
    assert not REF.to_byte(nans).any()
    # 0.5 * 255 = 127.5 exactly: a tie, to the even byte
    assert REF.to_byte(np.array([0.5], f))[0] == 128 and REF.to_byte(np.array([0.5], np.float16))[0] == 128


def test_conversion_on_both_sides_of_every_tie():
    """v * 255 in float32 against k + 0.5, for the float32 neighbours of (k + 0.5) / 255: the byte is the product's nearest integer, the
    even one where the float32 product IS k + 0.5"""
    for k in range(255):
        centre = np.float32((k + 0.5) / 255.0)
        for v in (np.nextafter(centre, np.float32(0)), centre, np.nextafter(centre, np.float32(1))):
            product = float(np.float32(v) * np.float32(255.0))  # the float32 product, exactly, as a double
            want = k if product < k + 0.5 else k + 1 if product > k + 0.5 else k + (k & 1)
            assert REF.to_byte(np.array([v], np.float32))[0] == want, (k, v)


def test_conversion_of_every_half():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = REF.to_byte(bits.view(np.float16))
    sign, e, m = bits >> 15, (bits >> 10) & 31, bits & 1023
    # the half's value as an exact double, the product in float32 (53 bits hold both exactly), the nearest-even integer by hand
    value = np.where(e == 0, m * 2.0 ** -24, (1024 + m) * 2.0 ** (e.astype(np.float64) - 25)) * np.where(sign == 1, -1.0, 1.0)
    nan, inf = (e == 31) & (m != 0), (e == 31) & (m == 0)
    value[nan] = 0.0
    value[inf] = np.where(sign[inf] == 1, -1.0, 2.0)
    product = (np.clip(value, 0.0, 1.0).astype(np.float32) * np.float32(255.0)).astype(np.float64)
    lo = np.floor(product)
    want = np.where(product - lo > 0.5, lo + 1, np.where(product - lo < 0.5, lo, lo + (lo % 2)))
    assert np.array_equal(got, want.astype(np.uint8))
    assert got[nan].max() == 0 and got[0x3C00] == 255 and got[0x7C00] == 255 and got[0xFC00] == 0 and got[0x8000] == 0


def test_premultiply_every_pair():
    img = DC.all_pairs()
    got = REF.premultiply(img)
    for c in range(0, 256, 5):
        for a in range(0, 256, 3):
            assert got[c, a].tolist() == [c * a // 255, (255 - c) * a // 255, (c ^ 0x55) * a // 255, a]
    c, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal(got[..., 0], c * a // 255) and np.array_equal(got[..., 3], a)
    assert np.array_equal(REF.premultiply(got[:, 255:]), got[:, 255:])  # alpha 255 changes nothing


def test_channel_rules():
    v = np.array([[[0.25, 1.0]]], np.float32)
    assert REF.convert(v, REF.PLANAR_F32).tolist() == [[[64, 64, 64, 255], [255, 255, 255, 255]]]
    rgb = np.array([[[1.0]], [[0.5]], [[0.0]]], np.float32)
    assert REF.convert(rgb, REF.PLANAR_F32, REF.STRAIGHT_ALPHA).tolist() == [[[255, 128, 0, 255]]]
    rgba = np.concatenate([rgb, np.array([[[0.5]]], np.float32)])
    assert REF.convert(rgba, REF.PLANAR_F32).tolist() == [[[255, 128, 0, 128]]]
    assert REF.convert(rgba, REF.PLANAR_F32, REF.STRAIGHT_ALPHA).tolist() == [[[128, 64, 0, 128]]]


def test_chain_is_the_flippy_chain():
    """img1.flippy stores pixie's own minifyBy2 chain of its level 0, 100 x 100 and opaque, written back as straight alpha: the chain made
    here of level 0 (premultiplied: the same bytes), taken back to straight alpha, is the stored one bit for bit down to 4 x 4 -- through the
    odd extents 25, 13 and 7 --, and the premultiply rule takes the stored levels to within 1 of the chain (it rounds down twice)"""
    stored = load_flippy_levels("img1.flippy")
    assert [l.shape[0] for l in stored] == [100, 50, 25, 13, 7, 4, 2, 1] and (stored[0][..., 3] == 255).all()
    mine = REF.chain(REF.premultiply(stored[0]))
    assert len(mine) == 7 and np.array_equal(mine[0], stored[0])
    for l in range(1, 7):
        assert mine[l].shape == stored[l].shape
        a = mine[l][..., 3:4].astype(int)
        straight = np.concatenate([np.where(a > 0, mine[l][..., :3].astype(int) * 255 // np.maximum(a, 1), 0), a], axis=2)
        d = np.abs(straight - stored[l].astype(int))
        assert d.max() <= (0 if stored[l].shape[0] >= 4 else 1), (l, int(d.max()))
        again = mine[l].astype(int) - REF.premultiply(stored[l]).astype(int)
        assert again.min() >= 0 and again.max() <= 1, l
    assert (mine[3][-1, :-1, 3] == 128).all() and mine[3][-1, -1, 3] == 64  # 25 -> 13: the half row and the quarter corner


def test_chain_and_ink_known_answers():
    assert REF.chain(np.zeros((1, 40, 4), np.uint8)) == [] and REF.chain(np.zeros((40, 1, 4), np.uint8)) == []
    assert [l.shape[:2] for l in REF.chain(np.zeros((3, 5, 4), np.uint8))] == [(3, 5), (2, 3)]
    img = np.zeros((3, 3, 4), np.uint8)
    img[..., 0] = [[10, 20, 200], [30, 40, 100], [250, 150, 255]]
    got = REF.minify(img)[..., 0]
    assert got.tolist() == [[25, ((127 * 200 + 128 * 100) // 255) * 128 // 255], [((127 * 250 + 128 * 150) // 255) * 128 // 255, 64 * 255 // 255]]
    ink = np.zeros((5, 7, 4), np.uint8)
    ink[1, 2] = (0, 0, 0, 17)
    ink[3, 5] = (33, 0, 0, 16)
    boxes = REF.ink_boxes(ink)
    assert boxes[0].tolist() == [2, 1, 6, 4] and boxes[1].tolist() == [2, 1, 3, 2] and boxes[2].tolist() == [0, 0, 0, 0]
    assert boxes[8].tolist() == [5, 3, 6, 4] and boxes[10].tolist() == [5, 3, 6, 4] and boxes[11].tolist() == [0, 0, 0, 0]
    assert REF.ink_boxes(np.zeros((129, 2, 4), np.uint8)) is None and REF.ink_boxes(np.zeros((128, 128, 4), np.uint8)) is not None


# ------------------------------------------------------------------------------------------------------------------ 2. the calls
def packed_area(ctx):
    area = C.c_int64()
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(area)) == 0
    return area.value


def image(**kw):
    base = dict(data=0x10000, width=16, height=9, pitch_bytes=64, plane_bytes=0, format=REF.RGBA8, channels=4, flags=0, reserved=0)
    base.update(kw)
    return DeviceImage(**base)


def planar(**kw):
    base = dict(format=REF.PLANAR_F32, channels=3, plane_bytes=64 * 9)
    base.update(kw)
    return image(**base)


REFUSED = [  # (the struct, or None; the text behind the call's name)
    (None, "null image"),
    (image(data=None), "null image"),
    (image(width=0), "empty image"),
    (image(height=-2), "empty image"),
    (image(format=3), "unknown format"),
    (image(flags=2), "unknown flag"),
    (image(flags=1 | 1 << 31), "unknown flag"),
    (image(reserved=7), "reserved must be 0"),
    (image(channels=3), "channels must be 4 for RGBA8 and 1, 3 or 4 for a planar format"),
    (planar(channels=2), "channels must be 4 for RGBA8 and 1, 3 or 4 for a planar format"),
    (planar(channels=0), "channels must be 4 for RGBA8 and 1, 3 or 4 for a planar format"),
    (planar(format=REF.PLANAR_F16, channels=5), "channels must be 4 for RGBA8 and 1, 3 or 4 for a planar format"),
    (image(data=0x10002), "data and pitch_bytes must be multiples of the element size"),
    (image(pitch_bytes=66), "data and pitch_bytes must be multiples of the element size"),
    (planar(data=0x10002), "data and pitch_bytes must be multiples of the element size"),
    (planar(format=REF.PLANAR_F16, data=0x10001), "data and pitch_bytes must be multiples of the element size"),
    (planar(format=REF.PLANAR_F16, pitch_bytes=33), "data and pitch_bytes must be multiples of the element size"),
    (image(pitch_bytes=60), "pitch_bytes is below a row's bytes"),
    (image(pitch_bytes=-64), "pitch_bytes is below a row's bytes"),
    (planar(format=REF.PLANAR_F16, pitch_bytes=30), "pitch_bytes is below a row's bytes"),
    (planar(plane_bytes=64 * 9 - 4), "plane_bytes is below pitch_bytes * height"),
    (planar(plane_bytes=0), "plane_bytes is below pitch_bytes * height"),
    (planar(format=REF.PLANAR_F16, plane_bytes=64 * 9 + 1), "plane_bytes must be a multiple of the element size"),
]


def test_refusals_leave_directory_packer_and_epoch_untouched():
    ctx = HipContext(atlas_size=256, record_only=True)
    L = ctx.L
    assert ctx.put_image_device(7, 0x10000, 16, 9, 64)[2:] == (16, 9)
    out = (C.c_int * 4)()
    before = (ctx.atlas_usage(), packed_area(ctx))
    for i, (img, text) in enumerate(REFUSED):
        ref = C.byref(img) if img is not None else None
        for name, call in (("put_image_device", lambda: L.fdh_put_image_device(ctx.h, 9, ref, out)), ("update_image_device", lambda: L.fdh_update_image_device(ctx.h, 7, ref))):
            assert call() == INVALID, (i, name)
            assert L.fdh_last_error().decode() == f"{name}: {text}", (i, name)
            assert (ctx.atlas_usage(), packed_area(ctx)) == before and not ctx.has_image(9), (i, name)
    for img, text in ((image(), "unknown key"),):
        assert L.fdh_update_image_device(ctx.h, 9, C.byref(img)) == INVALID and L.fdh_last_error().decode() == f"update_image_device: {text}"
    for img in (image(width=15), image(height=10), planar(format=REF.PLANAR_F16, width=8, pitch_bytes=16, plane_bytes=16 * 9)):
        assert L.fdh_update_image_device(ctx.h, 7, C.byref(img)) == INVALID and L.fdh_last_error().decode() == "update_image_device: size mismatch"
    assert (ctx.atlas_usage(), packed_area(ctx)) == before
    # one plane needs no plane stride; a call that goes through moves the epoch, and a put the packer too
    ctx.update_image_device(7, 0x10000, 16, 9, 64, format=REF.PLANAR_F32, channels=1)
    after = ctx.atlas_usage()
    assert after["epoch"] == before[0]["epoch"] + 1 and packed_area(ctx) == before[1]
    assert ctx.put_image_device(9, 0x10000, 16, 9, 32, format=REF.PLANAR_F16, channels=3, plane_bytes=32 * 9)[2:] == (16, 9)
    assert ctx.has_image(9) and packed_area(ctx) > before[1] and ctx.atlas_usage()["epoch"] == after["epoch"] + 1
    ctx.close()


def test_rectangles_pack_like_plain_images():
    """on a record-only context: every put against fdh_put_image of an image of that size on a second context -- the same rectangles, an
    existing key, growth that drops every entry, keep mode -- and a size no atlas takes"""
    for keep in (False, True):
        a, b = HipContext(atlas_size=64, record_only=True), HipContext(atlas_size=64, record_only=True)
        a.set_atlas_keep(keep), b.set_atlas_keep(keep)
        sizes = [(7, 5), (1, 1), (1, 9), (20, 11), (7, 5), (30, 30), (40, 3), (9, 9), (50, 50), (100, 20)]  # the atlas grows on the way
        for key, (w, h) in enumerate(sizes, start=1):
            if key == 5:
                key = 1  # an existing key
            got = a.put_image_device(key, 0x20000, w, h, 2 * w + 2, format=REF.PLANAR_F16, channels=1)
            assert got == b.put_image(key, np.zeros((h, w, 4), np.uint8)) and got[2:] == (w, h)
            assert (a.atlas_usage(), packed_area(a)) == (b.atlas_usage(), packed_area(b))
            assert [a.has_image(k) for k in range(1, 12)] == [b.has_image(k) for k in range(1, 12)]
        assert a.atlas_size() > 64
        codes = []
        for ctx, call in ((a, lambda: a.put_image_device(30, 0x20000, 16400, 2, 65600)), (b, lambda: b.put_image(30, np.zeros((2, 16400, 4), np.uint8)))):
            with pytest.raises(FigdrawHipError) as e:
                call()
            codes.append((e.value.code, ctx.atlas_usage(), packed_area(ctx)))
        assert codes[0] == codes[1] and codes[0][0] == -4
        a.close(), b.close()


def test_update_of_a_flippy_entry_on_a_record_only_context():
    from conftest import GOLDEN

    a, b = HipContext(atlas_size=512, record_only=True), HipContext(atlas_size=512, record_only=True)
    data = open(os.path.join(GOLDEN, "img1.flippy"), "rb").read()
    r = a.put_flippy(3, data)
    assert r == b.put_flippy(3, data)
    a.update_image_device(3, 0x10000, r[2], r[3], 4 * r[2])
    b.update_image(3, np.zeros((r[3], r[2], 4), np.uint8))
    assert a.atlas_usage() == b.atlas_usage()
    assert a.compact_atlas()["rects_moved"] == b.compact_atlas()["rects_moved"]  # both are chain entries now
    a.close(), b.close()


def test_device_image_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "device_image_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_glyphs"),
                           os.path.join(ROOT, "tests", "device_image_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device_image_abi_smoke: OK" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ 3. the tensor convenience
class FakeTensor:
    """what tensor_image asks of a tensor, over a numpy array that stands for device memory"""

    def __init__(self, array, dtype=None):
        self.a, self.dtype, self.shape = array, dtype or f"torch.{array.dtype}", array.shape

    def data_ptr(self):
        return self.a.ctypes.data

    def stride(self):
        return tuple(s // self.a.itemsize for s in self.a.strides)

    def element_size(self):
        return self.a.itemsize


def fields(img):
    return (img.width, img.height, img.pitch_bytes, img.plane_bytes, img.format, img.channels, img.flags, img.reserved)


def test_tensor_layouts():
    T = context.tensor_image
    hwc = np.zeros((9, 16, 4), np.uint8)
    assert fields(T(FakeTensor(hwc))) == (16, 9, 64, 0, REF.RGBA8, 4, 0, 0)
    assert fields(T(FakeTensor(np.zeros((9, 20, 4), np.uint8)[:, 2:18]), True)) == (16, 9, 80, 0, REF.RGBA8, 4, 1, 0)
    chw = np.zeros((3, 9, 16), np.float32)
    assert fields(T(FakeTensor(chw))) == (16, 9, 64, 576, REF.PLANAR_F32, 3, 0, 0)
    assert T(FakeTensor(chw)).data == chw.ctypes.data
    assert fields(T(FakeTensor(np.zeros((4, 12, 20), np.float16)[:, 1:10, 3:19]))) == (16, 9, 40, 480, REF.PLANAR_F16, 4, 0, 0)
    assert fields(T(FakeTensor(np.zeros((9, 16), np.float32)))) == (16, 9, 64, 0, REF.PLANAR_F32, 1, 0, 0)
    assert fields(T(FakeTensor(np.zeros((1, 9, 16), np.float16)))) == (16, 9, 32, 0, REF.PLANAR_F16, 1, 0, 0)
    for bad in (FakeTensor(np.zeros((9, 16, 3), np.uint8)),                              # RGB bytes
                FakeTensor(np.zeros((4, 9, 16), np.uint8)),                              # CHW bytes
                FakeTensor(np.zeros((9, 16, 8), np.uint8)[:, :, ::2]),                   # texels that are not packed
                FakeTensor(np.zeros((16, 9, 4), np.uint8).transpose(1, 0, 2)),           # columns where rows should be
                FakeTensor(np.zeros((9, 16, 3), np.float32).transpose(2, 0, 1)),         # HWC floats seen as CHW: no unit-stride rows
                FakeTensor(np.zeros((2, 9, 16), np.float32)),                            # two planes
                FakeTensor(np.zeros((3, 9, 32), np.float32)[:, :, ::2]),
                FakeTensor(np.broadcast_to(np.zeros((1, 9, 16), np.float32), (3, 9, 16))),  # planes that are one plane
                FakeTensor(np.zeros((3, 9, 16), np.float64)),
                FakeTensor(np.zeros((2, 3, 9, 16), np.float32))):
        with pytest.raises(ValueError):
            T(bad)
    src = open(context.__file__).read()
    assert "import torch" not in src and "from torch" not in src


# ------------------------------------------------------------------------------------------------------------------ 4. the kernel's source
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_image_import.hip compiled as plain C++ under the sequential shim of tests/emu with the driver of tests/device_image_emu -> the
    directory of ./emu and ./emu_san: the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "device_image_emu", ("k_image_import.hip", "fdh_image_import.h"), {"emu": (), "emu_san": emu_build.SAN}, opt="-O2")


def place_of(i, w, h):
    """an entry's place for case i: odd coordinates of every residue, and an atlas that just takes it"""
    x, y = 4 + (i * 7) % 13, 4 + (i * 5) % 11
    size = 16
    while size < max(x + w, y + h) + 4:
        size *= 2
    n_levels = size.bit_length()  # levels size, size / 2, .. 1
    return x, y, size, min(n_levels, 14)


def through_the_shim(tmp, cases, exe="./emu"):
    """-> per case ([the stored levels], the ink block as 64 ints), what the program printed"""
    places = []
    with open(os.path.join(tmp, "cases.bin"), "wb") as f:
        for i, case in enumerate(cases):
            w, h = DC.size_of(case)
            buf, align, pitch, plane, channels = DC.pack(case)
            x, y, size, n_levels = place_of(i, w, h)
            places.append((x, y, size, n_levels))
            f.write(np.array([w, h, case[1], channels, case[2], pitch, plane, align, len(buf), x, y, size, n_levels, 0], np.int32).tobytes())
            f.write(buf)
    r = subprocess.run([exe, "cases.bin", "out.bin"], cwd=tmp, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (exe, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    raw = np.fromfile(os.path.join(tmp, "out.bin"), np.uint8)
    out, at = [], 0
    for case, (x, y, size, n_levels) in zip(cases, places):
        w, h = DC.size_of(case)
        levels = []
        while w > 1 and h > 1 and len(levels) < n_levels:
            levels.append(raw[at:at + w * h * 4].reshape(h, w, 4))
            at += w * h * 4
            w, h = (w + 1) // 2, (h + 1) // 2
        out.append((levels, raw[at:at + 256].view(np.int32)))
        at += 256
    assert at == len(raw)
    return out, r.stdout


def ink_of(block):
    """the host's reading of the ink block: a box whose x1 is still 0 has no texel"""
    boxes = block.reshape(16, 4).astype(np.int64)
    boxes[boxes[:, 2] == 0] = 0
    return boxes


def check(case, got):
    levels, block = got
    want = REF.chain(DC.texels(case))
    assert len(levels) == len(want), case[0]
    for l, (a, b) in enumerate(zip(levels, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{case[0]}: level {l} differs in {int((a != b).any(axis=2).sum())} texels"
    boxes = REF.ink_boxes(DC.texels(case))
    if boxes is None:
        assert block.reshape(16, 4).tolist() == [[32767, 32767, 0, 0]] * 16, case[0]  # untouched
    else:
        assert np.array_equal(ink_of(block), boxes), case[0]


@pytest.fixture(scope="module")
def emulated(shim):
    cases = DC.cases(large=True)
    got, said = through_the_shim(shim, cases)
    print(said.strip())
    return cases, got


def test_the_kernel_source_against_the_reference(emulated):
    """every level of every case and the ink block, byte for byte; the program itself refuses a texel written outside the rectangles"""
    cases, got = emulated
    assert len(cases) > 50
    for case, g in zip(cases, got):
        check(case, g)


def test_nothing_is_stored_of_a_line(emulated):
    cases, got = emulated
    by_name = {c[0]: g for c, g in zip(cases, got)}
    for name in ("noise 1 x 1", "noise 1 x 40", "noise 40 x 1"):
        assert by_name[name][0] == []  # (its ink boxes are measured all the same: check() has compared them)
    assert len(by_name["noise 1025 x 1023"][0]) == 10


def test_the_shim_under_sanitizers(shim, emulated):
    """the stand-alone program built with -fsanitize=address,undefined on every case but the large one: a read past either end of a source
    that ends with its last element, a store outside a level or the level-5 image, is an error there"""
    cases, fields = emulated
    pick = [i for i, c in enumerate(cases) if DC.size_of(c)[0] <= 260]
    assert len(pick) == len(cases) - 1
    got, _ = through_the_shim(shim, [cases[i] for i in pick], exe="./emu_san")
    for i, g in zip(pick, got):
        check(cases[i], g)
