"""Batches of images from device memory (fdh_put_images_device, fdh_update_images_device; include_glyphs/figdraw_hip_device_images.h), what a CPU
can check: the calls' rules on record-only contexts against the single calls and through C99; the tables of fdh_image_batch.h, compiled as
they stand (tests/image_batch_tables_emu), against a painter written here; and the source of the batched kernels of k_image_import.hip under
the host shim of tests/emu (tests/device_images_emu) against the reference tests/device_image_ref.py, byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import device_image_cases as DC
import device_image_ref as REF
import emu_build
from conftest import GOLDEN, ROOT
from figdraw_amd import context
from figdraw_amd.context import DeviceImage, FigdrawHipError, HipContext

INVALID, ATLAS_FULL = -1, -4
CSRC = os.path.join(ROOT, "figdraw_amd", "csrc")
OWNER_LEVEL = 4  # msdf::kOwnerLevel
PAIR = [(4, 4, 100, 100), (112, 4, 100, 100)]  # in an atlas of 256 the two share a column of level 6 (tests/test_device_image.py)


# ------------------------------------------------------------------------------------------------------------------ 1. the calls
def packed_area(ctx):
    area = C.c_int64()
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(area)) == 0
    return area.value


def state(ctx):
    return ctx.atlas_usage(), packed_area(ctx)


def image(**kw):
    base = dict(data=0x10000, width=16, height=9, pitch_bytes=64, plane_bytes=0, format=REF.RGBA8, channels=4, flags=0, reserved=0)
    base.update(kw)
    return DeviceImage(**base)


def planar(**kw):
    base = dict(format=REF.PLANAR_F32, channels=3, plane_bytes=64 * 9)
    base.update(kw)
    return image(**base)


def item(key, w, h):
    return (key, 0x20000, w, h, 4 * w)


def raw_put(ctx, keys, images, n=None, update=False, rects=None):
    """the C call itself -> (the status, the rectangles array)"""
    n = len(keys) if n is None else n
    k = (C.c_int64 * max(len(keys), 1))(*keys)
    arr = (DeviceImage * max(len(images), 1))(*images)
    out = ((C.c_int * 4) * max(len(keys), 1))() if rects is None else rects
    for r in out:
        r[:] = [-7, -7, -7, -7]
    if update:
        return ctx.L.fdh_update_images_device(ctx.h, C.addressof(k), C.addressof(arr), n), out
    return ctx.L.fdh_put_images_device(ctx.h, C.addressof(k), C.addressof(arr), n, C.addressof(out)), out


@pytest.mark.parametrize("order", ["given", "reversed"])
def test_a_batch_packs_like_single_calls(order):
    sizes = DC.SIZES if order == "given" else DC.SIZES[::-1]
    a, b = HipContext(atlas_size=1024, record_only=True), HipContext(atlas_size=1024, record_only=True)
    got = a.put_images_device([item(k, w, h) for k, (w, h) in enumerate(sizes, start=1)])
    want = [b.put_image_device(k, 0x20000, w, h, 4 * w) for k, (w, h) in enumerate(sizes, start=1)]
    assert got == want and [r[2:] for r in got] == sizes
    assert state(a) == state(b) and a.atlas_size() == 1024
    st = a.image_batch_stats()
    assert (st["images"], st["written"], st["dropped_by_growth"], st["launches"], st["bytes_copied"]) == (len(sizes), len(sizes), 0, 0, 0)
    assert st["tiles"] == sum(-(-w // 32) * -(-h // 32) for w, h in sizes if w > 1 and h > 1)
    # an update batch of a permuted subset moves the epoch as the single updates do, and nothing else
    subset = [(k, sizes[k - 1]) for k in (5, 2, 9, 1)]
    a.update_images_device([item(k, w, h) for k, (w, h) in subset])
    for k, (w, h) in subset:
        b.update_image_device(k, 0x20000, w, h, 4 * w)
    assert state(a) == state(b)
    assert a.image_batch_stats()["images"] == 4
    a.close(), b.close()


BAD_STRUCTS = [
    (image(data=None), "null image"),
    (image(width=0), "empty image"),
    (image(height=-2), "empty image"),
    (image(format=3), "unknown format"),
    (image(flags=2), "unknown flag"),
    (image(reserved=7), "reserved must be 0"),
    (image(channels=3), "channels must be 4 for RGBA8 and 1, 3 or 4 for a planar format"),
    (planar(channels=2), "channels must be 4 for RGBA8 and 1, 3 or 4 for a planar format"),
    (image(data=0x10002), "data and pitch_bytes must be multiples of the element size"),
    (planar(format=REF.PLANAR_F16, pitch_bytes=33), "data and pitch_bytes must be multiples of the element size"),
    (image(pitch_bytes=60), "pitch_bytes is below a row's bytes"),
    (planar(plane_bytes=64 * 9 - 4), "plane_bytes is below pitch_bytes * height"),
    (planar(format=REF.PLANAR_F16, plane_bytes=64 * 9 + 1), "plane_bytes must be a multiple of the element size"),
]


def test_refusals_leave_everything_untouched():
    """each rule by its own case, as the LAST image of a batch whose others are good: nothing is placed, begun or bumped, out_rects is not
    written, and the stats stay those of the last batch that passed"""
    ctx = HipContext(atlas_size=256, record_only=True)
    L = ctx.L
    good = [image(), planar(), image(width=8, height=2, pitch_bytes=32)]
    assert ctx.put_images_device(zip((1, 2, 3), good)) and ctx.image_batch_stats()["images"] == 3
    before, stats = state(ctx), ctx.image_batch_stats()

    def refused(code_and_rects, who, text):
        code, rects = code_and_rects
        assert code == INVALID and L.fdh_last_error().decode() == f"{who}: {text}", (who, text, code, L.fdh_last_error())
        assert state(ctx) == before and ctx.image_batch_stats() == stats and not ctx.has_image(9), (who, text)
        assert all(list(r) == [-7] * 4 for r in rects), (who, text)

    for update, who in ((False, "put_images_device"), (True, "update_images_device")):
        keys = [1, 2, 3] if update else [7, 8, 9]
        refused(raw_put(ctx, keys, good, n=-1, update=update), who, "bad image array")
        k = (C.c_int64 * 3)(*keys)
        arr = (DeviceImage * 3)(*good)
        for a, b in ((None, C.addressof(arr)), (C.addressof(k), None)):
            code = L.fdh_update_images_device(ctx.h, a, b, 3) if update else L.fdh_put_images_device(ctx.h, a, b, 3, None)
            refused((code, []), who, "bad image array")
        for bad, text in BAD_STRUCTS:
            refused(raw_put(ctx, keys, good[:2] + [bad], update=update), who, text)
        refused(raw_put(ctx, [keys[0], keys[1], keys[0]], good[:2] + [good[0]], update=update), who, "a key occurs twice")
        wide = image(width=2049, height=2, pitch_bytes=4 * 2049)
        high = image(width=2, height=2049, pitch_bytes=8)
        for big in (wide, high):
            refused(raw_put(ctx, keys, good[:2] + [big], update=update), who, "an image of a batch is at most 2048 x 2048")
    refused(raw_put(ctx, [1, 2, 9], good, update=True), "update_images_device", "unknown key")
    refused(raw_put(ctx, [1, 2, 3], good[:2] + [image(width=8, height=3, pitch_bytes=32)], update=True), "update_images_device", "size mismatch")
    refused(raw_put(ctx, [3, 2, 1], good, update=True), "update_images_device", "size mismatch")  # (the first image already)
    # the limits on the batch as a whole
    many = [image()] * 65536
    code, _ = raw_put(ctx, list(range(100, 100 + 65536)), many)
    refused((code, []), "put_images_device", "at most 65535 images")
    full = image(width=2048, height=2048, pitch_bytes=8192)
    code, _ = raw_put(ctx, list(range(100, 165)), [full] * 64 + [image(width=1, height=1, pitch_bytes=4)])  # 64 * 4096 + 1 tiles
    refused((code, []), "put_images_device", "at most 2^18 tiles in a batch")
    # and a batch that passes moves on: the epoch by one per image, the stats to its own
    assert raw_put(ctx, [1, 2, 3], good, update=True)[0] == 0
    assert ctx.atlas_usage()["epoch"] == before[0]["epoch"] + 3 and packed_area(ctx) == before[1]
    ctx.close()


def test_exactly_two_to_the_18_tiles_pass_validation():
    ctx = HipContext(atlas_size=256, record_only=True)
    full = image(width=2048, height=2048, pitch_bytes=8192)
    code, _ = raw_put(ctx, list(range(1, 65)), [full] * 64)
    assert code == ATLAS_FULL  # 49 of them fill 16384 x 16384: the batch was placed, not refused
    assert ctx.image_batch_stats()["images"] == 64
    ctx.close()


def test_an_empty_batch():
    ctx = HipContext(atlas_size=256, record_only=True)
    before = state(ctx)
    assert ctx.put_images_device([]) == [] and ctx.update_images_device([]) is None
    assert ctx.L.fdh_put_images_device(ctx.h, None, None, 0, None) == 0 and ctx.L.fdh_update_images_device(ctx.h, None, None, 0) == 0
    assert state(ctx) == before
    ctx.close()


def test_growth_in_the_middle_of_a_batch():
    """an atlas of 256 and a batch that needs 512: the images before the one that grows the atlas are gone, as after single calls"""
    sizes = [(100, 100), (100, 100), (60, 60), (120, 120), (90, 40), (33, 31)]
    a, b = HipContext(atlas_size=256, record_only=True), HipContext(atlas_size=256, record_only=True)
    assert a.put_image_device(50, 0x20000, 20, 20, 80) == b.put_image_device(50, 0x20000, 20, 20, 80)
    got = a.put_images_device([item(k, w, h) for k, (w, h) in enumerate(sizes, start=1)])
    want = [b.put_image_device(k, 0x20000, w, h, 4 * w) for k, (w, h) in enumerate(sizes, start=1)]
    assert got == want and a.atlas_size() == b.atlas_size() == 512 and state(a) == state(b)
    alive = [a.has_image(k) for k in range(1, 7)]
    assert alive == [b.has_image(k) for k in range(1, 7)] and not a.has_image(50) and not alive[0] and alive[-1]
    st = a.image_batch_stats()
    assert st["dropped_by_growth"] == alive.count(False) > 0 and st["written"] == alive.count(True) and st["images"] == 6
    a.close(), b.close()


def test_atlas_full_keeps_the_images_before():
    """50 images of 2048 x 2048: 49 fill an atlas of 16384, the fiftieth has no place"""
    a, b = HipContext(atlas_size=16384, record_only=True), HipContext(atlas_size=16384, record_only=True)
    n = 50
    with pytest.raises(FigdrawHipError) as e:
        a.put_images_device([(k, 0x20000, 2048, 2048, 8192) for k in range(1, n + 1)])
    assert e.value.code == ATLAS_FULL
    failed_at = None
    for k in range(1, n + 1):
        try:
            b.put_image_device(k, 0x20000, 2048, 2048, 8192)
        except FigdrawHipError as err:
            assert err.code == ATLAS_FULL
            failed_at = k
            break
    assert failed_at == 50 and state(a) == state(b)
    assert [a.has_image(k) for k in range(1, n + 1)] == [True] * 49 + [False]
    st = a.image_batch_stats()
    assert (st["images"], st["written"], st["dropped_by_growth"]) == (50, 49, 0)
    a.close(), b.close()


def test_keep_mode_makes_room_once():
    a = HipContext(atlas_size=256, record_only=True)
    a.set_atlas_keep(True)
    for k, (w, h) in enumerate([(100, 100), (60, 60), (20, 20)], start=50):
        a.put_image_device(k, 0x20000, w, h, 4 * w)
    before = a.atlas_usage()
    sizes = [(100, 100), (120, 120), (90, 40), (100, 100), (33, 31)]
    got = a.put_images_device([item(k, w, h) for k, (w, h) in enumerate(sizes, start=1)])
    after = a.atlas_usage()
    assert after["size"] > 256 and after["compactions"] == before["compactions"] + 1 and after["rebuilds"] == before["rebuilds"]
    assert all(a.has_image(k) for k in (50, 51, 52, 1, 2, 3, 4, 5)) and [a.image_rect(k) for k in range(1, 6)] == got
    st = a.image_batch_stats()
    assert (st["written"], st["dropped_by_growth"]) == (5, 0)
    a.close()


def test_update_batch_of_a_flippy_entry():
    a, b = HipContext(atlas_size=512, record_only=True), HipContext(atlas_size=512, record_only=True)
    data = open(os.path.join(GOLDEN, "img1.flippy"), "rb").read()
    r = a.put_flippy(3, data)
    assert r == b.put_flippy(3, data)
    assert a.put_image_device(4, 0x10000, 30, 20, 120) == b.put_image_device(4, 0x10000, 30, 20, 120)
    a.update_images_device([(4, 0x10000, 30, 20, 120), (3, 0x10000, r[2], r[3], 4 * r[2])])
    b.update_image_device(4, 0x10000, 30, 20, 120)
    b.update_image(3, np.zeros((r[3], r[2], 4), np.uint8))
    assert a.atlas_usage() == b.atlas_usage()
    assert a.compact_atlas()["rects_moved"] == b.compact_atlas()["rects_moved"]  # both are chain entries now
    a.close(), b.close()


def test_device_images_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "device_images_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_glyphs"),
                           os.path.join(ROOT, "tests", "device_images_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device_images_abi_smoke: OK" in r.stdout


def test_the_binding_knows_the_struct_and_cuts_a_tensor_without_a_copy():
    ctx = HipContext(atlas_size=256, record_only=True)
    assert ctx.L.fdh_sizeof_device_image() == C.sizeof(DeviceImage)
    ctx.close()

    class Fake:
        def __init__(self, a):
            self.a, self.dtype, self.shape = a, f"torch.{a.dtype}", a.shape

        def data_ptr(self):
            return self.a.ctypes.data

        def stride(self):
            return tuple(s // self.a.itemsize for s in self.a.strides)

        def element_size(self):
            return self.a.itemsize

    nchw = np.zeros((5, 3, 12, 20), np.float16)[:, :, 1:10, 2:18]
    imgs = context.tensor_images(Fake(nchw))
    assert [i.data for i in imgs] == [nchw[k].ctypes.data for k in range(5)]
    assert {(i.width, i.height, i.pitch_bytes, i.plane_bytes, i.format, i.channels) for i in imgs} == {(16, 9, 40, 480, REF.PLANAR_F16, 3)}
    nhwc = np.zeros((3, 9, 16, 4), np.uint8)
    imgs = context.tensor_images(Fake(nhwc), True)
    assert [(i.data, i.width, i.height, i.pitch_bytes, i.format, i.flags) for i in imgs] == [(nhwc[k].ctypes.data, 16, 9, 64, REF.RGBA8, 1) for k in range(3)]
    assert len(context.tensor_images([Fake(nhwc[0]), Fake(nchw[1])])) == 2
    with pytest.raises(ValueError):
        context.tensor_images(Fake(nchw[0]))


# ------------------------------------------------------------------------------------------------------------------ 2. the tables
def level_size(v, l):
    return (v + (1 << l) - 1) >> l


def deep_levels(g, n_levels):
    """the levels from OWNER_LEVEL on that store texels of the image"""
    out = []
    for l in range(OWNER_LEVEL, n_levels):
        if not (level_size(g[2], l) > 1 and level_size(g[3], l) > 1):
            break
        out.append(l)
    return out


def restated(n_levels, first, m, images):
    """images: (x, y, w, h, format) -> the tables by brute force; the owner of a texel is its last painter"""
    part = images[first:first + m]
    records, tiles_of, owner_words, scratch, ink_blocks = [], [], 0, 0, 0
    for k, (x, y, w, h, fmt) in enumerate(part):
        n_store = 0
        while n_store < n_levels and level_size(w, n_store) > 1 and level_size(h, n_store) > 1:
            n_store += 1
        tw, th = (level_size(w, 5), level_size(h, 5)) if w > 1 and h > 1 else (0, 0)
        ink = int(tw * th > 0 and w <= 128 and h <= 128)
        records.append(dict(x=x, y=y, w=w, h=h, n_store=n_store, ink=ink, scratch_off=scratch, ink_off=ink_blocks, owner_off=owner_words * 32,
                            lw=[level_size(w, l) for l in range(6)], lh=[level_size(h, l) for l in range(6)]))
        tiles_of.append([k | tx << 16 | ty << 22 for ty in range(th) for tx in range(tw)])
        scratch += tw * th
        ink_blocks += tw * th * ink
        owner_words += (sum(level_size(w, l) * level_size(h, l) for l in deep_levels(part[k], n_levels)) + 31) // 32
    groups, tile_words = [], []
    for fmt in range(3):
        words = [t for k, g in enumerate(part) if g[4] == fmt for t in tiles_of[k]]
        groups += [len(tile_words), len(words)]
        tile_words += words
    owner = [0] * (owner_words + 1)
    for l in range(OWNER_LEVEL, n_levels):
        painted = {}
        for k, g in enumerate(part):
            if l in deep_levels(g, n_levels):
                for j in range(level_size(g[3], l)):
                    for i in range(level_size(g[2], l)):
                        painted[((g[0] >> l) + i, (g[1] >> l) + j)] = k
        for k, g in enumerate(part):
            if l not in deep_levels(g, n_levels):
                continue
            bit = records[k]["owner_off"] + sum(level_size(g[2], d) * level_size(g[3], d) for d in range(OWNER_LEVEL, l))
            for j in range(level_size(g[3], l)):
                for i in range(level_size(g[2], l)):
                    if painted[((g[0] >> l) + i, (g[1] >> l) + j)] == k:
                        owner[bit >> 5] |= 1 << (bit & 31)
                    bit += 1
    return dict(records=records, tiles=tile_words, groups=groups, tails=[k for k, r in enumerate(records) if r["n_store"] > 6], owner=owner, ink_blocks=ink_blocks)


F = (REF.RGBA8, REF.PLANAR_F32, REF.PLANAR_F16)
MIXED = [(4, 4, 12, 11), (24, 4, 100, 70), (132, 4, 12, 11), (152, 4, 70, 129), (4, 141, 300, 40), (4, 189, 1, 40), (13, 189, 40, 1)]
TABLE_CASES = {  # name -> (n_levels, first, m, [(x, y, w, h, format)])
    "the level-6 pair": (9, 0, 2, [g + (REF.RGBA8,) for g in PAIR]),
    "the level-6 pair, the other way round": (9, 0, 2, [g + (REF.PLANAR_F32,) for g in PAIR[::-1]]),
    "three, the middle one 1 texel high": (9, 0, 3, [(4, 4, 100, 100, 0), (112, 4, 100, 1, 2), (112, 13, 100, 90, 1)]),
    "formats that alternate": (10, 0, 7, [g + (F[k % 3],) for k, g in enumerate(MIXED)]),
    "formats that alternate the other way": (10, 0, 7, [g + (F[(2 * k + 1) % 3],) for k, g in enumerate(MIXED)]),
    "one format": (10, 0, 7, [g + (REF.PLANAR_F16,) for g in MIXED]),
    "a batch cut at first = 2": (10, 2, 4, [g + (F[k % 3],) for k, g in enumerate(MIXED)]),
    "an atlas of 6 levels": (6, 0, 5, [g + (F[k % 2],) for k, g in enumerate(MIXED[:5])]),
    "a 2048 x 34 image beside a small one": (13, 0, 2, [(4, 4, 2048, 34, 0), (4, 46, 40, 40, 0)]),
}


@pytest.fixture(scope="module")
def table_programs(tmp_path_factory):
    """tests/image_batch_tables_emu/main.cpp with g++ alone, fdh_image_batch.h and what it includes beside it -> the directory of `tables` and
    of `tables_san`"""
    return emu_build.build(tmp_path_factory, "image_batch_tables_emu", ("fdh_image_batch.h", "fdh_image_import.h", "fdh_glyph_tables.h", "fdh_msdf_host.h"),
                           {"tables": (), "tables_san": emu_build.SAN}, source="main.cpp")


def test_the_header_is_plain():
    import re
    text = open(os.path.join(CSRC, "fdh_image_batch.h")).read()
    assert set(re.findall(r'#include "([^"]+)"', text)) == {"fdh_glyph_tables.h", "fdh_image_import.h"}
    assert "hip" not in " ".join(re.findall(r"#include <([^>]+)>", text))


@pytest.mark.parametrize("exe", ["tables", "tables_san"])
@pytest.mark.parametrize("case", list(TABLE_CASES))
def test_tables_are_the_painters(table_programs, exe, case):
    n_levels, first, m, images = TABLE_CASES[case]
    src = os.path.join(table_programs, f"{exe}.txt")
    with open(src, "w") as f:
        f.write(f"{n_levels} {first} {m} {len(images)}\n" + "".join("%d %d %d %d %d\n" % g for g in images))
    r = subprocess.run([os.path.join(table_programs, exe), src], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"{r.returncode} {r.stdout}{r.stderr}"
    lines = r.stdout.splitlines()
    want = restated(n_levels, first, m, images)
    n_tiles, n_tails = len(want["tiles"]), len(want["tails"])
    words = m * 32 + n_tiles + n_tails + len(want["owner"])
    assert lines[1] == f"n_tiles {n_tiles} n_tails {n_tails} ink_blocks {want['ink_blocks']} words {words} at {m * 32} {m * 32 + n_tiles} {m * 32 + n_tiles + n_tails}"
    assert [int(v) for v in lines[2].split()[1:]] == want["groups"]
    for k, g in enumerate(want["records"]):
        assert lines[3 + k] == ("image %d at %d %d size %d %d n_store %d ink %d scratch_off %d ink_off %d owner_off %d" % (k, g["x"], g["y"], g["w"], g["h"], g["n_store"], g["ink"],
                                g["scratch_off"], g["ink_off"], g["owner_off"]) + " lw " + " ".join(map(str, g["lw"])) + " lh " + " ".join(map(str, g["lh"])))
    got_tiles = [int(v) for v in lines[3 + m].split()[1:]]
    assert got_tiles == want["tiles"]
    assert [int(v) for v in lines[4 + m].split()[1:]] == want["tails"]
    assert [int(v) for v in lines[5 + m].split()[1:]] == want["owner"]
    # every tile is named once, and a format's tiles lie together
    part = images[first:first + m]
    named = sorted((t & 0xFFFF, (t >> 16) & 63, t >> 22) for t in got_tiles)
    assert named == sorted((k, tx, ty) for k, g in enumerate(part) if g[2] > 1 and g[3] > 1 for ty in range(level_size(g[3], 5)) for tx in range(level_size(g[2], 5)))
    formats = [part[t & 0xFFFF][4] for t in got_tiles]
    assert formats == sorted(formats)
    # what is reserved before the first placement -- for all images, in an atlas of that many levels -- holds what is copied
    whole = restated(n_levels, 0, len(images), images)
    assert int(lines[0].split()[1]) == len(images) * 33 + len(whole["tiles"]) + len(whole["owner"]) >= words


def test_the_table_cases_can_go_wrong():
    a = restated(*TABLE_CASES["the level-6 pair"])
    bits = lambda t: sum(bin(w).count("1") for w in t["owner"])  # noqa: E731
    per_image = 7 * 7 + 4 * 4 + 2 * 2  # levels 4, 5 and 6 of a 100 x 100 image
    assert bits(a) == 2 * per_image - 4 - 2  # the shared columns of levels 5 and 6, four texels and two, belong to the later image alone
    b = restated(*TABLE_CASES["the level-6 pair, the other way round"])
    assert bits(b) == bits(a) and a["owner"] != b["owner"] and a["tails"] == [0, 1]
    thin = restated(*TABLE_CASES["three, the middle one 1 texel high"])
    assert [r["n_store"] for r in thin["records"]] == [7, 0, 7] and len(thin["tiles"]) == 16 + 12 and thin["groups"] == [0, 16, 16, 12, 28, 0]
    alt = restated(*TABLE_CASES["formats that alternate"])
    assert all(n > 0 for n in alt["groups"][1::2]) and [t & 0xFFFF for t in alt["tiles"]] != sorted(t & 0xFFFF for t in alt["tiles"])
    assert restated(*TABLE_CASES["a 2048 x 34 image beside a small one"])["records"][0]["lw"][5] == 64


# ------------------------------------------------------------------------------------------------------------------ 3. the kernels' source
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_image_import.hip compiled as plain C++ under the sequential shim of tests/emu with the driver of tests/device_images_emu -> the
    directory of ./emu and ./emu_san: the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "device_images_emu", ("k_image_import.hip", "fdh_image_import.h", "fdh_image_batch.h", "fdh_glyph_tables.h", "fdh_msdf_host.h"),
                           {"emu": (), "emu_san": emu_build.SAN}, opt="-O2")


def run_batch(tmp, exe, cases, rects, size):
    """-> ([the levels' first rows as (rows, size >> l, 4) uint8], [per image its folded ink block], what the program printed)"""
    n_levels = min(size.bit_length(), 14)
    out_rows = max(y + h for _, y, _, h in rects)
    with open(os.path.join(tmp, "batch.bin"), "wb") as f:
        f.write(np.array([len(cases), size, n_levels, out_rows], np.int32).tobytes())
        for case, (x, y, w, h) in zip(cases, rects):
            assert (w, h) == DC.size_of(case)
            buf, align, pitch, plane, channels = DC.pack(case)
            f.write(np.array([w, h, case[1], channels, case[2], pitch, plane, align, len(buf), x, y, 0], np.int32).tobytes())
            f.write(buf)
    r = subprocess.run([exe, "batch.bin", "out.bin"], cwd=tmp, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (exe, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    raw = np.fromfile(os.path.join(tmp, "out.bin"), np.uint8)
    levels, at = [], 0
    for l in range(n_levels):
        LS = size >> l
        rows = min(LS, (out_rows >> l) + 2)
        levels.append(raw[at:at + rows * LS * 4].reshape(rows, LS, 4))
        at += rows * LS * 4
    inks = [raw[at + 256 * k:at + 256 * (k + 1)].view(np.int32) for k in range(len(cases))]
    assert at + 256 * len(cases) == len(raw)
    return levels, inks, r.stdout


def expected(cases, rects, size, shapes):
    """the atlas after single puts in array order, by the reference: the later image wins a shared texel"""
    levels = [np.full(s, 0xEE, np.uint8) for s in shapes]
    for case, (x, y, w, h) in zip(cases, rects):
        for l, img in enumerate(REF.chain(DC.texels(case), len(shapes))):
            levels[l][(y >> l):(y >> l) + img.shape[0], (x >> l):(x >> l) + img.shape[1]] = img
    return levels


def check_batch(cases, rects, size, got):
    levels, inks, _ = got
    want = expected(cases, rects, size, [l.shape for l in levels])
    for l, (a, b) in enumerate(zip(levels, want)):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero((a != b).any(axis=2))
            raise AssertionError(f"level {l} differs in {len(xs)} texels, the first at ({xs[0]}, {ys[0]}): {a[ys[0], xs[0]]} != {b[ys[0], xs[0]]}")
    for case, (x, y, w, h), block in zip(cases, rects, inks):
        boxes = REF.ink_boxes(DC.texels(case))
        if boxes is None or w == 1 or h == 1:  # (a line has no tile: the host measures its boxes, Importer::make)
            assert block.reshape(16, 4).tolist() == [[32767, 32767, 0, 0]] * 16, case[0]
        else:
            got_boxes = block.reshape(16, 4).astype(np.int64)
            got_boxes[got_boxes[:, 2] == 0] = 0
            assert np.array_equal(got_boxes, boxes), case[0]


@pytest.fixture(scope="module")
def mixed_batch():
    """all of cases(large=False), a 2048 x 34 image -- the widest level-5 row, 64 texels, of a chain that ends there -- and a 2048 x 66 one,
    whose level-5 image of 64 x 3 the tail takes on, with the places a record-only context gives them in an atlas of 4096"""
    cases = DC.cases(large=False)
    cases.insert(7, ("noise 2048 x 34", REF.RGBA8, 1, DC.noise_rgba(np.random.default_rng(5), 2048, 34), "pitch 16"))
    cases.insert(20, ("noise 2048 x 66", REF.RGBA8, 0, DC.noise_rgba(np.random.default_rng(6), 2048, 66), "data + 4"))
    ctx = HipContext(atlas_size=4096, record_only=True)
    rects = ctx.put_images_device([(k,) + (0x20000,) + DC.size_of(c) + (4 * DC.size_of(c)[0],) for k, c in enumerate(cases)])
    assert ctx.atlas_size() == 4096
    ctx.close()
    return cases, rects


def pair_cases():
    rng = np.random.default_rng(11)
    return [("a", REF.RGBA8, 0, DC.noise_rgba(rng, 100, 100), "tight"), ("b", REF.PLANAR_F32, 1, DC.float_planes(rng, np.float32, 4, 100, 100), "pitch 4")]


@pytest.fixture(scope="module")
def emulated(shim, mixed_batch):
    cases, rects = mixed_batch
    got = run_batch(shim, "./emu", cases, rects, 4096)
    print(got[2].strip())
    return got


def test_the_mixed_batch_against_the_reference(mixed_batch, emulated):
    cases, rects = mixed_batch
    assert len(cases) > 50 and {c[1] for c in cases} == {0, 1, 2} and {c[4] for c in cases} == set(DC.LAYOUTS) and {c[2] for c in cases} == {0, 1}
    assert "launches 4" in emulated[2]  # three formats and the tails
    check_batch(cases, rects, 4096, emulated)
    x, y, w, h = rects[20]
    assert (w, h) == (2048, 66) and (emulated[0][6][y >> 6:(y >> 6) + 2, x >> 6:(x >> 6) + 32] != 0xEE).all()  # its level 6, 32 x 2, is the tail's


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_the_level_6_pair(shim, order):
    """the later image of the array wins the shared column, whichever of the two it is"""
    both = pair_cases()
    cases, rects = [both[k] for k in order], [PAIR[k] for k in order]
    got = run_batch(shim, "./emu", cases, rects, 256)
    check_batch(cases, rects, 256, got)
    one = expected(cases[:1], rects[:1], 256, [l.shape for l in got[0]])[6]
    assert not np.array_equal(one[0:2, 0:4], got[0][6][0:2, 0:4])  # (the second image did change level 6 of the first)
    san = run_batch(shim, "./emu_san", cases, rects, 256)
    assert all(np.array_equal(a, b) for a, b in zip(got[0], san[0])) and all(np.array_equal(a, b) for a, b in zip(got[1], san[1]))


def test_the_mixed_batch_under_sanitizers(shim, mixed_batch, emulated):
    """the stand-alone program built with -fsanitize=address,undefined: a read past either end of a source, of the tables, a store outside a
    level, the scratch or the ink blocks is an error there; the bytes are the plain build's"""
    cases, rects = mixed_batch
    san = run_batch(shim, "./emu_san", cases, rects, 4096)
    assert all(np.array_equal(a, b) for a, b in zip(emulated[0], san[0])) and all(np.array_equal(a, b) for a, b in zip(emulated[1], san[1]))
