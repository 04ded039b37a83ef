"""Batches of decoded video frames (fdh_put_video_frames, fdh_update_video_frames; include_glyphs/figdraw_hip_video_frames.h), what a CPU can
check: the calls' rules on record-only contexts against the single calls and through C99; the tables of fdh_video_batch.h, compiled as they
stand (tests/video_batch_tables_emu), against a painter written here; and the source of the batched kernels of k_video_import.hip, with
k_image_import_tail_batch, under the host shim of tests/emu (tests/video_frames_emu) against the reference tests/video_frame_ref.py and the
host chain, byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emu_build
import video_frame_cases as VC
import video_frame_ref as REF
from conftest import GOLDEN, ROOT
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext, VideoFrame
from test_video_frame_host import REFUSED, bgra, frame, p010, packed_area

INVALID, ATLAS_FULL = -1, -4
CSRC = os.path.join(ROOT, "figdraw_amd", "csrc")
OWNER_LEVEL = 4  # msdf::kOwnerLevel
PAIR = [(4, 4, 100, 100), (112, 4, 100, 100)]  # in an atlas of 256 the two share a column of level 6


# ------------------------------------------------------------------------------------------------------------------ 1. the calls
def state(ctx):
    return ctx.atlas_usage(), packed_area(ctx)


def digest_of_a_frame(ctx, keys):
    """a frame that draws every entry that is still in the atlas once, at its own size -> the digest of its records (the rectangles are in them)"""
    ctx.begin_frame(1600, 1200, True, (0.1, 0.2, 0.3, 1.0))
    for i, k in enumerate(keys):
        if ctx.has_image(k):
            r = ctx.image_rect(k)
            ctx.draw_image(k, (3.0 + 37 * (i % 40), 5.0 + 90 * (i // 40)), [(255, 255, 255, 255)] * 4, (float(r[2]), float(r[3])))
    ctx.end_frame()
    return ctx.record_digest()


def item(key, w, h):
    """an NV12 frame at made-up addresses (a record-only context reads nothing)"""
    return (key, 0x20000, 0x40000, w, h, w + 3, 2 * ((w + 1) // 2) + 2)


def single_put(ctx, it, update=False):
    return (ctx.update_video_frame if update else ctx.put_video_frame)(*it)


def raw_put(ctx, keys, frames, n=None, update=False):
    """the C call itself -> (the status, the rectangles array)"""
    n = len(keys) if n is None else n
    k = (C.c_int64 * max(len(keys), 1))(*keys)
    arr = (VideoFrame * max(len(frames), 1))()
    for i, f in enumerate(frames):
        C.memmove(C.byref(arr, i * C.sizeof(VideoFrame)), C.byref(f), C.sizeof(VideoFrame))
    out = ((C.c_int * 4) * max(len(keys), 1))()
    for r in out:
        r[:] = [-7, -7, -7, -7]
    if update:
        return ctx.L.fdh_update_video_frames(ctx.h, C.addressof(k), C.addressof(arr), n), out
    return ctx.L.fdh_put_video_frames(ctx.h, C.addressof(k), C.addressof(arr), n, C.addressof(out)), out


@pytest.mark.parametrize("order", ["given", "reversed"])
def test_a_batch_packs_like_single_calls(order):
    sizes = VC.SIZES + [VC.LARGEST, (40, 1), (300, 40)]
    sizes = sizes if order == "given" else sizes[::-1]
    a, b = HipContext(atlas_size=1024, record_only=True), HipContext(atlas_size=1024, record_only=True)
    got = a.put_video_frames([item(k, w, h) for k, (w, h) in enumerate(sizes, start=1)])
    want = [single_put(b, item(k, w, h)) for k, (w, h) in enumerate(sizes, start=1)]
    assert got == want and [r[2:] for r in got] == sizes
    assert state(a) == state(b) and a.atlas_size() == 1024
    keys = range(1, len(sizes) + 1)
    assert digest_of_a_frame(b, keys[1:]) != digest_of_a_frame(a, keys) == digest_of_a_frame(b, keys)
    st = a.video_batch_stats()
    assert (st["frames"], st["written"], st["dropped_by_growth"], st["launches"], st["bytes_copied"]) == (len(sizes), len(sizes), 0, 0, 0)
    assert st["tiles"] == sum(-(-w // 32) * -(-h // 32) for w, h in sizes)  # (a line keeps its tiles)
    # an update batch of a permuted subset moves the epoch as the single updates do, and nothing else
    subset = [(k, sizes[k - 1]) for k in (5, 2, 9, 1)]
    a.update_video_frames([item(k, w, h) for k, (w, h) in subset])
    for k, (w, h) in subset:
        single_put(b, item(k, w, h), update=True)
    assert state(a) == state(b) and digest_of_a_frame(a, keys) == digest_of_a_frame(b, keys)
    assert a.video_batch_stats()["frames"] == 4
    a.close(), b.close()


def test_refusals_leave_everything_untouched():
    """every refusal of the single header by its own case, as the first, the middle and the last frame of a batch whose others are good:
    nothing is placed, begun or bumped, out_rects is not written, and the stats stay those of the last batch that passed"""
    ctx = HipContext(atlas_size=256, record_only=True)
    L = ctx.L
    good = [frame(), p010(), bgra(width=8, height=2, pitch_y=32)]
    assert ctx.put_video_frames(zip((1, 2, 3), good)) and ctx.video_batch_stats()["frames"] == 3
    before, stats = state(ctx), ctx.video_batch_stats()

    def refused(code_and_rects, who, text):
        code, rects = code_and_rects
        assert code == INVALID and L.fdh_last_error().decode() == f"{who}: {text}", (who, text, code, L.fdh_last_error())
        assert state(ctx) == before and ctx.video_batch_stats() == stats and not any(ctx.has_image(k) for k in (7, 8, 9)), (who, text)
        assert all(list(r) == [-7] * 4 for r in rects), (who, text)

    structs = [(f, text) for f, text in REFUSED if f is not None]  # (an array has no null struct: the null arrays stand for it)
    assert len(structs) == len(REFUSED) - 1 >= 36
    for update, who in ((False, "put_video_frames"), (True, "update_video_frames")):
        keys = [1, 2, 3] if update else [7, 8, 9]
        refused(raw_put(ctx, keys, good, n=-1, update=update), who, "bad frame array")
        k = (C.c_int64 * 3)(*keys)
        arr = (VideoFrame * 3)()
        for a, b in ((None, C.addressof(arr)), (C.addressof(k), None)):
            code = L.fdh_update_video_frames(ctx.h, a, b, 3) if update else L.fdh_put_video_frames(ctx.h, a, b, 3, None)
            refused((code, []), who, "bad frame array")
        for bad, text in structs:
            for at in (0, 1, 2):
                refused(raw_put(ctx, keys, good[:at] + [bad] + good[at + 1:], update=update), who, text)
        refused(raw_put(ctx, [keys[0], keys[1], keys[0]], good[:2] + [good[0]], update=update), who, "a key occurs twice")
        wide = frame(width=2049, height=2, pitch_y=2049, pitch_uv=2050)
        high = bgra(width=2, height=2049, pitch_y=8)
        for big in (wide, high):
            refused(raw_put(ctx, keys, good[:2] + [big], update=update), who, "a frame of a batch is at most 2048 x 2048")
    refused(raw_put(ctx, [1, 2, 9], good, update=True), "update_video_frames", "unknown key")
    refused(raw_put(ctx, [1, 2, 3], good[:2] + [bgra(width=8, height=3, pitch_y=32)], update=True), "update_video_frames", "size mismatch")
    refused(raw_put(ctx, [3, 2, 1], good, update=True), "update_video_frames", "size mismatch")  # (the first frame already)
    # the limits on the batch as a whole
    code, _ = raw_put(ctx, list(range(100, 100 + 65536)), [frame()] * 65536)
    refused((code, []), "put_video_frames", "at most 65535 frames")
    full = frame(width=2048, height=2048, pitch_y=2048, pitch_uv=2048)
    code, _ = raw_put(ctx, list(range(100, 165)), [full] * 64 + [bgra(width=1, height=1, pitch_y=4)])  # 64 * 4096 + 1 tiles
    refused((code, []), "put_video_frames", "at most 2^18 tiles in a batch")
    # and a batch that passes moves on: the epoch by one per frame, the stats to its own
    assert raw_put(ctx, [1, 2, 3], good, update=True)[0] == 0
    assert ctx.atlas_usage()["epoch"] == before[0]["epoch"] + 3 and packed_area(ctx) == before[1]
    ctx.close()


def test_exactly_two_to_the_18_tiles_pass_validation():
    ctx = HipContext(atlas_size=256, record_only=True)
    full = frame(width=2048, height=2048, pitch_y=2048, pitch_uv=2048)
    code, _ = raw_put(ctx, list(range(1, 65)), [full] * 64)
    assert code == ATLAS_FULL  # 49 of them fill 16384 x 16384: the batch was placed, not refused
    assert ctx.video_batch_stats()["frames"] == 64
    ctx.close()


def test_an_empty_batch():
    ctx = HipContext(atlas_size=256, record_only=True)
    before = state(ctx)
    assert ctx.put_video_frames([]) == [] and ctx.update_video_frames([]) is None
    assert ctx.L.fdh_put_video_frames(ctx.h, None, None, 0, None) == 0 and ctx.L.fdh_update_video_frames(ctx.h, None, None, 0) == 0
    assert state(ctx) == before and ctx.video_batch_stats()["frames"] == 0
    ctx.close()


def test_growth_in_the_middle_of_a_batch():
    """an atlas of 256 and a batch that needs 512: the frames before the one that grows the atlas are gone, as after single calls"""
    sizes = [(100, 100), (100, 100), (60, 60), (120, 120), (90, 40), (33, 31)]
    a, b = HipContext(atlas_size=256, record_only=True), HipContext(atlas_size=256, record_only=True)
    assert single_put(a, item(50, 20, 20)) == single_put(b, item(50, 20, 20))
    got = a.put_video_frames([item(k, w, h) for k, (w, h) in enumerate(sizes, start=1)])
    want = [single_put(b, item(k, w, h)) for k, (w, h) in enumerate(sizes, start=1)]
    assert got == want and [r[2:] for r in got] == sizes and a.atlas_size() == b.atlas_size() == 512 and state(a) == state(b)
    assert digest_of_a_frame(a, range(1, 7)) == digest_of_a_frame(b, range(1, 7))
    alive = [a.has_image(k) for k in range(1, 7)]
    assert alive == [b.has_image(k) for k in range(1, 7)] and not a.has_image(50) and not alive[0] and alive[-1]
    st = a.video_batch_stats()
    assert st["dropped_by_growth"] == alive.count(False) > 0 and st["written"] == alive.count(True) and st["frames"] == 6
    a.close(), b.close()


def test_atlas_full_keeps_the_frames_before():
    """50 frames of 2048 x 2048: 49 fill an atlas of 16384, the fiftieth has no place"""
    a, b = HipContext(atlas_size=16384, record_only=True), HipContext(atlas_size=16384, record_only=True)
    n = 50
    with pytest.raises(FigdrawHipError) as e:
        a.put_video_frames([item(k, 2048, 2048) for k in range(1, n + 1)])
    assert e.value.code == ATLAS_FULL
    failed_at = None
    for k in range(1, n + 1):
        try:
            single_put(b, item(k, 2048, 2048))
        except FigdrawHipError as err:
            assert err.code == ATLAS_FULL
            failed_at = k
            break
    assert failed_at == 50 and state(a) == state(b)
    assert [a.has_image(k) for k in range(1, n + 1)] == [True] * 49 + [False]
    st = a.video_batch_stats()
    assert (st["frames"], st["written"], st["dropped_by_growth"]) == (50, 49, 0)
    a.close(), b.close()


def test_keep_mode_makes_room_once():
    a = HipContext(atlas_size=256, record_only=True)
    a.set_atlas_keep(True)
    for k, (w, h) in enumerate([(100, 100), (60, 60), (20, 20)], start=50):
        single_put(a, item(k, w, h))
    before = a.atlas_usage()
    sizes = [(100, 100), (120, 120), (90, 40), (100, 100), (33, 31)]
    got = a.put_video_frames([item(k, w, h) for k, (w, h) in enumerate(sizes, start=1)])
    after = a.atlas_usage()
    assert after["size"] > 256 and after["compactions"] == before["compactions"] + 1 and after["rebuilds"] == before["rebuilds"]
    assert all(a.has_image(k) for k in (50, 51, 52, 1, 2, 3, 4, 5)) and [a.image_rect(k) for k in range(1, 6)] == got
    st = a.video_batch_stats()
    assert (st["written"], st["dropped_by_growth"]) == (5, 0)
    a.close()


def test_update_batch_of_a_flippy_entry():
    a, b = HipContext(atlas_size=512, record_only=True), HipContext(atlas_size=512, record_only=True)
    data = open(os.path.join(GOLDEN, "img1.flippy"), "rb").read()
    r = a.put_flippy(3, data)
    assert r == b.put_flippy(3, data)
    assert single_put(a, item(4, 30, 20)) == single_put(b, item(4, 30, 20))
    a.update_video_frames([item(4, 30, 20), item(3, r[2], r[3])])
    single_put(b, item(4, 30, 20), update=True)
    b.update_image(3, np.zeros((r[3], r[2], 4), np.uint8))
    assert a.atlas_usage() == b.atlas_usage()
    assert a.compact_atlas()["rects_moved"] == b.compact_atlas()["rects_moved"]  # both are chain entries now
    a.close(), b.close()


def test_video_frames_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "video_frames_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_glyphs"),
                           os.path.join(ROOT, "tests", "video_frames_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "video_frames_abi_smoke: OK" in r.stdout


def test_the_binding_knows_the_struct():
    ctx = HipContext(atlas_size=256, record_only=True)
    assert ctx.L.fdh_sizeof_video_frame() == C.sizeof(VideoFrame) == 64
    assert C.sizeof(context.VideoBatchStats) == 32
    # an item as a tuple and as a struct are the same frame
    f = context.video_frame(0x10000, 0x20000, 16, 9, 16, 16, REF.NV12, REF.BT601, REF.FULL, REF.CHROMA_LINEAR)
    n, keys, arr = ctx._video_frame_arrays([(5, f), (6, 0x10000, 0x20000, 16, 9, 16, 16, REF.NV12, REF.BT601, REF.FULL, REF.CHROMA_LINEAR), (7, 0x10000, 0x20000, 16, 9, 16, 16)])
    assert n == 3 and list(keys) == [5, 6, 7] and bytes(arr[0]) == bytes(arr[1]) == bytes(f)
    assert (arr[2].format, arr[2].matrix, arr[2].range, arr[2].flags) == (REF.NV12, REF.BT709, REF.LIMITED, 0)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the tables
def level_size(v, l):
    return (v + (1 << l) - 1) >> l


def deep_levels(g, n_levels):
    """the levels from OWNER_LEVEL on that store texels of the frame"""
    out = []
    for l in range(OWNER_LEVEL, n_levels):
        if not (level_size(g[2], l) > 1 and level_size(g[3], l) > 1):
            break
        out.append(l)
    return out


def group_of(fmt, flags):
    return 0 if fmt == REF.BGRA8 else 1 + 2 * (fmt == REF.P010) + (flags & 1)


def restated(n_levels, first, m, frames):
    """frames: (x, y, w, h, format, flags) -> the tables by brute force; the owner of a texel is its last painter"""
    part = frames[first:first + m]
    records, tiles_of, owner_words, scratch, ink_blocks = [], [], 0, 0, 0
    for k, (x, y, w, h, fmt, flags) in enumerate(part):
        n_store = 0
        while n_store < n_levels and level_size(w, n_store) > 1 and level_size(h, n_store) > 1:
            n_store += 1
        tw, th = level_size(w, 5), level_size(h, 5)  # (a line keeps its tiles)
        ink = int(w <= 128 and h <= 128)
        records.append(dict(x=x, y=y, w=w, h=h, n_store=n_store, ink=ink, scratch_off=scratch, ink_off=ink_blocks, owner_off=owner_words * 32,
                            lw=[level_size(w, l) for l in range(6)], lh=[level_size(h, l) for l in range(6)]))
        tiles_of.append([k | tx << 16 | ty << 22 for ty in range(th) for tx in range(tw)])
        scratch += tw * th
        ink_blocks += tw * th * ink
        owner_words += (sum(level_size(w, l) * level_size(h, l) for l in deep_levels(part[k], n_levels)) + 31) // 32
    groups, tile_words = [], []
    for group in range(5):
        words = [t for k, g in enumerate(part) if group_of(g[4], g[5]) == group for t in tiles_of[k]]
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
    return dict(records=records, tiles=tile_words, groups=groups, tails=[r for r in records if r["n_store"] > 6], owner=owner, ink_blocks=ink_blocks)


KINDS = [(REF.BGRA8, 0), (REF.NV12, 0), (REF.NV12, 1), (REF.P010, 0), (REF.P010, 1)]
MIXED = [(4, 4, 12, 11), (24, 4, 100, 70), (132, 4, 12, 11), (152, 4, 70, 129), (4, 141, 300, 40), (4, 189, 1, 40), (13, 189, 40, 1)]
TABLE_CASES = {  # name -> (n_levels, first, m, [(x, y, w, h, format, flags)])
    "the level-6 pair": (9, 0, 2, [g + KINDS[1] for g in PAIR]),
    "the level-6 pair, the other way round": (9, 0, 2, [g + KINDS[k] for k, g in zip((4, 0), PAIR[::-1])]),
    "three, the middle one 1 texel high": (9, 0, 3, [(4, 4, 100, 100) + KINDS[0], (112, 4, 100, 1) + KINDS[2], (112, 13, 100, 90) + KINDS[1]]),
    "groups that alternate": (10, 0, 7, [g + KINDS[k % 5] for k, g in enumerate(MIXED)]),
    "groups that alternate the other way": (10, 0, 7, [g + KINDS[(3 * k + 1) % 5] for k, g in enumerate(MIXED)]),
    "one group": (10, 0, 7, [g + KINDS[4] for g in MIXED]),
    "a batch cut at first = 2": (10, 2, 4, [g + KINDS[k % 5] for k, g in enumerate(MIXED)]),
    "an atlas of 6 levels": (6, 0, 5, [g + KINDS[k % 2] for k, g in enumerate(MIXED[:5])]),
    "a 2048 x 66 frame beside a small one": (13, 0, 2, [(4, 4, 2048, 66) + KINDS[1], (4, 78, 40, 40) + KINDS[1]]),
}


@pytest.fixture(scope="module")
def table_programs(tmp_path_factory):
    """tests/video_batch_tables_emu/main.cpp with g++ alone, fdh_video_batch.h and what it includes beside it -> the directory of `tables` and
    of `tables_san`"""
    return emu_build.build(tmp_path_factory, "video_batch_tables_emu", ("fdh_video_batch.h", "fdh_video_import.h", "fdh_image_import.h", "fdh_glyph_tables.h", "fdh_msdf_host.h"),
                           {"tables": (), "tables_san": emu_build.SAN}, source="main.cpp")


def test_the_header_is_plain():
    text = open(os.path.join(CSRC, "fdh_video_batch.h")).read()
    assert set(re.findall(r'#include "([^"]+)"', text)) == {"fdh_glyph_tables.h", "fdh_video_import.h"}
    assert "hip" not in " ".join(re.findall(r"#include <([^>]+)>", text))
    public = open(os.path.join(ROOT, "include_glyphs", "figdraw_hip_video_frames.h")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)", public) == ["figdraw_hip_video_frame.h"] and "//" not in re.sub(r"/\*.*?\*/", "", public, flags=re.S)
    # and the kernel's unit includes what it included: tests/test_video_frame_host.py copies a fixed list of files beside it
    assert re.findall(r'#include "([^"]+)"', open(os.path.join(CSRC, "k_video_import.hip")).read()) == ["fdh_device.h", "fdh_video_import.h"]


def run_tables(table_programs, exe, case):
    n_levels, first, m, frames = TABLE_CASES[case]
    src = os.path.join(table_programs, f"{exe}.txt")
    with open(src, "w") as f:
        f.write(f"{n_levels} {first} {m} {len(frames)}\n" + "".join("%d %d %d %d %d %d\n" % g for g in frames))
    r = subprocess.run([os.path.join(table_programs, exe), src], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"{r.returncode} {r.stdout}{r.stderr}"
    return r.stdout.splitlines()


def check_tables(lines, case):
    """what the program printed against the tables restated here"""
    n_levels, first, m, frames = TABLE_CASES[case]
    want = restated(n_levels, first, m, frames)
    n_tiles, n_tails = len(want["tiles"]), len(want["tails"])
    at = [m * 42, m * 42 + n_tails * 32, m * 42 + n_tails * 32 + n_tiles, m * 42 + n_tails * 33 + n_tiles]
    words = at[3] + len(want["owner"])
    assert lines[1] == f"n_tiles {n_tiles} n_tails {n_tails} ink_blocks {want['ink_blocks']} words {words} at {at[0]} {at[1]} {at[2]} {at[3]}"
    assert [int(v) for v in lines[2].split()[1:]] == want["groups"]
    rest = " at %d %d size %d %d n_store %d"
    for k, g in enumerate(want["records"]):
        assert lines[3 + k] == ("frame %d" % k + rest % (g["x"], g["y"], g["w"], g["h"], g["n_store"]) + " ink %d scratch_off %d ink_off %d owner_off %d" % (g["ink"], g["scratch_off"], g["ink_off"], g["owner_off"])
                                + " lw " + " ".join(map(str, g["lw"])) + " lh " + " ".join(map(str, g["lh"])))
    for k, g in enumerate(want["tails"]):
        assert lines[3 + m + k] == ("tail %d" % k + rest % (g["x"], g["y"], g["w"], g["h"], g["n_store"]) + " scratch_off %d owner_off %d" % (g["scratch_off"], g["owner_off"])
                                    + " lw " + " ".join(map(str, g["lw"])) + " lh " + " ".join(map(str, g["lh"])))
    base = 3 + m + n_tails
    got_tiles = [int(v) for v in lines[base].split()[1:]]
    assert got_tiles == want["tiles"]
    assert [int(v) for v in lines[base + 1].split()[1:]] == list(range(n_tails))  # the tails' indices point into the tails' records
    assert [int(v) for v in lines[base + 2].split()[1:]] == want["owner"]
    # every tile is named once, and a group's tiles lie together
    part = frames[first:first + m]
    named = sorted((t & 0xFFFF, (t >> 16) & 63, t >> 22) for t in got_tiles)
    assert named == sorted((k, tx, ty) for k, g in enumerate(part) for ty in range(level_size(g[3], 5)) for tx in range(level_size(g[2], 5)))
    groups = [group_of(*part[t & 0xFFFF][4:]) for t in got_tiles]
    assert groups == sorted(groups)
    # what is reserved before the first placement -- for all frames, in an atlas of that many levels -- holds what is copied
    whole = restated(n_levels, 0, len(frames), frames)
    assert int(lines[0].split()[1]) == len(frames) * 42 + len(whole["tails"]) * 33 + len(whole["tiles"]) + len(whole["owner"]) >= words


@pytest.mark.parametrize("exe", ["tables", "tables_san"])
@pytest.mark.parametrize("case", list(TABLE_CASES))
def test_tables_are_the_painters(table_programs, exe, case):
    check_tables(run_tables(table_programs, exe, case), case)


def test_a_mutated_table_fails_the_check(table_programs):
    """one owner bit, two tile words swapped across a group's border, a tail's offset, a record's n_store: each makes check_tables fail"""
    case = "groups that alternate"
    lines = run_tables(table_programs, "tables", case)
    check_tables(lines, case)
    m, n_tails = TABLE_CASES[case][2], int(lines[1].split()[3])
    assert n_tails >= 2
    base = 3 + m + n_tails

    def edited(row, f):
        words = lines[row].split()
        f(words)
        return lines[:row] + [" ".join(words)] + lines[row + 1:]

    def flip(words):
        words[1] = str(int(words[1]) ^ 1)

    def swap(words):
        first_group_end = int(lines[2].split()[2])
        words[first_group_end], words[first_group_end + 1] = words[first_group_end + 1], words[first_group_end]

    def bump(name):
        def f(words):
            i = words.index(name) + 1
            words[i] = str(int(words[i]) + 1)
        return f

    mutants = [edited(base + 2, flip), edited(base, swap), edited(3 + m + 1, bump("scratch_off")), edited(3 + 1, bump("n_store")), edited(base + 1, flip)]
    for mutant in mutants:
        assert mutant != lines
        with pytest.raises(AssertionError):
            check_tables(mutant, case)


def test_the_table_cases_can_go_wrong():
    a = restated(*TABLE_CASES["the level-6 pair"])
    bits = lambda t: sum(bin(w).count("1") for w in t["owner"])  # noqa: E731
    per_frame = 7 * 7 + 4 * 4 + 2 * 2  # levels 4, 5 and 6 of a 100 x 100 frame
    assert bits(a) == 2 * per_frame - 4 - 2  # the shared columns of levels 5 and 6, four texels and two, belong to the later frame alone
    b = restated(*TABLE_CASES["the level-6 pair, the other way round"])
    assert bits(b) == bits(a) and a["owner"] != b["owner"] and len(a["tails"]) == 2 and b["groups"][1::2] == [16, 0, 0, 0, 16]
    thin = restated(*TABLE_CASES["three, the middle one 1 texel high"])
    assert [r["n_store"] for r in thin["records"]] == [7, 0, 7] and len(thin["tiles"]) == 16 + 4 + 12 and thin["groups"] == [0, 16, 16, 12, 28, 4, 32, 0, 32, 0]
    assert [r["ink"] for r in thin["records"]] == [1, 1, 1] and len(thin["tails"]) == 2
    alt = restated(*TABLE_CASES["groups that alternate"])
    assert all(n > 0 for n in alt["groups"][1::2]) and [t & 0xFFFF for t in alt["tiles"]] != sorted(t & 0xFFFF for t in alt["tiles"])
    assert restated(*TABLE_CASES["a 2048 x 66 frame beside a small one"])["records"][0]["lw"][5] == 64


# ------------------------------------------------------------------------------------------------------------------ 3. the kernels' source
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_video_import.hip and k_image_import.hip compiled as plain C++ under the sequential shim of tests/emu with the driver of
    tests/video_frames_emu -> the directory of ./emu and ./emu_san: the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "video_frames_emu", ("k_video_import.hip", "fdh_video_import.h", "k_image_import.hip", "fdh_image_import.h", "fdh_video_batch.h",
                                                                  "fdh_glyph_tables.h", "fdh_msdf_host.h"), {"emu": (), "emu_san": emu_build.SAN}, opt="-O2")


def run_batch(tmp, exe, cases, rects, size):
    """-> ([the levels' first rows as (rows, size >> l, 4) uint8], [per frame its folded ink block], what the program printed)"""
    n_levels = min(size.bit_length(), 14)
    out_rows = max(y + h for _, y, _, h in rects)
    with open(os.path.join(tmp, "batch.bin"), "wb") as f:
        f.write(np.array([len(cases), size, n_levels, out_rows], np.int32).tobytes())
        for case, (x, y, w, h) in zip(cases, rects):
            assert (w, h) == VC.size_of(case)
            (ybuf, yalign, ypitch), c = VC.pack(case)
            cbuf, calign, cpitch = c if c else (b"", 0, 0)
            f.write(np.array([w, h, case[1], case[2], case[3], case[4], ypitch, cpitch, yalign, calign, len(ybuf), len(cbuf), x, y, 0, 0], np.int32).tobytes())
            f.write(ybuf)
            f.write(cbuf)
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


def expected(cases, rects, shapes):
    """the atlas after single puts in array order, by the reference's texels and the host chain: the later frame wins a shared texel"""
    levels = [np.full(s, 0xEE, np.uint8) for s in shapes]
    for case, (x, y, w, h) in zip(cases, rects):
        for l, img in enumerate(REF.chain(VC.texels(case), len(shapes))):
            levels[l][(y >> l):(y >> l) + img.shape[0], (x >> l):(x >> l) + img.shape[1]] = img
    return levels


def check_batch(cases, rects, got):
    levels, inks, _ = got
    want = expected(cases, rects, [l.shape for l in levels])
    for l, (a, b) in enumerate(zip(levels, want)):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero((a != b).any(axis=2))
            raise AssertionError(f"level {l} differs in {len(xs)} texels, the first at ({xs[0]}, {ys[0]}): {a[ys[0], xs[0]]} != {b[ys[0], xs[0]]}")
    for case, block in zip(cases, inks):
        boxes = REF.ink_boxes(VC.texels(case))
        if boxes is None:
            assert block.reshape(16, 4).tolist() == [[32767, 32767, 0, 0]] * 16, case[0]
        else:  # (a line too: its tiles leave their blocks)
            got_boxes = block.reshape(16, 4).astype(np.int64)
            got_boxes[got_boxes[:, 2] == 0] = 0
            assert np.array_equal(got_boxes, boxes), case[0]


def batch_cases(**kw):
    """VC.cases under names of their own: VC.texels keeps its results by name, and cases(largest=False) draws other noise for the cases
    behind the sizes than the cases() of the single calls' tests do"""
    return [("batch " + c[0],) + c[1:] for c in VC.cases(**kw)]


@pytest.fixture(scope="module")
def mixed_batch():
    """all of cases(largest=False) with the places a record-only context gives them in an atlas of 1024"""
    cases = batch_cases(largest=False)
    ctx = HipContext(atlas_size=1024, record_only=True)
    rects = ctx.put_video_frames([item(k, *VC.size_of(c)) for k, c in enumerate(cases)])
    assert ctx.atlas_size() == 1024
    ctx.close()
    return cases, rects


def pair_cases():
    rng = np.random.default_rng(11)
    luma, chroma = VC.noise_yuv(rng, REF.P010, 100, 100)
    return [("pair a", REF.BGRA8, 0, 0, REF.STRAIGHT_ALPHA, VC.noise_bgra(rng, 100, 100), None, "tight"), ("pair b", REF.P010, REF.BT2020, REF.FULL, REF.CHROMA_LINEAR, luma, chroma, "padded")]


@pytest.fixture(scope="module")
def emulated(shim, mixed_batch):
    cases, rects = mixed_batch
    got = run_batch(shim, "./emu", cases, rects, 1024)
    print(got[2].strip())
    return got


def test_the_mixed_batch_against_the_reference(mixed_batch, emulated):
    cases, rects = mixed_batch
    assert len(cases) >= 40 and {group_of(c[1], c[4]) for c in cases} == {0, 1, 2, 3, 4} and {c[7] for c in cases} == {"tight", "padded", "aligned"}
    assert {VC.size_of(c) for c in cases} >= {(1, 1), (1, 9), (127, 129), (128, 128)}
    assert "launches 6" in emulated[2]  # five groups and the tails
    check_batch(cases, rects, emulated)


def test_the_mixed_batch_reversed(shim, mixed_batch):
    cases, rects = mixed_batch
    got = run_batch(shim, "./emu", cases[::-1], rects[::-1], 1024)
    check_batch(cases[::-1], rects[::-1], got)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_the_level_6_pair(shim, order):
    """the later frame of the array wins the shared column, whichever of the two it is"""
    both = pair_cases()
    cases, rects = [both[k] for k in order], [PAIR[k] for k in order]
    got = run_batch(shim, "./emu", cases, rects, 256)
    assert "tails 2 launches 3" in got[2]
    check_batch(cases, rects, got)
    one = expected(cases[:1], rects[:1], [l.shape for l in got[0]])[6]
    assert not np.array_equal(one[0:2, 0:4], got[0][6][0:2, 0:4])  # (the second frame did change level 6 of the first)
    san = run_batch(shim, "./emu_san", cases, rects, 256)
    assert all(np.array_equal(a, b) for a, b in zip(got[0], san[0])) and all(np.array_equal(a, b) for a, b in zip(got[1], san[1]))


def test_the_mixed_batch_under_sanitizers(shim, mixed_batch, emulated):
    """the stand-alone program built with -fsanitize=address,undefined: a read past either end of a plane, of the tables, a store outside a
    level, the scratch or the ink blocks is an error there; the bytes are the plain build's"""
    cases, rects = mixed_batch
    san = run_batch(shim, "./emu_san", cases, rects, 1024)
    assert all(np.array_equal(a, b) for a, b in zip(emulated[0], san[0])) and all(np.array_equal(a, b) for a, b in zip(emulated[1], san[1]))
