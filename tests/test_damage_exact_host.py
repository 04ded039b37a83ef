"""Exact damage readback, the host side (include/figdraw_hip_exact.h): the header and the C ABI, and the source of k_damage_filter itself
under the threaded host shim of tests/emu (tests/exact_emu), against numpy.  Everything here is equality of bytes and of counts."""
import os
import re
import subprocess

import numpy as np
import pytest

import emu_build
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "figdraw_hip_exact.h")
NEW_API = ("fdh_set_damage_exact", "fdh_damage_exact_stats")
INVALID = -1
EPOCH = 7  # what tests/exact_emu/emu.cpp passes as the epoch


# ------------------------------------------------------------------------------------------------------------------ header and ABI
def test_header_declares_and_library_exports_the_exact_api():
    src = open(HEADER).read()
    assert '#include "figdraw_hip.h"' in src
    declared = re.findall(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(", src)
    assert sorted(declared) == sorted(NEW_API)
    L = context.load()
    for name in NEW_API:
        assert hasattr(L, name), name
    others = ("figdraw_hip.h", "figdraw_hip_damage.h", "figdraw_hip_pick.h", "figdraw_hip_readback.h", "figdraw_hip_stream.h")
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(others + ("figdraw_hip_exact.h",))
    for other in others:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(r"\b%s\b" % n, text) for n in NEW_API), other


def test_exact_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "exact_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "exact_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "exact_abi_smoke: OK" in r.stdout
    src = open(os.path.join(ROOT, "tests", "exact_abi_smoke.c")).read()
    assert all(re.search(r"\b%s\b" % n, src) for n in NEW_API)


def test_record_only_context_refuses_the_mode_and_has_no_stats():
    ctx = HipContext(record_only=True)
    with pytest.raises(FigdrawHipError) as e:
        ctx.set_damage_exact(True)
    assert e.value.code == INVALID
    ctx.set_damage_exact(False)
    with pytest.raises(FigdrawHipError) as e:
        ctx.damage_exact_stats()
    assert e.value.code == INVALID
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the kernel's source on a CPU
def _grid(w, h):
    return (w + 63) // 64, (h + 63) // 64


def _tile_major(px):
    """a frame (h, w) uint32 as the mirror holds it: [bin][64][64], zeros past each tile's edge"""
    h, w = px.shape
    gx, gy = _grid(w, h)
    full = np.zeros((gy * 64, gx * 64), np.uint32)
    full[:h, :w] = px
    return np.ascontiguousarray(full.reshape(gy, 64, gx, 64).transpose(0, 2, 1, 3)).reshape(gx * gy, 64, 64)


def _differs(a, b):
    """the bins in which two frames differ, row-major"""
    return (_tile_major(a) != _tile_major(b)).any(axis=(1, 2))


def test_the_filter_kernel_source_under_a_host_shim(tmp_path):
    """figdraw_amd/csrc/k_damage_filter.hip itself, compiled as C++20 against the threaded shim of tests/emu (threads for lanes, a
    barrier for __syncthreads) with the driver of tests/exact_emu: the stamps, the count and every byte of the mirror against numpy.
    No device: the GPU tests hold the compiled kernel to the same."""
    emu_build.build(tmp_path, "exact_emu", ("k_damage_filter.hip", "fdh_damage_read.h"), {"emu": ()}, threads=True)
    runs = [0]

    def run(what, frame, mirror, pending=None, fill=False):
        """-> (stamps, count, mirror) after the kernel.  pending: a bool per bin (all = 0), or None (all = 1)"""
        h, w = frame.shape
        nb = len(mirror)
        frame.astype("<u4").tofile(tmp_path / "frame.raw")
        mirror.astype("<u4").tofile(tmp_path / "mirror.raw")
        stamps_in = np.zeros(nb, np.uint32)
        if pending is not None:
            # bins that are not pending carry the stamps they can have: the value of a filtered bin, an older epoch, and 0
            stamps_in = np.where(pending, EPOCH, np.array([EPOCH - 1, 3, 0], np.uint32)[np.arange(nb) % 3]).astype(np.uint32)
            stamps_in.astype("<u4").tofile(tmp_path / "stamps.raw")
        args = ["./emu", str(w), str(h), "frame.raw", "mirror.raw", "0" if pending is not None else "1", "stamps.raw" if pending is not None else "-",
                "1" if fill else "0"]
        r = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, what + ": " + r.stdout + r.stderr
        runs[0] += 1
        return stamps_in, np.fromfile(tmp_path / "stamps_out.raw", "<u4"), int(r.stdout.split()[0]), np.fromfile(tmp_path / "mirror_out.raw", "<u4").reshape(nb, 64, 64)

    def check(what, frame, held, pending=None, mirror=None):
        """held: the frame the mirror describes; mirror: its tile-major form when that is not _tile_major(held)"""
        mirror = _tile_major(held) if mirror is None else mirror
        nb = len(mirror)
        differs = _differs(frame, held)
        mine = np.ones(nb, bool) if pending is None else pending
        stamps_in, stamps, count, out = run(what, frame, mirror, pending)
        keep = mine & differs
        assert np.array_equal(stamps, np.where(keep, EPOCH, np.where(mine, EPOCH - 1, stamps_in))), f"{what}: the stamps"
        if mine.any():
            assert count == keep.sum(), f"{what}: the count is {count}, {keep.sum()} pending bins differ"
        else:
            assert count == 0xEEEEEEEE, f"{what}: no workgroup had a pending bin, yet the count was written"
        want = np.where(keep[:, None, None], _tile_major(frame), mirror)
        assert np.array_equal(out, want), f"{what}: the mirror (bins {np.nonzero((out != want).any(axis=(1, 2)))[0].tolist()})"
        return int(keep.sum())

    rng = np.random.RandomState(11)
    # 130 x 70: a 3 x 2 grid, last column 2 wide, last row 6 high; 513 x 389: rows that are not 16-byte aligned, a last column of 1 pixel;
    # 256 x 128: aligned, nothing clipped; 136 x 70 (beyond the issue's list): aligned rows AND a clipped column, of 8 pixels -- the only
    # size at which the 16-byte surface load runs beside a tile's edge
    for w, h in ((130, 70), (513, 389), (256, 128), (136, 70)):
        gx, gy = _grid(w, h)
        nb = gx * gy
        frame = rng.randint(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)
        pending = rng.rand(nb) < 0.5
        pending[0], pending[nb - 1] = True, False
        for p in (None, pending):
            tag = f"{w} x {h}, all = {int(p is None)}"
            assert check(f"{tag}: no bin differs", frame, frame.copy(), p) == 0
            assert check(f"{tag}: every bin differs", frame, frame ^ np.uint32(0x00010000), p) == (nb if p is None else p.sum())
            one = []
            held = frame.copy(); held[0, 0] ^= 1; one.append(("the first pixel of the frame", held))
            held = frame.copy(); held[63, 63] ^= 0x80000000; one.append(("the last pixel of bin 0", held))
            held = frame.copy(); held[h - 1, w - 1] ^= 0x100; one.append(("the last pixel of the last tile", held))
            held = frame.copy(); held[min(h - 1, 64 + 5), w - 1] ^= 1; one.append(("the last column", held))
            for name, held in one:
                n = check(f"{tag}: {name}", frame, held, p)
                assert n == int((_differs(frame, held) & (np.ones(nb, bool) if p is None else p)).sum()) <= 1
        # bytes outside a clipped tile's box.  On the surface, the pixels that follow a clipped tile's row belong to the next row's first
        # bin: a change there is that bin's alone.  In the mirror, the words of a slot that lie wholly past the tile's edge are not read.
        if w % 64:
            cw, only0 = w % 64, np.zeros(nb, bool)
            held = frame.copy(); held[1:64, 0:4] ^= 0xFF  # what a 16-byte load at the end of rows 0 .. 62 of the last column would reach into
            only0[0] = True
            assert np.array_equal(_differs(frame, held), only0)
            last_col = np.zeros(nb, bool); last_col[gx - 1::gx] = True
            assert check(f"{w} x {h}: pixels after a clipped row, the last column pending", frame, held, last_col) == 0
            assert check(f"{w} x {h}: pixels after a clipped row, every bin pending", frame, held, None) == 1
            def with_garbage(px):
                m = _tile_major(px)
                m[gx - 1::gx, :, (cw + 3) // 4 * 4:] = 0xDEADBEEF
                m[nb - gx:, h % 64:, :] = 0xDEADBEEF
                assert (m != _tile_major(px)).any()
                return m
            assert check(f"{w} x {h}: mirror words past the tiles' edges", frame, frame.copy(), None, with_garbage(frame)) == 0
            held = frame.copy(); held[h - 1, w - 1] ^= 1
            assert check(f"{w} x {h}: mirror words past the tiles' edges, the last tile changed", frame, held, None, with_garbage(held)) == 1
        # the fill form: every slot takes its tile, zeros past the edge; no stamp, no count
        garbage = rng.randint(0, 2 ** 32, (nb, 64, 64), dtype=np.uint64).astype(np.uint32)
        stamps_in, stamps, count, out = run(f"{w} x {h}: fill", frame, garbage, None, fill=True)
        assert np.array_equal(out, _tile_major(frame)) and np.array_equal(stamps, stamps_in) and count == 0xEEEEEEEE, f"{w} x {h}: fill"
    assert runs[0] > 40
