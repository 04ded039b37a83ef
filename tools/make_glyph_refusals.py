#!/usr/bin/env python3
"""Writes tests/golden/glyph_refusals.json: every refusal of the glyph entry points as the built library answers it on a record-only context
(tests/test_glyph_refusals_host.py replays the table).  One case per `throw` of the glyph code; for the calls that take segments of 8
floats each applicable refusal twice, with a cubic in the outline and without one (without one the call is the six-float call, and where
that call refuses, it does so under its own name); and some calls to which two refusals apply, to pin which one wins.
Run it on the commit whose answers are to be kept, not on the one under test.

  make_glyph_refusals.py [--check]      --check: write nothing, compare with the file"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

LCD_FILTER, LCD_CONTEXT, MTSDF, CORRECT, OVERLAP = 1, 2, 4, 8, 32
N = None  # NaN
SQ6 = [[2, 2, N, N, 10, 2], [10, 2, N, N, 10, 9], [10, 9, N, N, 2, 9], [2, 9, N, N, 2, 2]]
TRI6 = [[2, 2, N, N, 10, 2], [10, 2, N, N, 6, 9], [6, 9, N, N, 2, 2]]
QUAD6 = [0, 0, 1000, 1000, 0, 0]  # 64 chords
# the same square in 8 floats, cubic-free; and with its right side a cubic
SQ8 = [[r[0], r[1], N, N, N, N, r[4], r[5]] for r in SQ6]
TRI8 = [[r[0], r[1], N, N, N, N, r[4], r[5]] for r in TRI6]
CU8 = [SQ8[0], [10, 2, 12, 4, 12, 7, 10, 9], SQ8[2], SQ8[3]]
CUTRI8 = [TRI8[0], [10, 2, 11, 5, 9, 8, 6, 9], TRI8[2]]
QUAD8 = [0, 0, 1000, 1000, N, N, 0, 0]
CUBIC8 = [0, 0, 1000, 1000, -1000, 1000, 0, 0]  # 256 chords


SHAPES = {"SQ6": SQ6, "TRI6": TRI6, "QUAD6": [QUAD6], "SQ8": SQ8, "TRI8": TRI8, "CU8": CU8, "CUTRI8": CUTRI8, "QUAD8": [QUAD8], "CUBIC8": [CUBIC8]}


def rows(shape, first=None, times=1):
    """an outline: the first `first` segments (None: all) of a named shape, `times` times over"""
    return [[shape, len(SHAPES[shape]) if first is None else first, times]]


def single_cases(call, shapes):
    """shapes: {tag: (closed outline, open outline)}"""
    out = []
    for tag, (closed, opened) in shapes.items():
        def c(what, w=12, h=11, segs=closed, n=None, flags=0):
            out.append({"what": f"{call}, {tag}: {what}", "call": call, "args": {"key": 700, "w": w, "h": h, "segs": segs, "n": n, "flags": flags}})
        c("width 0", w=0)
        c("height 4097", h=4097)
        c("a negative segment count", n=-1)
        c("segments without a pointer", segs=None, n=4)
        c("an unknown flag", flags=16)
        c("an unknown flag beside FDH_GLYPH_MTSDF", flags=MTSDF | 64)
        c("a range without FDH_GLYPH_MTSDF", flags=4 << 8)
        c("a range of 65", flags=MTSDF | 65 << 8)
        c("FDH_GLYPH_MTSDF_CORRECT alone", flags=CORRECT)
        c("FDH_GLYPH_MTSDF_OVERLAP alone", flags=OVERLAP)
        c("FDH_GLYPH_MTSDF_OVERLAP with FDH_GLYPH_MTSDF", flags=MTSDF | OVERLAP, segs=opened)  # (refused for the open contour, or for the cubic)
        c("a distance field with FDH_GLYPH_LCD_FILTER", flags=MTSDF | LCD_FILTER)
        c("a distance field with FDH_GLYPH_LCD_CONTEXT", flags=MTSDF | LCD_CONTEXT)
        c("65536 segments", flags=MTSDF, segs=rows(closed[0][0], None, 16384))
        c("an open contour", flags=MTSDF, segs=opened)
        # two at once
        c("width 0 and an unknown flag", w=0, flags=16)
        c("a negative segment count and height 0", h=0, n=-1)
        c("a range of 65 and FDH_GLYPH_MTSDF_CORRECT, both without FDH_GLYPH_MTSDF", flags=CORRECT | 65 << 8)
        c("an LCD flag and an open contour", flags=MTSDF | LCD_FILTER, segs=opened)
        c("65536 segments of an open contour", flags=MTSDF, segs=rows(opened[0][0], 3, 21846))
        c("FDH_GLYPH_MTSDF_OVERLAP and FDH_GLYPH_MTSDF_CORRECT alone", flags=CORRECT | OVERLAP)
    return out


def field_batch_cases(call, shapes):
    out = []
    for tag, (closed, opened, tri) in shapes.items():
        good = {"key": 700, "w": 12, "h": 11, "segs": closed}

        def c(what, glyphs=(good,), flags=MTSDF, **more):
            out.append({"what": f"{call}, {tag}: {what}", "call": call, "args": dict({"glyphs": list(glyphs), "flags": flags}, **more)})
        g = lambda **kw: dict(good, **kw)  # noqa: E731
        c("an LCD flag", flags=MTSDF | LCD_FILTER)
        c("an unknown flag", flags=MTSDF | 16)
        c("no FDH_GLYPH_MTSDF", flags=0)
        c("FDH_GLYPH_MTSDF_CORRECT alone", flags=CORRECT)
        c("a range of 65 in the flags", flags=MTSDF | 65 << 8)
        c("a negative glyph count", n_glyphs=-1)
        c("glyphs without a pointer", null_array=True)
        c("65536 glyphs", glyphs=[g(times=65536)])
        c("a 4097-wide glyph", glyphs=[good, g(w=4097)])
        c("a 0-high glyph", glyphs=[good, g(h=0)])
        c("a negative segment count", glyphs=[good, g(segs=None, n=-1)])
        c("segments without a pointer", glyphs=[good, g(segs=None, n=4)])
        c("65536 segments in one glyph", glyphs=[good, g(segs=rows(closed[0][0], None, 16384))])
        c("a range of 65", glyphs=[good, g(range=65)])
        c("2^24 + 1 texels", glyphs=[g(w=2048, h=2048, times=4), g(w=1, h=1)])
        many = rows(tri[0][0], None, 21845)
        c("2^20 + 1 segments", glyphs=[g(segs=many, times=16), g(segs=rows(tri[0][0], None, 3) + rows(closed[0][0], None, 2))])
        c("an open contour in the middle", glyphs=[good, g(segs=opened), good])
        c("FDH_GLYPH_MTSDF_OVERLAP", glyphs=[good, g(segs=opened)], flags=MTSDF | OVERLAP)  # (refused for the open contour, or for the cubic)
        # two at once
        c("no FDH_GLYPH_MTSDF and an unknown flag", flags=16)
        c("a range of 65 in the flags and glyphs without a pointer", flags=MTSDF | 65 << 8, null_array=True)
        c("a 0-high glyph after one of a range of 65", glyphs=[g(range=65), g(h=0)])
        c("an open contour before a 4097-wide glyph", glyphs=[g(segs=opened), g(w=4097)])
        c("2^24 + 1 texels and an open contour", glyphs=[g(w=2048, h=2048, times=4), g(w=1, h=1, segs=opened)])
        c("65536 glyphs and no FDH_GLYPH_MTSDF", glyphs=[g(times=65536)], flags=0)
    return out


def coverage_batch_cases(call, shapes):
    out = []
    for tag, (closed, steep, chords) in shapes.items():
        good = {"key": 700, "w": 12, "h": 11, "segs": closed}

        def c(what, glyphs=(good,), flags=0, **more):
            out.append({"what": f"{call}, {tag}: {what}", "call": call, "args": dict({"glyphs": list(glyphs), "flags": flags}, **more)})
        g = lambda **kw: dict(good, **kw)  # noqa: E731
        c("FDH_GLYPH_MTSDF", flags=MTSDF)
        c("an unknown flag", flags=LCD_FILTER | 16)
        c("a negative glyph count", n_glyphs=-1)
        c("glyphs without a pointer", null_array=True)
        c("65536 glyphs", glyphs=[g(times=65536)])
        c("a 4097-wide glyph", glyphs=[good, g(w=4097)])
        c("a 0-high glyph", glyphs=[good, g(h=0)])
        c("a negative segment count", glyphs=[good, g(segs=None, n=-1)])
        c("segments without a pointer", glyphs=[good, g(segs=None, n=4)])
        c("a distance range", glyphs=[good, g(range=4)])
        c("2^20 + 1 segments", glyphs=[g(segs=rows(closed[0][0], None, 1 << 18)), g(segs=rows(closed[0][0], 1))])
        c("2^24 + 1 texels", glyphs=[g(w=2048, h=2048, times=4), g(w=1, h=1)])
        c(f"2^22 + {chords} flattened lines", glyphs=[g(segs=rows(steep, None, (1 << 22) // chords + 1))])
        # two at once
        c("FDH_GLYPH_MTSDF and glyphs without a pointer", flags=MTSDF, null_array=True)
        c("a distance range before a 0-high glyph", glyphs=[g(range=4), g(h=0)])
        c("2^20 + 1 segments before a 4097-wide glyph", glyphs=[g(segs=rows(closed[0][0], None, 1 << 18)), g(segs=rows(closed[0][0], 1)), g(w=4097)])
        c("2^24 + 1 texels and 2^22 flattened lines", glyphs=[g(w=2048, h=2048, times=4), g(w=1, h=1, segs=rows(steep, None, (1 << 22) // chords + 1))])
    return out


def cases():
    out = []
    for what, a in (("width 0", dict(w=0, h=4, rgba=True, flags=0)), ("height -1", dict(w=4, h=-1, rgba=True, flags=0)), ("no texels", dict(w=4, h=4, rgba=False, flags=0)),
                    ("an unknown flag", dict(w=4, h=4, rgba=True, flags=4)), ("no texels and an unknown flag", dict(w=4, h=4, rgba=False, flags=8))):
        out.append({"what": f"put_glyph_image: {what}", "call": "put_glyph_image", "args": dict(a, key=700)})
    out += single_cases("put_glyph_outline", {"lines": (rows("SQ6"), rows("SQ6", 3))})
    out += single_cases("put_glyph_outline_cubic", {"no cubic": (rows("SQ8"), rows("SQ8", 3)), "a cubic": (rows("CU8"), rows("CU8", 3))})
    out += field_batch_cases("put_glyph_outlines", {"lines": (rows("SQ6"), rows("SQ6", 3), rows("TRI6"))})
    out += field_batch_cases("put_glyph_outlines_cubic", {"no cubic": (rows("SQ8"), rows("SQ8", 3), rows("TRI8")), "a cubic": (rows("CU8"), rows("CU8", 3), rows("CUTRI8"))})
    out += coverage_batch_cases("put_glyph_coverage_batch", {"lines": (rows("SQ6"), "QUAD6", 64)})
    out += coverage_batch_cases("put_glyph_coverage_batch_cubic", {"no cubic": (rows("SQ8"), "QUAD8", 64), "a cubic": (rows("CU8"), "CUBIC8", 256)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    import test_glyph_refusals_host as T
    from figdraw_amd.context import HipContext

    ctx = HipContext(record_only=True)
    table = []
    for c in cases():
        code, message = T.run(ctx, c["call"], c["args"], SHAPES)
        assert code != 0, f"{c['what']}: accepted"
        table.append(dict(c, code=code, message=message))
    ctx.close()
    if a.check:
        assert {"shapes": SHAPES, "cases": table} == json.load(open(T.GOLDEN)), "the library's answers are not the file's"
        print(f"{len(table)} refusals as recorded")
        return
    with open(T.GOLDEN, "w") as f:
        f.write('{"shapes": ' + json.dumps(SHAPES) + ',\n"cases": [\n' + ",\n".join(json.dumps(c) for c in table) + "\n]}\n")
    print(f"{len(table)} refusals -> {T.GOLDEN}")


if __name__ == "__main__":
    main()
