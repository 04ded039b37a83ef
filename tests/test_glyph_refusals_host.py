"""Every refusal of the glyph entry points (fdh_put_glyph_image, fdh_put_glyph_outline, fdh_put_glyph_outline_cubic, fdh_put_glyph_outlines,
fdh_put_glyph_outlines_cubic, fdh_put_glyph_coverage_batch, fdh_put_glyph_coverage_batch_cubic), replayed on a record-only context:
tests/golden/glyph_refusals.json holds (call, arguments, code, message) as the library answered before the glyph code moved out of
class Atlas (tools/make_glyph_refusals.py wrote it, and lists the cases).  The code and the message text are part of what a caller sees:
which of several applicable errors wins, and under which call's name a cubic call without a cubic reports.  Everything here is equality."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from figdraw_amd.context import FigdrawHipError, GlyphOutline, HipContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "glyph_refusals.json")
FLOATS = {"put_glyph_outline": 6, "put_glyph_outlines": 6, "put_glyph_coverage_batch": 6,
          "put_glyph_outline_cubic": 8, "put_glyph_outlines_cubic": 8, "put_glyph_coverage_batch_cubic": 8}


def segments(spec, floats, shapes):
    """spec: None (no array), or parts [shape name, its first k segments, times] one after the other; a shape: rows of floats, null = NaN
    -> float32 (n, floats)"""
    if spec is None:
        return None
    parts = [np.tile(np.array([[np.nan if v is None else v for v in row] for row in shapes[name][:first]], np.float32).reshape(-1, floats), (times, 1)) for name, first, times in spec]
    return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, floats), np.float32))


def run(ctx, call, a, shapes):
    """the C call itself -> (status, message of the error it raised through the wrapper's own check, or "")"""
    L, keep = ctx.L, []
    if call == "put_glyph_image":
        rgba = np.zeros((max(a["h"], 1), max(a["w"], 1), 4), np.uint8)
        rc = L.fdh_put_glyph_image(ctx.h, a["key"], a["w"], a["h"], rgba.ctypes.data if a["rgba"] else None, a["flags"], (C.c_int * 4)())
    elif call in ("put_glyph_outline", "put_glyph_outline_cubic"):
        segs = segments(a["segs"], FLOATS[call], shapes)
        n = a["n"] if a.get("n") is not None else len(segs)
        rc = getattr(L, "fdh_" + call)(ctx.h, a["key"], a["w"], a["h"], segs.ctypes.data if segs is not None and len(segs) else None, n, a["flags"], (C.c_int * 4)())
    else:
        glyphs = [g for g in a["glyphs"] for _ in range(g.get("times", 1))]
        arr = (GlyphOutline * max(len(glyphs), 1))()
        shared = {}
        for i, (slot, g) in enumerate(zip(arr, glyphs)):
            spec = json.dumps(g["segs"])
            if spec not in shared:
                shared[spec] = segments(g["segs"], FLOATS[call], shapes)
            segs = shared[spec]
            slot.key, slot.width, slot.height, slot.sdf_range = g["key"] + i, g["w"], g["h"], g.get("range", 0)
            slot.segs = segs.ctypes.data if segs is not None and len(segs) else None
            slot.n_segs = g["n"] if g.get("n") is not None else len(segs)
        keep.append(shared)
        out = ((C.c_int * 4) * max(len(glyphs), 1))()
        n = a["n_glyphs"] if a.get("n_glyphs") is not None else len(glyphs)
        rc = getattr(L, "fdh_" + call)(ctx.h, None if a.get("null_array") else C.addressof(arr), n, a["flags"], C.addressof(out))
    try:
        ctx._ck(rc)
    except FigdrawHipError as e:
        assert e.code == rc
        return rc, str(e)[len(f"[{rc}] "):]
    return rc, ""


TABLE = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {"shapes": {}, "cases": []}  # (the tool that writes the file imports run() from here)

CASES = TABLE["cases"]


def test_the_table_covers_every_entry_point():
    assert {c["call"] for c in CASES} == set(FLOATS) | {"put_glyph_image"}
    assert all(c["code"] != 0 and c["message"] for c in CASES)
    assert len({c["what"] for c in CASES}) == len(CASES)


@pytest.fixture(scope="module")
def ctx():
    c = HipContext(record_only=True)
    yield c
    c.close()


@pytest.mark.parametrize("case", CASES, ids=[c["what"] for c in CASES])
def test_refusal_is_the_recorded_one(ctx, case):
    size, stats = ctx.atlas_size(), (ctx.glyph_batch_stats(), ctx.glyph_coverage_batch_stats())
    assert run(ctx, case["call"], case["args"], TABLE["shapes"]) == (case["code"], case["message"])
    assert ctx.atlas_size() == size and not ctx.has_image(case["args"].get("key", 700))  # nothing was placed
    assert (ctx.glyph_batch_stats(), ctx.glyph_coverage_batch_stats()) == stats  # a refused batch leaves the figures of the call before it
