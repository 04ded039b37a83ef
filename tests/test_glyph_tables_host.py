"""The tables of a batch of glyphs (figdraw_amd/csrc/fdh_glyph_tables.h: batch_tables, batch_table_words and their helpers), compiled as they stand
into a stand-alone program (tests/glyph_tables_emu/main.cpp: plain C++, once more under AddressSanitizer and UBSan) and compared with a restatement
by brute force: the tiles of every glyph counted through, and for every level from kOwnerLevel on the level rectangles painted in array
order into a dictionary of texels -- a texel's owner is its last painter, which is what single puts in that order leave.  Everything here is equality."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "figdraw_amd", "csrc")
OWNER_LEVEL = 4  # msdf::kOwnerLevel
GLYPH_WORDS = 16  # sizeof(msdf::BatchGlyph) / 4
MARGIN = 4        # the packer's: rectangles are 2 * MARGIN apart

# name -> (n_levels, thin_tiles, first, m, [(x, y, w, h, n_edges)])
BESIDE = [(4, 4, 33, 33, 5), (4 + 33 + 2 * MARGIN, 4, 33, 33, 7)]  # levels 4 and 5 of the two overlap in a column; neither has a level 6
THIN = [(4, 4, 1, 40, 4), (13, 4, 40, 1, 4)]
MIXED = [(4, 4, 12, 11, 3), (24, 4, 100, 70, 9), (132, 4, 12, 11, 2)]  # no level >= 4; levels 4, 5 and 6; none
CASES = {
    "two 33 x 33 glyphs side by side": (11, 1, 0, 2, BESIDE),
    "the same two, the other way round": (11, 1, 0, 2, BESIDE[::-1]),
    "a 1 x 40 and a 40 x 1 glyph with tiles": (11, 1, 0, 2, THIN),
    "a 1 x 40 and a 40 x 1 glyph without": (11, 0, 0, 2, THIN),
    "thin glyphs beside a 33 x 33 one, without tiles": (11, 0, 0, 3, THIN + [(61, 4, 33, 33, 6)]),
    "a glyph without deep levels beside one with three": (11, 1, 0, 3, MIXED),
    "the same in an atlas of 6 levels": (6, 1, 0, 3, MIXED),
    "a batch cut at first = 1": (11, 1, 1, 2, MIXED),
    "a batch cut at first = 1 and before its last glyph": (11, 0, 1, 1, MIXED),
    "three overlapping at level 5 of 12": (12, 1, 0, 3, [(4, 4, 40, 40, 1), (52, 4, 40, 40, 1), (4, 52, 90, 40, 1)]),
}


def level_size(v, l):
    return (v + (1 << l) - 1) >> l


def has_level(g, l):
    return level_size(g[2], l) > 1 and level_size(g[3], l) > 1


def deep_levels(g, n_levels):
    """the levels from OWNER_LEVEL on that store texels of the glyph"""
    out = []
    for l in range(OWNER_LEVEL, n_levels):
        if not has_level(g, l):
            break
        out.append(l)
    return out


def restated(n_levels, thin, first, m, glyphs):
    part = glyphs[first:first + m]
    tiles = [((w + 7) // 8) * ((h + 7) // 8) if thin or (w > 1 and h > 1) else 0 for _, _, w, h, _ in part]
    records, tile_words, field_off, owner_words = [], [], 0, 0
    base = sum(g[4] for g in glyphs[:first])
    owner_off = []
    for k, g in enumerate(part):
        owner_off.append(owner_words * 32)
        records.append({"x": g[0], "y": g[1], "w": g[2], "h": g[3], "edge_off": sum(q[4] for q in glyphs[:first + k]) - base, "n_edges": g[4],
                        "field_off": field_off, "first_tile": len(tile_words), "owner_off": owner_words * 32})
        field_off += g[2] * g[3]
        tile_words += [k] * tiles[k]
        owner_words += (sum(level_size(g[2], l) * level_size(g[3], l) for l in deep_levels(g, n_levels)) + 31) // 32
    owner = [0] * (owner_words + 1)  # (one word more than the bits need, as the tables have)
    for l in range(OWNER_LEVEL, n_levels):
        painted = {}
        for k, (x, y, w, h, _) in enumerate(part):
            if has_level(part[k], l):
                for j in range(level_size(h, l)):
                    for i in range(level_size(w, l)):
                        painted[((x >> l) + i, (y >> l) + j)] = k
        for k, (x, y, w, h, _) in enumerate(part):
            if l not in deep_levels(part[k], n_levels):
                continue
            bit = owner_off[k] + sum(level_size(w, d) * level_size(h, d) for d in range(OWNER_LEVEL, l))
            for j in range(level_size(h, l)):
                for i in range(level_size(w, l)):
                    if painted[((x >> l) + i, (y >> l) + j)] == k:
                        owner[bit >> 5] |= 1 << (bit & 31)
                    bit += 1
    return {"n_tiles": len(tile_words), "n_edges": sum(g[4] for g in part), "records": records, "tiles": tile_words, "owner": owner}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """tests/glyph_tables_emu/main.cpp with g++ alone -> the directory of `tables` and of `tables_san`"""
    tmp = tmp_path_factory.mktemp("glyph_tables_emu")
    cc = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "glyph_tables_emu", "main.cpp")]
    subprocess.check_call(cc + ["-o", str(tmp / "tables")])
    subprocess.check_call(cc + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(tmp / "tables_san")])
    return tmp


def test_the_header_includes_the_standard_library_and_the_msdf_host_header_only():
    import re
    text = open(os.path.join(CSRC, "fdh_glyph_tables.h")).read()
    assert set(re.findall(r'#include "([^"]+)"', text)) == {"fdh_msdf_host.h"}
    assert "hip" not in " ".join(re.findall(r"#include <([^>]+)>", text))


@pytest.mark.parametrize("exe", ["tables", "tables_san"])
@pytest.mark.parametrize("case", list(CASES))
def test_tables_are_the_painters(programs, exe, case):
    n_levels, thin, first, m, glyphs = CASES[case]
    src = programs / f"{exe}.txt"
    src.write_text(f"{n_levels} {thin} {first} {m} {len(glyphs)}\n" + "".join("%d %d %d %d %d\n" % g for g in glyphs))
    r = subprocess.run([str(programs / exe), str(src)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"{r.returncode} {r.stdout}{r.stderr}"
    lines = r.stdout.splitlines()
    want = restated(n_levels, bool(thin), first, m, glyphs)
    words = m * GLYPH_WORDS + want["n_tiles"] + len(want["owner"])
    assert lines[1] == f"n_tiles {want['n_tiles']} n_edges {want['n_edges']} words {words}"
    assert lines[2:2 + m] == ["glyph %d at %d %d size %d %d edge_off %d n_edges %d field_off %d first_tile %d owner_off %d"
                              % (k, g["x"], g["y"], g["w"], g["h"], g["edge_off"], g["n_edges"], g["field_off"], g["first_tile"], g["owner_off"]) for k, g in enumerate(want["records"])]
    assert [int(v) for v in lines[2 + m].split()[1:]] == want["tiles"]
    assert [int(v) for v in lines[3 + m].split()[1:]] == want["owner"]
    # what is reserved before the first placement -- for all glyphs, in an atlas of that many levels -- holds what is copied
    reserved = int(lines[0].split()[1])
    assert reserved >= words and reserved == len(glyphs) * GLYPH_WORDS + restated(n_levels, bool(thin), 0, len(glyphs), glyphs)["n_tiles"] + len(restated(n_levels, bool(thin), 0, len(glyphs), glyphs)["owner"])


def test_the_cases_can_go_wrong():
    """the overlap, the thin glyphs and the cut are in the cases: a table that ignored painter's order, thin_tiles or `first` would differ"""
    a = restated(*CASES["two 33 x 33 glyphs side by side"])
    bits = lambda t: sum(bin(w).count("1") for w in t["owner"])  # noqa: E731
    assert bits(a) == 2 * (3 * 3 + 2 * 2) - (3 + 2)  # a column of level 4 and one of level 5 belong to the later glyph alone
    assert a["owner"] != restated(*CASES["the same two, the other way round"])["owner"]
    assert restated(*CASES["a 1 x 40 and a 40 x 1 glyph with tiles"])["n_tiles"] == 10 and restated(*CASES["a 1 x 40 and a 40 x 1 glyph without"])["n_tiles"] == 0
    mixed = restated(*CASES["a glyph without deep levels beside one with three"])
    assert [g["owner_off"] for g in mixed["records"]] == [0, 0, 64] and bits(mixed) == 7 * 5 + 4 * 3 + 2 * 2
    assert bits(restated(*CASES["the same in an atlas of 6 levels"])) == 7 * 5 + 4 * 3
    cut = restated(*CASES["a batch cut at first = 1"])
    assert [g["edge_off"] for g in cut["records"]] == [0, 9] and cut["n_edges"] == 11
