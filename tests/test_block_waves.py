"""Block waves change no byte.  In the full-frame launch of the no-clip builds (k_composite_tiles<4> and <4 | 32>) a bin whose list holds at
most FDH_BLOCK_MAX draws gets one wave per 32 x 32 block -- four strips shaded one after the other by the same body, with the interior
form of its prologue and epilogue -- where the frame has no partial strip (W a multiple of 32, H of 8, pitch of 4, no stripe), the order of
the previous frame is at hand and the launch has no deep strips; everything else keeps one wave per strip.  FDH_BLOCK_WAVES=0 turns the
form off.  Every sequence of frames below is rendered in four child processes (the switches are read once per process) --
the form off, on with a threshold of 8, on with a threshold of 254 (every bin takes it) and the library's defaults -- and every frame must
come out byte for byte the same as with the form off; fdh_block_wave_bins says which launches took the form and for how many bins."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

BLOCK_MAX = 8
OPAQUE = (0.2, 0.4, 0.9, 1.0)
TRANSLUCENT = (0.2, 0.4, 0.9, 0.5)

# draws per 64 x 64 bin of a 512 x 128 frame (8 x 2 bins), row by row: BLOCK_MAX - 1, BLOCK_MAX and BLOCK_MAX + 1 draws, bins with none.
# The launch takes bins longest list first per class (bin index mod 8) and the boundary is the same position in every class: here ONE bin
# (index 2) is over the threshold, so the longest bin of every class keeps one wave per strip and the other eight get block waves -- among
# them the bin with 7 draws (its class-mate has 8), one of the two with 8 of class 1, and both empty ones.  72 draws: more than a direct launch takes.
PILES = [7, 8, 9, 0, 3, 2, 1, 4,
         8, 8, 1, 5, 0, 6, 2, 8]
# the same frame with 40 draws piled into a bin it left empty (index 3), and with the 9-draw bin emptied
PILES_40 = [7, 8, 0, 40, 3, 2, 1, 4,
            8, 8, 1, 5, 0, 6, 2, 8]


def pile(lst, bx, by, n, seed):
    """n one-draw nodes (a translucent fill, rounded corners) inside bin (bx, by): each crosses strips and blocks of the bin, none leaves it"""
    from figdraw_amd.scene import Fig, FigKind, rect, rgba

    rng = np.random.RandomState(1000 * seed + 17 * bx + by)
    for _ in range(n):
        w, h = int(rng.randint(12, 50)), int(rng.randint(12, 50))
        x, y = int(rng.randint(4, 60 - w + 1)), int(rng.randint(4, 60 - h + 1))
        lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(64 * bx + x, 64 * by + y, w, h), corners=[int(rng.randint(0, 9))] * 4,
                        fill=rgba(int(rng.randint(256)), int(rng.randint(256)), int(rng.randint(256)), int(rng.randint(60, 256)))))


def piles_scene(piles, bins_x=8, seed=1):
    from figdraw_amd.scene import RenderList, Renders

    lst = RenderList()
    for i, n in enumerate(piles):
        pile(lst, i % bins_x, i // bins_x, n, seed)
    out = Renders()
    out.setLayer(0, lst)
    return out


def nodes_scene(w, h, copies=8):
    """every path of the no-clip build (test_opaque_surface's nodes: fills, a 3-stop gradient, strokes, elliptical corners, drop and inner
    shadows, a shared distance field, an opaque core that cuts the lists), spread over the frame; more than 64 draws"""
    from figdraw_amd.scene import RenderList, Renders

    import test_opaque_surface as TO

    lst = RenderList()
    for c in range(copies):
        for n in TO._small_nodes(dx=float((37 * c) % max(w - 60, 1)) - 20.0, dy=float((23 * c) % max(h - 30, 1)) - 10.0):
            lst.addRoot(n)
    out = Renders()
    out.setLayer(0, lst)
    return out


# name -> (w, h, clear colour, stripe or None, [scene of frame 0, 1, ...], the launches of frames >= 1 can take the form)
def _sequences():
    seq = {}
    for tag, clear in (("opaque", OPAQUE), ("translucent", TRANSLUCENT)):  # <4 | 32> and <4>
        seq[f"one_bin_{tag}"] = (64, 64, clear, None, [lambda: nodes_scene(64, 64)] * 3, True)
        # the bottom bin row holds rows 64 .. 71: one strip of each of its upper blocks, its lower blocks wholly off the frame
        seq[f"bottom_row_{tag}"] = (128, 72, clear, None, [lambda: nodes_scene(128, 72)] * 3, True)
        seq[f"piles_{tag}"] = (512, 128, clear, None, [lambda: piles_scene(PILES)] * 3, True)
    seq["tall_tail"] = (96, 200, OPAQUE, None, [lambda: nodes_scene(96, 200, copies=12)] * 3, True)  # H = 3 bins + 8 rows
    seq["width_200"] = (200, 136, OPAQUE, None, [lambda: nodes_scene(200, 136)] * 3, False)  # partial strips on the right
    seq["pitch_202"] = (202, 136, OPAQUE, None, [lambda: nodes_scene(202, 136)] * 3, False)  # ... and no 16-byte rows
    seq["height_132"] = (128, 132, OPAQUE, None, [lambda: nodes_scene(128, 132)] * 3, False)  # a strip of four rows at the bottom
    seq["striped"] = (128, 128, OPAQUE, (40, 104), [lambda: nodes_scene(128, 128)] * 3, False)
    # a stale order and a stale boundary: 40 draws into a bin the frames before left empty (its blocks have one wave each), and back
    seq["stale"] = (512, 128, OPAQUE, None, [lambda: piles_scene(PILES)] * 3 + [lambda: piles_scene(PILES_40), lambda: piles_scene(PILES)], True)
    seq["stale_reverse"] = (512, 128, TRANSLUCENT, None, [lambda: piles_scene(PILES_40)] * 3 + [lambda: piles_scene(PILES), lambda: piles_scene(PILES_40)], True)
    return seq


SEQUENCES = _sequences()
# (no direct launches and no deep strips where the form is looked for: a frame of a handful of draws has no lists, and a launch with deep
# strips -- bins of 24 draws, which the nodes' frames have -- is k_composite_deep's; the defaults keep both)
COMMON = {"FDH_DIRECT": "0", "FDH_DEEP_MIN": "0"}
SETTINGS = {"off": {"FDH_BLOCK_WAVES": "0", **COMMON}, "on8": {"FDH_BLOCK_MAX": str(BLOCK_MAX), **COMMON},
            "on254": {"FDH_BLOCK_MAX": "254", **COMMON}, "default": {}}


def render_all():
    """(a child process) every sequence on a context of its own -> 'name/i': pixels of frame i, and name -> [block_wave_bins after frame i]"""
    from figdraw_amd.context import HipContext

    frames, bins = {}, {}
    for name, (w, h, clear, stripe, scenes, _) in SEQUENCES.items():
        ctx = HipContext(device=0)
        if stripe:
            ctx.set_stripe(*stripe)
        bins[name] = []
        for i, make in enumerate(scenes):
            ctx.render_frame(make(), w, h, color=clear)
            ctx.sync()  # (the sorting waves' counts are on the host before the next frame is scheduled)
            px = ctx.read_pixels()
            frames[f"{name}/{i}"] = (px[stripe[0]:stripe[1]] if stripe else px).copy()  # (a striped context renders its rows only)
            bins[name].append(ctx.block_wave_bins())
        ctx.close()
    return frames, bins


@pytest.fixture(scope="module")
def runs():
    """setting -> (frames, bins)"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_block_waves as T\n"
            "frames, bins = T.render_all()\n"
            "np.savez(sys.argv[1], **frames)\n"
            "print('BINS', bins)\n") % (ROOT, HERE)
    out = {}
    keep = {k: v for k, v in os.environ.items() if k not in ("FDH_BLOCK_WAVES", "FDH_BLOCK_MAX")}
    with tempfile.TemporaryDirectory() as td:
        for tag, env in SETTINGS.items():
            path = os.path.join(td, tag + ".npz")
            r = subprocess.run([sys.executable, "-c", code, path], env={**keep, **env}, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, (tag, r.stderr[-2000:])
            out[tag] = (dict(np.load(path)), eval([ln for ln in r.stdout.splitlines() if ln.startswith("BINS ")][-1][5:]))
    return out


FRAMES = [f"{name}/{i}" for name, s in SEQUENCES.items() for i in range(len(s[4]))]


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["on8", "on254", "default"])
@pytest.mark.parametrize("frame", FRAMES)
def test_the_form_changes_no_byte(runs, setting, frame):
    got, want = runs[setting][0][frame], runs["off"][0][frame]
    assert got.shape == want.shape
    assert np.array_equal(got, want), (setting, frame, int((got != want).any(axis=2).sum()), "pixels differ; block_wave_bins",
                                       runs[setting][1][frame.split("/")[0]])


@pytest.mark.gpu
def test_frames_are_not_blank(runs):
    """(the comparison above is between frames that hold something: every frame has pixels that are not the clear colour)"""
    for frame, px in runs["off"][0].items():
        assert len(np.unique(px.reshape(-1, 4), axis=0)) > 16, frame


@pytest.mark.gpu
def test_which_launches_take_the_form(runs):
    """Off: never.  On: never on a context's first frame (no order yet), never for frames with partial strips, a pitch that is no multiple
    of 4 or a stripe; from the second frame on everywhere else -- the second frame with what the host knew when it was scheduled, the third
    with the sorting waves' count.  A forced build (tools/suite_off_defaults.sh) is not the no-clip build: never."""
    forced = os.environ.get("FDH_FORCE_KERNEL_PATHS") in ("1", "2", "3", "8", "19")
    for name, bins in runs["off"][1].items():
        assert all(b == -1 for b in bins), ("off", name, bins)
    for setting in ("on8", "on254"):
        for name, (w, h, _, _, scenes, can) in SEQUENCES.items():
            bins = runs[setting][1][name]
            assert bins[0] == -1, (setting, name, bins)
            if not can or forced:
                assert all(b == -1 for b in bins), (setting, name, bins)
            else:
                assert all(b >= 0 for b in bins[1:]), (setting, name, bins)
    if forced:
        return
    n_bins = lambda name: ((SEQUENCES[name][0] + 63) // 64) * ((SEQUENCES[name][1] + 63) // 64)
    for name in SEQUENCES:
        if SEQUENCES[name][5]:  # a threshold of 254: every bin of these frames, once the count is known
            assert runs["on254"][1][name][2] == n_bins(name), (name, runs["on254"][1][name])
    # a threshold of 8 on the piles: one bin is over it, so the longest bin of each of the eight classes keeps one wave per strip
    for name in ("piles_opaque", "piles_translucent"):
        assert runs["on8"][1][name][2] == 8, (name, runs["on8"][1][name])
    # ... and a frame that piles 40 draws into an empty bin is scheduled with the boundary of the frames before it
    assert runs["on8"][1]["stale"][3] == 8, runs["on8"][1]["stale"]


def test_the_piles_hold_the_draws_they_say():
    """(no GPU) one draw per node of a pile: the counts in PILES are the bins' list lengths"""
    from figdraw_amd.context import HipContext

    for piles in (PILES, PILES_40):
        rec = HipContext(record_only=True)
        rec.record_begin()
        rec.render_frame(piles_scene(piles), 512, 128)
        calls = rec.record_calls()
        rec.close()
        draws = [c for c in calls if c[0] == "draw_rounded_rect_sdf"]
        assert len(draws) == sum(piles) and sum(piles) > 64, (len(draws), sum(piles), sorted({str(c[0]) for c in calls}))


def test_a_context_that_has_launched_nothing_reports_no_block_waves():
    """(no GPU) include_schedule/figdraw_hip_schedule.h: the entry point is exported, and -1 before any full-frame launch"""
    from figdraw_amd.context import HipContext

    rec = HipContext(record_only=True)
    rec.render_frame(piles_scene(PILES), 512, 128)
    assert rec.block_wave_bins() == -1
    rec.close()
    hdr = open(os.path.join(ROOT, "include_schedule", "figdraw_hip_schedule.h")).read()
    assert "FDH_API int fdh_block_wave_bins(FdhContext*, int* out);" in hdr
