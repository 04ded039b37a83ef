"""GPU suite: what a recorded frame hands the device is what the commit before RecordedFrame / FrameEnv / CallLog handed it.

fdh_debug_record_digest (tests/test_recorded_frame_host.py) does not see BinRec flags and core bands, the list stride, the deepest clip,
the blur jobs or phase 0's fragment counts -- what the frame's bookkeeping computes.  The device does: tests/golden/
recorded_frame_gpu_pins.json holds, per frame of each case, as the library of that commit gave them on an MI355X (tools/
make_recorded_frame_pins.py --gpu): the sha256 of the frame's pixels; the eight words of fdh_debug_bin_digest where the frame has a bin
launch (a direct frame -- no phase of more than 64 draws -- has none, and its count buffer holds what the allocation held: not pinned);
fdh_debug_verify_upload's out[0..2] == 0 and out[10..11] (out[10], the number of pieces, only where the calling thread records alone or the
pieces were consolidated into one: with pool threads it is decided by which thread took which chunk -- the parent itself gave 5, then 7
for two frames of one scene); fdh_last_upload_bytes; the integer fields of FdhFrameStats.  The shapes are the
smallest at which each path still exists; every case is a handful of frames."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import ref_scenes as RS
from figdraw_amd import scene as S
from figdraw_amd.context import HipContext
from test_recorded_frame_host import consolidate_scene, rects_scene, retained_sequence

pytestmark = pytest.mark.gpu
PIN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recorded_frame_gpu_pins.json")


def snap(ctx, binned, pieces=True):
    px = ctx.read_pixels()
    out = {"pixels": hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest()}
    if binned:
        words = (C.c_uint64 * 8)()
        ctx._ck(ctx.L.fdh_debug_bin_digest(ctx.h, words))
        out["bin_digest"] = [f"{v:016x}" for v in words]
    v = ctx.verify_upload()
    out["upload"] = {"differ": v[0:3], "records": v[11]}
    if pieces:
        out["upload"]["pieces"] = v[10]
    out["upload_bytes"] = ctx.last_upload_bytes()
    st = ctx.frame_stats()
    out["stats"] = {"fragments": st.fragments, "by_mode": list(st.fragments_main_by_mode), "elliptical": st.fragments_main_elliptical,
                    "other": st.fragments_main_other, "bytes_algorithmic": st.bytes_algorithmic, "clear_folded": st.clear_folded,
                    "n_draws": st.n_draws, "n_phases": st.n_phases, "n_blurs": st.n_blurs}
    return out


def frames(scene, w, h, threads=0, binned=True, n=2, pieces=None):
    ctx = HipContext(device=0)
    ctx.set_walk_threads(threads)
    out = []
    for _ in range(n):
        ctx.render_frame(scene, w, h)
        out.append(snap(ctx, binned, pieces=threads == 0 if pieces is None else pieces))
    ctx.close()
    return out


def clip_scene(kids, w=320, h=200):
    """`kids` siblings under a clipping parent"""
    lst = S.RenderList()
    parent = lst.addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(10, 10, w - 20, h - 20), fill=S.rgba(230, 230, 240, 255), corners=[14] * 4, flags=S.FigFlags.NfClipContent))
    for k in range(kids):
        lst.addChild(parent, S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(5.0 * k, 3.0 * k, 40, 30), corners=[k % 5] * 4, fill=S.rgba((k * 41) & 255, 90, (k * 17) & 255, 255)))
    sc = S.Renders()
    sc.setLayer(0, lst)
    return sc


def blur_in_clip_scene(w=320, h=200):
    lst = S.RenderList()
    lst.addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(0, 0, w, h), fill=S.rgba(40, 160, 90, 255)))
    for k in range(12):
        lst.addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(25.0 * k, 14.0 * k, 50, 24), corners=[3] * 4, fill=S.rgba(250, (k * 20) & 255, 30, 255)))
    parent = lst.addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(30, 20, 260, 160), fill=S.rgba(255, 255, 255, 60), corners=[20] * 4, flags=S.FigFlags.NfClipContent))
    lst.addChild(parent, S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(20, 40, 120, 60), fill=S.rgba(0, 0, 200, 255)))
    lst.addChild(parent, S.Fig(kind=S.FigKind.nkBackdropBlur, screenBox=S.rect(60, 50, 180, 100), blur=10.0, corners=[8] * 4, fill=S.rgba(255, 255, 255, 50)))
    lst.addChild(parent, S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(200, 30, 120, 150), fill=S.rgba(200, 0, 0, 180), corners=[6] * 4))
    sc = S.Renders()
    sc.setLayer(0, lst)
    return sc


def case_bin_frame():
    return frames(rects_scene(200, 320, 200), 320, 200)


def case_direct_frame():
    return frames(rects_scene(40, 320, 200), 320, 200, binned=False)


def case_blurs():  # a full-frame blur (the fused route) and a 96 x 64 node (the one-kernel small route): three phases
    sc = rects_scene(200, 320, 200, blurs=((0, 0, 320, 200, 12.0), (100, 60, 96, 64, 6.0)))
    return {f"t{t}": frames(sc, 320, 200, threads=t) for t in (0, 3)}


def case_blur_in_clip():  # the two-pass route (clip state to carry), the clip reopened in the next phase
    return frames(blur_in_clip_scene(), 320, 200, binned=False)


def case_spill_plane():
    return frames(RS.deep_clips(128.0, 128.0, depth=18), 128, 128, binned=False)


def case_siblings_under_clip():
    return frames(clip_scene(60), 320, 200, threads=3, binned=False)


def case_consolidate():
    return frames(consolidate_scene(), 800, 600, threads=3, pieces=True)


def case_wide_frame():
    return frames(rects_scene(80, 8200, 64, seed=3), 8200, 64)


def case_retained():  # four renders after the retain: patch_runs uploads what differs from the shadow
    ctx = HipContext(device=0)
    steps = {}
    retained_sequence(ctx, on_render=lambda c, step: steps.__setitem__(step, snap(c, False)))
    ctx.close()
    return steps


def case_picking():
    ctx = HipContext(device=0)
    ctx.set_pick(True)
    ctx.render_frame(RS.nested_clips(128.0, 128.0), 128, 128)
    out = snap(ctx, False)
    region = ctx.pick_region(0, 0, 128, 128)
    out["region"] = hashlib.sha256(np.ascontiguousarray(region, dtype=np.int32).tobytes()).hexdigest()
    out["tags"] = ctx.pick_draw_tags().tolist()
    ctx.close()
    return out


CASES = {"bin_frame": case_bin_frame, "direct_frame": case_direct_frame, "blurs": case_blurs, "blur_in_clip": case_blur_in_clip, "spill_plane": case_spill_plane,
         "siblings_under_clip": case_siblings_under_clip, "consolidate": case_consolidate, "wide_frame": case_wide_frame, "retained": case_retained,
         "picking": case_picking}


@pytest.fixture(scope="module")
def pins():
    with open(PIN_FILE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_reach_the_device_as_the_parent_sent_them(name, pins):
    got = json.loads(json.dumps(CASES[name]()))
    want = pins[name]
    if isinstance(got, dict):
        assert sorted(got) == sorted(want)
        for key in got:
            assert got[key] == want[key], f"{name}/{key}"
    assert got == want


def test_the_cases_reach_the_paths_they_are_for(pins):
    assert all(f["upload"]["differ"] == [0, 0, 0] for f in pins["bin_frame"] + pins["consolidate"] + pins["wide_frame"])
    assert pins["blurs"]["t0"][0]["stats"]["n_phases"] == 3 and pins["blurs"]["t3"][0]["stats"]["n_blurs"] == 2
    assert pins["blur_in_clip"][0]["stats"]["n_phases"] == 2
    assert pins["consolidate"][0]["upload"]["pieces"] == 1
    assert pins["retained"]["update_nodes"]["upload_bytes"] < pins["retained"]["retain"]["upload_bytes"]
    assert len(pins["picking"]["tags"]) == pins["picking"]["upload"]["records"]
