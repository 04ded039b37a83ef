"""The order in which the image and video imports (figdraw_amd/csrc/fdh_import.h, class Importer) ask their questions, as a record-only
context shows it, over the ten single calls and the four batch calls: what the struct is refused for comes before "unknown key" and
"size mismatch", a refused call leaves the atlas as it was, and the same key can be put afterwards.  No device, no kernel: on a record-only
context the pointers are looked at (null, alignment) and never followed."""
import pytest

from figdraw_amd.context import FigdrawHipError, HipContext

P = 0x10000  # the planes: addresses nobody follows, aligned for every format here


def half(v):
    return (v + 1) // 2


# name of the call as its refusals give it -> (the method, what it takes behind the key for a frame of w x h)
SINGLE = {
    "image_device": lambda w, h: (P, w, h, 4 * w),                                                          # RGBA8
    "video_frame": lambda w, h: (P, 2 * P, w, h, w, 2 * half(w)),                                            # NV12
    "video_planes": lambda w, h: ((P, 2 * P, 3 * P), w, h, (w, half(w), half(w))),                           # I420
    "video_422": lambda w, h: ((P, 2 * P, 3 * P), w, h, (w, half(w), half(w))),                              # I422
    "video_alpha": lambda w, h: ((P, 2 * P, 3 * P, 4 * P), w, h, (w, half(w), half(w), w)),                  # A420
}
BATCH = {
    "images_device": lambda key, w, h: [(key, P, w, h, 4 * w)],
    "video_frames": lambda key, w, h: [(key, P, 2 * P, w, h, w, 2 * half(w))],
}
EMPTY = {"image_device": "empty image", "images_device": "empty image"}  # (every other family: "empty frame")


def calls():
    """(the call's name, put or update, call(ctx, key, w, h))"""
    out = []
    for verb in ("put", "update"):
        for family, args in SINGLE.items():
            out.append((f"{verb}_{family}", verb, lambda ctx, key, w, h, m=f"{verb}_{family}", a=args: getattr(ctx, m)(key, *a(w, h))))
        for family, items in BATCH.items():
            out.append((f"{verb}_{family}", verb, lambda ctx, key, w, h, m=f"{verb}_{family}", i=items: getattr(ctx, m)(i(key, w, h))))
    return out


CALLS = calls()
PUTS = {name[len("put_"):]: call for name, verb, call in CALLS if verb == "put"}


def state(ctx):
    u = ctx.atlas_usage()
    return u["epoch"], u["entries"], u


def refused(call, ctx, key, w, h):
    with pytest.raises(FigdrawHipError) as e:
        call(ctx, key, w, h)
    assert e.value.code == -1
    return str(e.value)


def test_the_table_is_every_call():
    assert len(CALLS) == 14 and len({name for name, _, _ in CALLS}) == 14
    assert sum(verb == "update" for _, verb, _ in CALLS) == 7


@pytest.mark.parametrize("name,verb,call", CALLS, ids=[c[0] for c in CALLS])
def test_the_struct_is_asked_first(name, verb, call):
    """(a): width = 0 and a key the atlas has never seen"""
    ctx = HipContext(atlas_size=64, record_only=True)
    family = name[len(verb) + 1:]
    PUTS[family](ctx, 1, 2, 2)
    before = state(ctx)
    text = refused(call, ctx, 77, 0, 2)
    assert text == f"[-1] {name}: {EMPTY.get(family, 'empty frame')}", text
    assert "unknown key" not in text and "size mismatch" not in text
    assert state(ctx) == before and not ctx.has_image(77)
    ctx.close()


@pytest.mark.parametrize("name,verb,call", [c for c in CALLS if c[1] == "update"], ids=[c[0] for c in CALLS if c[1] == "update"])
def test_then_the_key_and_the_size(name, verb, call):
    """(b): a valid struct and an unknown key; a valid struct of another size than the entry's"""
    ctx = HipContext(atlas_size=64, record_only=True)
    family = name[len("update_"):]
    assert PUTS[family](ctx, 1, 2, 2) is not None
    before = state(ctx)
    assert refused(call, ctx, 77, 2, 2) == f"[-1] {name}: unknown key"
    assert refused(call, ctx, 1, 4, 2) == f"[-1] {name}: size mismatch"
    assert refused(call, ctx, 1, 2, 4) == f"[-1] {name}: size mismatch"
    assert state(ctx) == before
    call(ctx, 1, 2, 2)  # and the entry's own size is taken
    after = state(ctx)
    assert after[1] == before[1] and after[0] > before[0]
    ctx.close()


@pytest.mark.parametrize("name,verb,call", [c for c in CALLS if c[1] == "put"], ids=[c[0] for c in CALLS if c[1] == "put"])
def test_a_refused_put_leaves_nothing(name, verb, call):
    """(c): epoch, entry count and usage are what they were; the same key is put afterwards"""
    ctx = HipContext(atlas_size=64, record_only=True)
    call(ctx, 1, 2, 2)
    before = state(ctx)
    for w, h in ((0, 2), (2, 0), (-3, 2)):
        assert "empty" in refused(call, ctx, 5, w, h)
        assert state(ctx) == before and not ctx.has_image(5)
    call(ctx, 5, 2, 2)
    after = state(ctx)
    assert ctx.has_image(5) and ctx.image_rect(5)[2:] == (2, 2)
    assert after[1] == before[1] + 1 and after[0] > before[0]
    ctx.close()
