"""The decoder-surface case of tests/test_video_frame.py, a process of its own (torch loads its own copies of the ROCm libraries: they stay
out of the suite's process): one torch allocation on the device that holds an NV12 surface the way a decoder lays it out -- `height` rows
of luma at a pitch wider than the frame, the chroma rows behind them at pitch * height -- goes through HipContext.put_video_frame /
update_video_frame as two views of that allocation, against fdh_put_image / fdh_update_image of the bytes tests/video_frame_ref.py makes
of it.  Prints "video_frame_tensor_child: OK"."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import video_frame_ref as REF  # noqa: E402


def same_atlases(a, b, what):
    assert a.atlas_usage() == b.atlas_usage(), what
    for l in range(a.atlas_size().bit_length()):
        assert np.array_equal(a.read_atlas_level(l), b.read_atlas_level(l)), (what, l)


def main():
    import torch

    from figdraw_amd.context import HipContext

    w, h, pitch = 150, 90, 256  # the surface: 90 rows of luma and 45 of chroma, 256 bytes apart
    g = torch.Generator().manual_seed(21)
    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    for step, flags in enumerate((0, REF.CHROMA_LINEAR)):
        surface = torch.randint(0, 256, (h + h // 2, pitch), generator=g, dtype=torch.uint8).to("cuda:0")
        luma, chroma = surface[:h], surface[h:]  # two views of one allocation
        assert chroma.data_ptr() == luma.data_ptr() + pitch * h
        torch.cuda.synchronize()
        cpu = surface.cpu().numpy()
        texels = REF.convert(cpu[:h, :w].copy(), cpu[h:, :w].reshape(h // 2, w // 2, 2).copy(), REF.NV12, REF.BT709, REF.LIMITED, flags)
        if step == 0:
            r = dev.put_video_frame(1, luma.data_ptr(), chroma.data_ptr(), w, h, pitch, pitch, REF.NV12, REF.BT709, REF.LIMITED, flags)
            assert r == host.put_image(1, texels) == (4, 4, w, h)
        else:
            dev.update_video_frame(1, luma.data_ptr(), chroma.data_ptr(), w, h, pitch, pitch, REF.NV12, REF.BT709, REF.LIMITED, flags)
            host.update_image(1, texels)
        same_atlases(dev, host, f"a decoder surface, flags {flags}")
    dev.close(), host.close()
    print("video_frame_tensor_child: OK")


if __name__ == "__main__":
    main()
