"""The tensor case of tests/test_device_images.py, a process of its own (torch loads its own copies of the ROCm libraries: they stay out of
the suite's process): an N x C x H x W float16 tensor on the device through HipContext.put_image_tensors / update_image_tensors, cut along
its first axis without a copy, against N put_image_tensor / update_image_tensor calls.  Prints "device_images_tensor_child: OK"."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def same_atlases(a, b, what):
    assert a.atlas_usage() == b.atlas_usage(), what
    for l in range(a.atlas_size().bit_length()):
        assert np.array_equal(a.read_atlas_level(l), b.read_atlas_level(l)), (what, l)


def main():
    import torch

    from figdraw_amd.context import HipContext

    g = torch.Generator().manual_seed(28)
    n = 6
    t = (torch.rand((n, 4, 77, 130), generator=g) * 1.4 - 0.2).half().to("cuda:0")
    t[0, 0, 13, 15], t[1, 1, 14, 16], t[5, 3, 6, 4] = float("nan"), float("inf"), -0.0  # (inside the view below)
    view = t[:, :, 5:70, 3:124]  # a pitch and a plane stride that are not the view's extent
    nhwc = (torch.rand((3, 40, 50, 4), generator=g) * 255).to(torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    batch, single = HipContext(atlas_size=512, device=0), HipContext(atlas_size=512, device=0)
    keys = list(range(1, n + 1))
    got = batch.put_image_tensors(keys, view, straight_alpha=True)
    assert got == [single.put_image_tensor(k, view[k - 1], straight_alpha=True) for k in keys] and got[0][2:] == (121, 65)
    assert batch.image_batch_stats()["launches"] == 2  # one format, and the tails
    same_atlases(batch, single, "N x C x H x W")
    assert batch.put_image_tensors([11, 12, 13], nhwc) == [single.put_image_tensor(11 + k, nhwc[k]) for k in range(3)]
    same_atlases(batch, single, "N x H x W x 4")
    three = [view[4, :3], view[2, :1], view[0]]  # a sequence of tensors of other channel counts, for the entries 2, 5, 3
    batch.update_image_tensors([2, 5, 3], three)
    for k, x in zip((2, 5, 3), three):
        single.update_image_tensor(k, x)
    same_atlases(batch, single, "updates")
    batch.close(), single.close()
    print("device_images_tensor_child: OK")


if __name__ == "__main__":
    main()
