"""The tensor case of tests/test_device_image.py, a process of its own (torch loads its own copies of the ROCm libraries: they stay out of
the suite's process): CHW float32, CHW float16 and HWC uint8 tensors on the device through HipContext.put_image_tensor /
update_image_tensor against fdh_put_image / fdh_update_image of the bytes tests/device_image_ref.py makes of them.  Prints
"device_image_tensor_child: OK"."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import device_image_cases as DC  # noqa: E402
import device_image_ref as REF  # noqa: E402


def same_atlases(a, b, what):
    assert a.atlas_usage() == b.atlas_usage(), what
    for l in range(a.atlas_size().bit_length()):
        assert np.array_equal(a.read_atlas_level(l), b.read_atlas_level(l)), (what, l)


def main():
    import torch

    from figdraw_amd.context import HipContext

    g = torch.Generator().manual_seed(18)
    t = (torch.rand((4, 77, 130), generator=g) * 1.4 - 0.2).to("cuda:0")
    t[0, 13, 15], t[1, 14, 16], t[3, 5, 3] = float("nan"), float("inf"), -0.0  # (inside the view below)
    view = t[:, 5:70, 3:124]  # a pitch and a plane stride that are not the view's extent
    torch.cuda.synchronize()
    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    texels = REF.convert(view.cpu().numpy().copy(), REF.PLANAR_F32, REF.STRAIGHT_ALPHA)
    assert np.isnan(view.cpu().numpy()).sum() == 1
    assert dev.put_image_tensor(1, view, straight_alpha=True) == host.put_image(1, texels) == (4, 4, 121, 65)
    same_atlases(dev, host, "a tensor")
    hwc = torch.from_numpy(DC.noise_rgba(np.random.default_rng(19), 40, 50)).to("cuda:0")
    half = t[:3, 5:70, 3:124].half().contiguous()
    torch.cuda.synchronize()
    dev.update_image_tensor(1, half)
    host.update_image(1, REF.convert(half.cpu().numpy().copy(), REF.PLANAR_F16))
    assert dev.put_image_tensor(2, hwc) == host.put_image(2, hwc.cpu().numpy())
    same_atlases(dev, host, "tensors")
    try:
        dev.put_image_tensor(3, t.permute(1, 2, 0))
    except ValueError:
        pass
    else:
        raise AssertionError("an H x W x C float tensor went through")
    dev.close(), host.close()
    print("device_image_tensor_child: OK")


if __name__ == "__main__":
    main()
