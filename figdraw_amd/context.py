"""HipContext: the BackendContext-shaped Python binding over libfigdraw_hip.so.

Method names follow the reference's `BackendContext` (src/figdraw/figbackend.nim:245-705) in
snake_case; `render_frame` is `renderFrame` (figrender.nim:1960-1995).  There is no fallback: if
the shared library is missing or no gfx950 GPU is usable, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import numpy as np

from . import scene as S

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfigdraw_hip.so")
_lib = None

_F4 = C.c_float * 4
_F2 = C.c_float * 2
_COL4 = S.CColor * 4


class FigdrawHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class FrameStats(C.Structure):
    _fields_ = [("n_draws", C.c_int32), ("n_phases", C.c_int32), ("n_blurs", C.c_int32), ("n_bins", C.c_int32),
                ("ms_total", C.c_float), ("ms_bin", C.c_float), ("ms_composite", C.c_float),
                ("ms_composite_main", C.c_float), ("ms_blur_h", C.c_float), ("ms_blur_v", C.c_float),
                ("bytes_algorithmic", C.c_int64), ("bytes_composite_main", C.c_int64), ("bytes_blur", C.c_int64),
                ("fragments", C.c_int64), ("ms_host_record", C.c_float), ("ms_host_upload", C.c_float),
                ("ms_host_launch", C.c_float), ("clear_folded", C.c_float),
                ("ms_blur_big_h", C.c_float), ("ms_blur_big_v", C.c_float), ("bytes_blur_big_h", C.c_int64), ("bytes_blur_big_v", C.c_int64),
                ("fragments_main_by_mode", C.c_int64 * 4), ("fragments_main_elliptical", C.c_int64), ("fragments_main_other", C.c_int64),
                ("flops_composite_main", C.c_int64), ("ms_blur_fused", C.c_float), ("deep_bins", C.c_float),
                ("bytes_blur_fused", C.c_int64), ("bytes_frame_implementation", C.c_int64)]


class GlyphOutline(C.Structure):  # FdhGlyphOutline, include_glyphs/figdraw_hip_glyphs.h
    _fields_ = [("key", C.c_int64), ("segs", C.c_void_p), ("n_segs", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("sdf_range", C.c_uint32)]


class GlyphBatchStats(C.Structure):  # FdhGlyphBatchStats
    _fields_ = [("glyphs", C.c_int32), ("written", C.c_int32), ("dropped_by_growth", C.c_int32), ("tiles", C.c_int32), ("edges", C.c_int32),
                ("launches", C.c_int32), ("bytes_copied", C.c_int64)]


class AtlasMoveStats(C.Structure):  # FdhAtlasMoveStats (include_glyphs/figdraw_hip_atlas.h)
    _fields_ = [("entries", C.c_int32), ("rects_moved", C.c_int32), ("texels", C.c_int64), ("tiles", C.c_int32), ("launches", C.c_int32),
                ("size_before", C.c_int32), ("size_after", C.c_int32), ("packed_before", C.c_int64), ("packed_after", C.c_int64),
                ("us_pack", C.c_int32), ("us_alloc", C.c_int32), ("us_tables", C.c_int32), ("us_move", C.c_int32)]


class AtlasUsage(C.Structure):  # FdhAtlasUsage
    _fields_ = [("size", C.c_int32), ("entries", C.c_int32), ("used_area", C.c_int64), ("packed_area", C.c_int64), ("epoch", C.c_uint64),
                ("rebuilds", C.c_int64), ("compactions", C.c_int64)]


class DeviceImage(C.Structure):  # FdhDeviceImage (include_glyphs/figdraw_hip_device_image.h)
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("pitch_bytes", C.c_int64), ("plane_bytes", C.c_int64),
                ("format", C.c_uint32), ("channels", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class ImageBatchStats(C.Structure):  # FdhImageBatchStats (include_glyphs/figdraw_hip_device_images.h)
    _fields_ = [("images", C.c_int32), ("written", C.c_int32), ("dropped_by_growth", C.c_int32), ("tiles", C.c_int32), ("launches", C.c_int32),
                ("reserved", C.c_int32), ("bytes_copied", C.c_int64)]


IMAGE_RGBA8, IMAGE_PLANAR_F32, IMAGE_PLANAR_F16 = 0, 1, 2  # FdhDeviceImage.format
IMAGE_STRAIGHT_ALPHA = 1                                   # FdhDeviceImage.flags


class VideoBatchStats(C.Structure):  # FdhVideoBatchStats (include_glyphs/figdraw_hip_video_frames.h)
    _fields_ = [("frames", C.c_int32), ("written", C.c_int32), ("dropped_by_growth", C.c_int32), ("tiles", C.c_int32), ("launches", C.c_int32),
                ("reserved", C.c_int32), ("bytes_copied", C.c_int64)]


class VideoFrame(C.Structure):  # FdhVideoFrame (include_glyphs/figdraw_hip_video_frame.h)
    _fields_ = [("planes", C.c_void_p * 2), ("pitch_bytes", C.c_int64 * 2), ("width", C.c_int32), ("height", C.c_int32),
                ("format", C.c_uint32), ("matrix", C.c_uint32), ("range", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


VIDEO_BGRA8, VIDEO_NV12, VIDEO_P010 = 0, 1, 2                                     # FdhVideoFrame.format
VIDEO_BT601, VIDEO_BT709, VIDEO_BT2020 = 0, 1, 2                                   # FdhVideoFrame.matrix
VIDEO_LIMITED, VIDEO_FULL = 0, 1                                                   # FdhVideoFrame.range
VIDEO_CHROMA_LINEAR, VIDEO_STRAIGHT_ALPHA, VIDEO_IGNORE_ALPHA = 1, 2, 4            # FdhVideoFrame.flags


def video_frame(y_ptr, uv_ptr, width, height, pitch_y, pitch_uv, format, matrix=0, range=0, flags=0) -> VideoFrame:
    f = VideoFrame()
    f.planes[0], f.planes[1] = y_ptr or None, uv_ptr or None
    f.pitch_bytes[0], f.pitch_bytes[1] = int(pitch_y), int(pitch_uv)
    f.width, f.height, f.format, f.matrix, f.range, f.flags = int(width), int(height), int(format), int(matrix), int(range), int(flags)
    return f


def video_coefficients(format, matrix, range):
    """Yoff, Coff, cY, cRV, cGU, cGV, cBU of the integer YCbCr -> RGB conversion (fdh_video_coefficients): host only, no context"""
    L = load()
    out = (C.c_int32 * 7)()
    if L.fdh_video_coefficients(int(format), int(matrix), int(range), out) != 0:
        raise FigdrawHipError(-1, L.fdh_last_error().decode())
    return tuple(out)


def _video_target(t, ptrs, pitches, format, matrix, range, flags, rect):
    """the fields of a fresh VideoTarget, VideoPlanesTarget or VideoAlphaPlanesTarget: as many planes as it has"""
    for p, _ in enumerate(t.planes):
        t.planes[p], t.pitch_bytes[p] = ptrs[p] or None, int(pitches[p])
    t.rect[0], t.rect[1], t.rect[2], t.rect[3] = (int(v) for v in (rect if rect is not None else (0, 0, 0, 0)))
    t.format, t.matrix, t.range, t.flags = int(format), int(matrix), int(range), int(flags)
    return t


def _check_video(call, target, frame_w, frame_h):
    """one of the four fdh_check_video_*_target on `target`, or on None"""
    L = load()
    code = getattr(L, call)(C.byref(target) if target is not None else None, int(frame_w), int(frame_h))
    if code != 0:
        raise FigdrawHipError(code, L.fdh_last_error().decode())


class VideoTarget(C.Structure):  # FdhVideoTarget (include_video/figdraw_hip_video_out.h)
    _fields_ = [("planes", C.c_void_p * 2), ("pitch_bytes", C.c_int64 * 2), ("rect", C.c_int32 * 4),
                ("format", C.c_uint32), ("matrix", C.c_uint32), ("range", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


def video_target(y_ptr, uv_ptr, pitch_y, pitch_uv, format=VIDEO_NV12, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0, rect=None) -> VideoTarget:
    return _video_target(VideoTarget(), (y_ptr, uv_ptr), (pitch_y, pitch_uv), format, matrix, range, flags, rect)


def video_out_coefficients(format, matrix, range):
    """Yoff, Coff, kYR, kYG, kYB, kUR, kUG, kUB, kVR, kVG, kVB of the integer RGB -> YCbCr conversion (fdh_video_out_coefficients): host only,
    no context"""
    L = load()
    out = (C.c_int32 * 11)()
    if L.fdh_video_out_coefficients(int(format), int(matrix), int(range), out) != 0:
        raise FigdrawHipError(-1, L.fdh_last_error().decode())
    return tuple(out)


def check_video_target(target, frame_w, frame_h):
    """every rule of fdh_read_video_frame that needs no device, for a frame of frame_w x frame_h (fdh_check_video_target): raises
    FigdrawHipError where the call would refuse `target` (a VideoTarget, or None)"""
    _check_video("fdh_check_video_target", target, frame_w, frame_h)


class VideoPlanes(C.Structure):  # FdhVideoPlanes (include_video/figdraw_hip_video_planar.h)
    _fields_ = [("planes", C.c_void_p * 3), ("pitch_bytes", C.c_int64 * 3), ("width", C.c_int32), ("height", C.c_int32),
                ("format", C.c_uint32), ("matrix", C.c_uint32), ("range", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class VideoPlanesTarget(C.Structure):  # FdhVideoPlanesTarget
    _fields_ = [("planes", C.c_void_p * 3), ("pitch_bytes", C.c_int64 * 3), ("rect", C.c_int32 * 4),
                ("format", C.c_uint32), ("matrix", C.c_uint32), ("range", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


VIDEO_I420, VIDEO_I010, VIDEO_I444, VIDEO_I410 = 3, 4, 5, 6                        # FdhVideoPlanes.format, FdhVideoPlanesTarget.format


def video_planes(ptrs, width, height, pitches, format=VIDEO_I420, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0) -> VideoPlanes:
    """ptrs, pitches: of Y, Cb, Cr"""
    f = VideoPlanes()
    for p in (0, 1, 2):
        f.planes[p], f.pitch_bytes[p] = ptrs[p] or None, int(pitches[p])
    f.width, f.height, f.format, f.matrix, f.range, f.flags = int(width), int(height), int(format), int(matrix), int(range), int(flags)
    return f


def video_planes_target(ptrs, pitches, format=VIDEO_I420, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0, rect=None) -> VideoPlanesTarget:
    return _video_target(VideoPlanesTarget(), ptrs, pitches, format, matrix, range, flags, rect)


def check_video_planes_target(target, frame_w, frame_h):
    """every rule of fdh_read_video_planes that needs no device, for a frame of frame_w x frame_h (fdh_check_video_planes_target): raises
    FigdrawHipError where the call would refuse `target` (a VideoPlanesTarget, or None)"""
    _check_video("fdh_check_video_planes_target", target, frame_w, frame_h)


VIDEO_I422, VIDEO_I210, VIDEO_YUY2, VIDEO_UYVY = 7, 8, 9, 10                       # ... for the 4:2:2 calls (include_video/figdraw_hip_video_422.h)


def check_video_422_target(target, frame_w, frame_h):
    """every rule of fdh_read_video_422 that needs no device, for a frame of frame_w x frame_h (fdh_check_video_422_target): raises
    FigdrawHipError where the call would refuse `target` (a VideoPlanesTarget, or None)"""
    _check_video("fdh_check_video_422_target", target, frame_w, frame_h)


class VideoAlphaPlanes(C.Structure):  # FdhVideoAlphaPlanes (include_video/figdraw_hip_video_alpha.h)
    _fields_ = [("planes", C.c_void_p * 4), ("pitch_bytes", C.c_int64 * 4), ("width", C.c_int32), ("height", C.c_int32),
                ("format", C.c_uint32), ("matrix", C.c_uint32), ("range", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class VideoAlphaPlanesTarget(C.Structure):  # FdhVideoAlphaPlanesTarget
    _fields_ = [("planes", C.c_void_p * 4), ("pitch_bytes", C.c_int64 * 4), ("rect", C.c_int32 * 4),
                ("format", C.c_uint32), ("matrix", C.c_uint32), ("range", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


VIDEO_A420, VIDEO_A444, VIDEO_A410, VIDEO_UYVA = 11, 12, 13, 14                    # FdhVideoAlphaPlanes.format, FdhVideoAlphaPlanesTarget.format


def video_alpha_planes(ptrs, width, height, pitches, format=VIDEO_A420, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0) -> VideoAlphaPlanes:
    """ptrs, pitches: of Y, Cb, Cr, A; UYVA: (the UYVY plane, 0, 0, A)"""
    f = VideoAlphaPlanes()
    for p in (0, 1, 2, 3):
        f.planes[p], f.pitch_bytes[p] = ptrs[p] or None, int(pitches[p])
    f.width, f.height, f.format, f.matrix, f.range, f.flags = int(width), int(height), int(format), int(matrix), int(range), int(flags)
    return f


def video_alpha_planes_target(ptrs, pitches, format=VIDEO_A420, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0, rect=None) -> VideoAlphaPlanesTarget:
    return _video_target(VideoAlphaPlanesTarget(), ptrs, pitches, format, matrix, range, flags, rect)


def check_video_alpha_target(target, frame_w, frame_h):
    """every rule of fdh_read_video_alpha that needs no device, for a frame of frame_w x frame_h (fdh_check_video_alpha_target): raises
    FigdrawHipError where the call would refuse `target` (a VideoAlphaPlanesTarget, or None)"""
    _check_video("fdh_check_video_alpha_target", target, frame_w, frame_h)


def tensor_image(t, straight_alpha: bool = False) -> DeviceImage:
    """the FdhDeviceImage of a tensor: any object with data_ptr(), shape, stride(), dtype and element_size() (a torch tensor; torch is not
    imported here).  H x W x 4 uint8 is RGBA8; C x H x W (C = 1, 3, 4) or H x W of float32 / float16 is planar.  A layout that is not a row
    pitch plus a plane stride over unit-stride rows raises ValueError."""
    shape, stride, es = tuple(int(v) for v in t.shape), tuple(int(v) for v in t.stride()), int(t.element_size())
    dtype = str(t.dtype).split(".")[-1]
    flags = IMAGE_STRAIGHT_ALPHA if straight_alpha else 0
    if dtype == "uint8":
        if len(shape) != 3 or shape[2] != 4:
            raise ValueError(f"a uint8 image is H x W x 4 (RGBA8), not {shape}")
        h, w = shape[:2]
        if stride[2] != 1 or stride[1] != 4 or (h > 1 and stride[0] < 4 * w):
            raise ValueError(f"strides {stride} of an H x W x 4 image are not a row pitch over packed texels")
        return DeviceImage(t.data_ptr(), w, h, stride[0] if h > 1 else 4 * w, 0, IMAGE_RGBA8, 4, flags, 0)
    if dtype not in ("float32", "float16"):
        raise ValueError(f"dtype {t.dtype}: uint8 (H x W x 4), float32 or float16 (C x H x W or H x W)")
    if len(shape) == 2:
        shape, stride = (1,) + shape, (0,) + stride
    if len(shape) != 3 or shape[0] not in (1, 3, 4):
        raise ValueError(f"a planar image is C x H x W with C = 1, 3 or 4, or H x W, not {tuple(t.shape)}")
    c, h, w = shape
    pitch = stride[1] * es if h > 1 else w * es
    plane = stride[0] * es if c > 1 else 0
    if stride[2] != 1 or pitch < w * es or (c > 1 and plane < pitch * h):
        raise ValueError(f"strides {tuple(t.stride())} are not a plane stride and a row pitch over unit-stride rows")
    return DeviceImage(t.data_ptr(), w, h, pitch, plane, IMAGE_PLANAR_F32 if dtype == "float32" else IMAGE_PLANAR_F16, c, flags, 0)


class _TensorSlice:
    """index i along the first axis of a tensor, as tensor_image reads a tensor: the same memory, no copy"""

    def __init__(self, t, i):
        self.dtype, self.shape, self._stride, self._es = t.dtype, tuple(t.shape)[1:], tuple(t.stride())[1:], int(t.element_size())
        self._ptr = int(t.data_ptr()) + i * int(t.stride()[0]) * self._es

    def data_ptr(self):
        return self._ptr

    def stride(self):
        return self._stride

    def element_size(self):
        return self._es


def tensor_images(tensors, straight_alpha: bool = False):
    """the FdhDeviceImages of a sequence of what tensor_image takes, or of one N x C x H x W / N x H x W x 4 tensor cut along its first axis
    without a copy"""
    if hasattr(tensors, "data_ptr") and hasattr(tensors, "shape"):
        if len(tensors.shape) != 4:
            raise ValueError(f"one tensor for a batch is N x C x H x W or N x H x W x 4, not {tuple(tensors.shape)}")
        tensors = [_TensorSlice(tensors, i) for i in range(int(tensors.shape[0]))]
    return [tensor_image(t, straight_alpha) for t in tensors]


def build(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 the C-ABI library in-tree (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    args = ["make", "-C", csrc, "-s", "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("FIGDRAW_HIP_LIB", LIB_PATH)  # override: instrumented builds (csrc/Makefile `stats`)
    if not os.path.exists(path):
        raise FigdrawHipError(-2, f"{path} is missing: run __graft_entry__.build() (there is no CPU fallback)")
    L = C.CDLL(path)
    vp = C.c_void_p
    L.fdh_last_error.restype = C.c_char_p
    L.fdh_version.restype = C.c_char_p
    L.fdh_create.argtypes = [C.POINTER(vp), C.c_int, C.c_float, C.c_int, C.c_uint32]
    L.fdh_destroy.argtypes = [vp]
    L.fdh_set_stream.argtypes = [vp, vp]
    L.fdh_begin_frame.argtypes = [vp, C.c_int, C.c_int, C.c_int, _F4]
    L.fdh_end_frame.argtypes = [vp]
    L.fdh_save_transform.argtypes = [vp]
    L.fdh_restore_transform.argtypes = [vp]
    L.fdh_translate.argtypes = [vp, C.c_float, C.c_float]
    L.fdh_rotate.argtypes = [vp, C.c_float]
    L.fdh_scale.argtypes = [vp, C.c_float, C.c_float]
    L.fdh_apply_transform.argtypes = [vp, C.c_float * 16]
    L.fdh_transform_mirrors_y.argtypes = [vp, C.POINTER(C.c_int)]
    L.fdh_set_aa_factor.argtypes = [vp, C.c_float]
    L.fdh_get_aa_factor.argtypes = [vp, C.POINTER(C.c_float)]
    L.fdh_get_pixel_scale.argtypes = [vp, C.POINTER(C.c_float)]
    L.fdh_draw_rounded_rect_sdf.argtypes = [vp, _F4, _COL4, _F4, _F4, C.c_int, C.c_float, C.c_float, _F2, C.c_int,
                                            S.CColor, S.CColor, C.c_float]
    L.fdh_draw_rounded_rect_fill.argtypes = [vp, _F4, C.POINTER(S.CFill), _F4, _F4, C.c_int, C.c_float, C.c_float, _F2]
    L.fdh_draw_image.argtypes = [vp, C.c_int64, _F2, _COL4, _F2, C.c_int]
    L.fdh_draw_msdf.argtypes = [vp, C.c_int64, _F2, S.CColor, _F2, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]
    L.fdh_draw_image_adj.argtypes = [vp, C.c_int64, _F2, S.CColor, _F2]
    L.fdh_set_text_lcd_filtering.argtypes = [vp, C.c_int]
    L.fdh_get_text_lcd_filtering.argtypes = [vp, C.POINTER(C.c_int)]
    L.fdh_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.fdh_draw_quadratic_bezier_sdf.argtypes = [vp, _F4, C.POINTER(S.CFill), _F2, _F2, _F2, C.c_float, C.c_int]
    L.fdh_draw_filled_quad.argtypes = [vp, C.c_float * 8, _COL4]
    L.fdh_draw_rect.argtypes = [vp, _F4, S.CColor]
    L.fdh_draw_backdrop_blur.argtypes = [vp, _F4, _F4, _F4, C.c_float]
    L.fdh_begin_mask.argtypes = [vp, _F4, _F4, _F4]
    L.fdh_end_mask.argtypes = [vp]
    L.fdh_pop_mask.argtypes = [vp]
    L.fdh_begin_rect_mask.argtypes = [vp, _F4, _F4, _F4]
    L.fdh_pop_rect_mask.argtypes = [vp]
    L.fdh_set_text_subpixel_positioning.argtypes = [vp, C.c_int]
    L.fdh_set_text_subpixel_shift.argtypes = [vp, C.c_float]
    L.fdh_set_text_subpixel_glyph_variants.argtypes = [vp, C.c_int]
    L.fdh_put_image.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int * 4]
    L.fdh_update_image.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp]
    L.fdh_put_image_mips.argtypes = [vp, C.c_int64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int * 4]
    L.fdh_put_flippy.argtypes = [vp, C.c_int64, C.c_char_p, C.c_size_t, C.c_int * 4]
    L.fdh_remove_image.argtypes = [vp, C.c_int64]
    L.fdh_has_image.argtypes = [vp, C.c_int64, C.POINTER(C.c_int)]
    L.fdh_reset_atlas.argtypes = [vp, C.c_int]
    L.fdh_atlas_size.argtypes = [vp, C.POINTER(C.c_int)]
    L.fdh_atlas_packed_area.argtypes = [vp, C.POINTER(C.c_int64)]
    L.fdh_put_glyph_outline.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int, C.c_uint32, C.c_int * 4]
    L.fdh_put_glyph_image.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp, C.c_uint32, C.c_int * 4]
    if hasattr(L, "fdh_put_glyph_outlines"):  # include_glyphs/figdraw_hip_glyphs.h (absent from libraries built before it, as below)
        L.fdh_put_glyph_outlines.argtypes = [vp, vp, C.c_int, C.c_uint32, vp]
        L.fdh_glyph_batch_stats.argtypes = [vp, C.POINTER(GlyphBatchStats)]
        L.fdh_sizeof_glyph_outline.argtypes = []
    if hasattr(L, "fdh_put_glyph_outline_cubic"):  # include_glyphs/figdraw_hip_cubic.h
        L.fdh_put_glyph_outline_cubic.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int, C.c_uint32, C.c_int * 4]
    if hasattr(L, "fdh_put_glyph_coverage_batch"):  # include_glyphs/figdraw_hip_coverage.h
        L.fdh_put_glyph_coverage_batch.argtypes = [vp, vp, C.c_int, C.c_uint32, vp]
        L.fdh_glyph_coverage_batch_stats.argtypes = [vp, C.POINTER(GlyphBatchStats)]
    if hasattr(L, "fdh_put_glyph_outlines_cubic"):  # include_glyphs/figdraw_hip_cubic_batch.h
        L.fdh_put_glyph_outlines_cubic.argtypes = [vp, vp, C.c_int, C.c_uint32, vp]
        L.fdh_put_glyph_coverage_batch_cubic.argtypes = [vp, vp, C.c_int, C.c_uint32, vp]
    if hasattr(L, "fdh_put_image_sdf"):  # include_glyphs/figdraw_hip_image_sdf.h
        L.fdh_put_image_sdf.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int * 4]
        L.fdh_put_image_sdf_of.argtypes = [vp, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_uint32, C.c_int * 4]
    if hasattr(L, "fdh_put_image_device"):  # include_glyphs/figdraw_hip_device_image.h
        L.fdh_put_image_device.argtypes = [vp, C.c_int64, C.POINTER(DeviceImage), C.c_int * 4]
        L.fdh_update_image_device.argtypes = [vp, C.c_int64, C.POINTER(DeviceImage)]
    if hasattr(L, "fdh_put_images_device"):  # include_glyphs/figdraw_hip_device_images.h
        L.fdh_put_images_device.argtypes = [vp, vp, vp, C.c_int, vp]
        L.fdh_update_images_device.argtypes = [vp, vp, vp, C.c_int]
        L.fdh_image_batch_stats.argtypes = [vp, C.POINTER(ImageBatchStats)]
        L.fdh_sizeof_device_image.argtypes = []
    if hasattr(L, "fdh_put_video_frame"):  # include_glyphs/figdraw_hip_video_frame.h
        L.fdh_put_video_frame.argtypes = [vp, C.c_int64, C.POINTER(VideoFrame), C.c_int * 4]
        L.fdh_update_video_frame.argtypes = [vp, C.c_int64, C.POINTER(VideoFrame)]
        L.fdh_video_coefficients.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]
    if hasattr(L, "fdh_put_video_frames"):  # include_glyphs/figdraw_hip_video_frames.h
        L.fdh_put_video_frames.argtypes = [vp, vp, vp, C.c_int, vp]
        L.fdh_update_video_frames.argtypes = [vp, vp, vp, C.c_int]
        L.fdh_video_batch_stats.argtypes = [vp, C.POINTER(VideoBatchStats)]
        L.fdh_sizeof_video_frame.argtypes = []
        if L.fdh_sizeof_video_frame() != C.sizeof(VideoFrame):  # (the arrays of a batch are laid out here)
            raise ImportError(f"FdhVideoFrame is {L.fdh_sizeof_video_frame()} bytes in the library and {C.sizeof(VideoFrame)} in the binding")
    if hasattr(L, "fdh_read_video_frame"):  # include_video/figdraw_hip_video_out.h
        L.fdh_read_video_frame.argtypes = [vp, C.POINTER(VideoTarget)]
        L.fdh_check_video_target.argtypes = [C.POINTER(VideoTarget), C.c_int, C.c_int]
        L.fdh_video_out_coefficients.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]
    if hasattr(L, "fdh_put_video_planes"):  # include_video/figdraw_hip_video_planar.h
        L.fdh_put_video_planes.argtypes = [vp, C.c_int64, C.POINTER(VideoPlanes), C.c_int * 4]
        L.fdh_update_video_planes.argtypes = [vp, C.c_int64, C.POINTER(VideoPlanes)]
        L.fdh_read_video_planes.argtypes = [vp, C.POINTER(VideoPlanesTarget)]
        L.fdh_check_video_planes_target.argtypes = [C.POINTER(VideoPlanesTarget), C.c_int, C.c_int]
    if hasattr(L, "fdh_put_video_422"):  # include_video/figdraw_hip_video_422.h
        L.fdh_put_video_422.argtypes = [vp, C.c_int64, C.POINTER(VideoPlanes), C.c_int * 4]
        L.fdh_update_video_422.argtypes = [vp, C.c_int64, C.POINTER(VideoPlanes)]
        L.fdh_read_video_422.argtypes = [vp, C.POINTER(VideoPlanesTarget)]
        L.fdh_check_video_422_target.argtypes = [C.POINTER(VideoPlanesTarget), C.c_int, C.c_int]
    if hasattr(L, "fdh_put_video_alpha"):  # include_video/figdraw_hip_video_alpha.h
        L.fdh_put_video_alpha.argtypes = [vp, C.c_int64, C.POINTER(VideoAlphaPlanes), C.c_int * 4]
        L.fdh_update_video_alpha.argtypes = [vp, C.c_int64, C.POINTER(VideoAlphaPlanes)]
        L.fdh_read_video_alpha.argtypes = [vp, C.POINTER(VideoAlphaPlanesTarget)]
        L.fdh_check_video_alpha_target.argtypes = [C.POINTER(VideoAlphaPlanesTarget), C.c_int, C.c_int]
    if hasattr(L, "fdh_compact_atlas"):  # include_glyphs/figdraw_hip_atlas.h
        L.fdh_compact_atlas.argtypes = [vp, C.c_int, C.POINTER(AtlasMoveStats)]
        L.fdh_set_atlas_keep.argtypes = [vp, C.c_int]
        L.fdh_get_atlas_keep.argtypes = [vp, C.POINTER(C.c_int)]
        L.fdh_image_rect.argtypes = [vp, C.c_int64, C.c_int * 4]
        L.fdh_atlas_usage.argtypes = [vp, C.POINTER(AtlasUsage)]
        L.fdh_debug_read_atlas_level.argtypes = [vp, C.c_int, vp, C.c_int64]
    L.fdh_read_pixels.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.fdh_debug_read_surface.argtypes = [vp, C.c_int, vp]
    L.fdh_scene_retain.argtypes = [vp, vp, C.c_float, C.c_float, C.c_int, _F4]
    L.fdh_scene_update_nodes.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.fdh_scene_replace_root.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp]
    L.fdh_scene_insert_root.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp]
    L.fdh_scene_render.argtypes = [vp]
    L.fdh_scene_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.fdh_debug_record_digest.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.fdh_debug_verify_upload.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.fdh_debug_bin_digest.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.fdh_debug_staging_store_bytes.argtypes = [C.c_int, C.POINTER(C.c_int64)]
    L.fdh_last_upload_bytes.argtypes = [vp, C.POINTER(C.c_int64)]
    L.fdh_record_begin.argtypes = [vp]
    L.fdh_record_json.argtypes = [vp]
    L.fdh_record_json.restype = C.c_char_p
    L.fdh_frame_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.fdh_sync.argtypes = [vp]
    L.fdh_flush.argtypes = [vp]
    L.fdh_set_ui_scale.argtypes = [vp, C.c_float]
    L.fdh_render_frame.argtypes = [vp, vp, C.c_float, C.c_float, C.c_int, _F4]
    L.fdh_set_stripe.argtypes = [vp, C.c_int, C.c_int]
    L.fdh_set_blur_route.argtypes = [vp, C.c_int]
    L.fdh_set_cull.argtypes = [vp, C.c_int]
    L.fdh_culled_draws.argtypes = [vp, C.POINTER(C.c_int64)]
    L.fdh_set_walk_threads.argtypes = [vp, C.c_int]
    L.fdh_debug_host_times.argtypes = [vp, C.POINTER(C.c_int64)]
    L.fdh_walk_stats.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.fdh_stripe_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.fdh_comm_unique_id.argtypes = [C.c_char_p]
    L.fdh_comm_init.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    L.fdh_comm_destroy.argtypes = [vp]
    L.fdh_comm_share.argtypes = [vp, vp]
    L.fdh_gather_stripes.argtypes = [vp, C.c_int, vp]
    L.fdh_gather_frames.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.fdh_replay.argtypes = [vp, C.c_int]
    L.fdh_replay_async.argtypes = [vp, C.c_int]
    L.fdh_replay_timed.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.fdh_profile.argtypes = [vp, C.c_int]
    L.fdh_get_frame_stats.argtypes = [vp, C.POINTER(FrameStats)]
    if hasattr(L, "fdh_block_wave_bins"):  # (absent from libraries built before it, which FIGDRAW_HIP_LIB may name for an A/B)
        L.fdh_block_wave_bins.argtypes = [vp, C.POINTER(C.c_int)]
    # damage tracking (include/figdraw_hip_damage.h; absent from libraries built before it, which FIGDRAW_HIP_LIB may name for an A/B)
    if hasattr(L, "fdh_set_damage_tracking"):
        L.fdh_set_damage_tracking.argtypes = [vp, C.c_int]
        L.fdh_damage_bins.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.fdh_damage_changed_bins.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.fdh_damage_closure.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp]
    # damage readback (include/figdraw_hip_readback.h; likewise)
    if hasattr(L, "fdh_set_damage_readback"):
        L.fdh_set_damage_readback.argtypes = [vp, C.c_int]
        L.fdh_read_damage.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.fdh_read_damage_into.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.fdh_apply_damage.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp, vp, C.c_int]
    # coded damage readback (include/figdraw_hip_stream.h; likewise)
    if hasattr(L, "fdh_read_damage_coded"):
        L.fdh_read_damage_coded.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int)]
        L.fdh_decode_damage.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int64]
        L.fdh_coded_damage_bound.argtypes = [C.c_int, C.c_int]
        L.fdh_coded_damage_bound.restype = C.c_int64
    # exact damage readback (include/figdraw_hip_exact.h; likewise)
    if hasattr(L, "fdh_set_damage_exact"):
        L.fdh_set_damage_exact.argtypes = [vp, C.c_int]
        L.fdh_damage_exact_stats.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    # moved damage readback (include_readback/figdraw_hip_moves.h; likewise)
    if hasattr(L, "fdh_read_damage_moved"):
        L.fdh_read_damage_moved.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.fdh_decode_damage_moved.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int64]
        L.fdh_find_damage_moves.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int)]
    # picking (include/figdraw_hip_pick.h; likewise absent from older libraries)
    if hasattr(L, "fdh_set_pick"):
        L.fdh_set_pick.argtypes = [vp, C.c_int]
        L.fdh_set_pick_tag.argtypes = [vp, C.c_int32, C.c_int32]
        L.fdh_pick_points.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, vp, vp]
        L.fdh_pick_region.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, vp]
        L.fdh_pick_draw_tags.argtypes = [vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    assert L.fdh_sizeof_fig() == C.sizeof(S.CFig), (L.fdh_sizeof_fig(), C.sizeof(S.CFig))
    assert L.fdh_sizeof_glyph() == C.sizeof(S.CGlyph)
    assert L.fdh_sizeof_draw_op() == C.sizeof(S.CDrawOp)
    assert L.fdh_sizeof_text_rect() == C.sizeof(S.CTextRect)
    _lib = L
    return L


def _cols(colors):
    return _COL4(*[S.CColor(*[int(v) for v in c]) for c in colors])


class HipContext:
    """One GPU, one HIP stream, one RGBA8 surface (newContext, glcontext.nim:255-261)."""

    RECORD_ONLY = 1  # FDH_CREATE_RECORD_ONLY
    SYNC_SUBMIT = 2  # FDH_CREATE_SYNC_SUBMIT

    def __init__(self, atlas_size: int = 1024, pixel_scale: float = 1.0, device: int = 0, record_only: bool = False,
                 sync_submit: bool = False):
        """record_only: a call recorder -- the scene front-end and the atlas packer run, nothing is drawn and no GPU is
        needed (the RecordingBackend of the reference's tests/ttransform.nim); see record_begin / record_calls.
        sync_submit: end_frame prepares, uploads and launches on the calling thread instead of the context's submit thread."""
        self.L = load()
        h = C.c_void_p()
        rc = self.L.fdh_create(C.byref(h), atlas_size, pixel_scale, device,
                               (self.RECORD_ONLY if record_only else 0) | (self.SYNC_SUBMIT if sync_submit else 0))
        if rc != 0:
            raise FigdrawHipError(rc, self.L.fdh_last_error().decode())
        self.h = h
        self.W = self.H = 0
        self.device = device

    def _ck(self, rc):
        if rc != 0:
            raise FigdrawHipError(rc, self.L.fdh_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.fdh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- BackendContext surface
    def begin_frame(self, w, h, clear=True, color=(1.0, 1.0, 1.0, 1.0)):
        self.W, self.H = int(w), int(h)
        self._ck(self.L.fdh_begin_frame(self.h, int(w), int(h), int(bool(clear)), _F4(*color)))

    def end_frame(self):
        self._ck(self.L.fdh_end_frame(self.h))

    def save_transform(self):
        self._ck(self.L.fdh_save_transform(self.h))

    def restore_transform(self):
        self._ck(self.L.fdh_restore_transform(self.h))

    def translate(self, x, y):
        self._ck(self.L.fdh_translate(self.h, x, y))

    def rotate(self, a):
        self._ck(self.L.fdh_rotate(self.h, a))

    def scale(self, sx, sy=None):
        self._ck(self.L.fdh_scale(self.h, sx, sx if sy is None else sy))

    def apply_transform(self, m16):
        self._ck(self.L.fdh_apply_transform(self.h, (C.c_float * 16)(*m16)))

    def transform_mirrors_y(self) -> bool:
        out = C.c_int()
        self._ck(self.L.fdh_transform_mirrors_y(self.h, C.byref(out)))
        return bool(out.value)

    def set_aa_factor(self, aa):
        self._ck(self.L.fdh_set_aa_factor(self.h, aa))

    def sdf_aa_factor(self) -> float:
        out = C.c_float()
        self._ck(self.L.fdh_get_aa_factor(self.h, C.byref(out)))
        return out.value

    def draw_rounded_rect_sdf(self, rect, colors, radii_x, radii_y, mode, factor=4.0, spread=0.0, shape=(0.0, 0.0),
                              fill_mode=0, mid=(0, 0, 0, 0), stop=(0, 0, 0, 0), mid_pos=0.5):
        self._ck(self.L.fdh_draw_rounded_rect_sdf(self.h, _F4(*rect), _cols(colors), _F4(*radii_x), _F4(*radii_y), int(mode),
                                                  factor, spread, _F2(*shape), int(fill_mode), S.CColor(*mid),
                                                  S.CColor(*stop), mid_pos))

    def draw_rounded_rect_fill(self, rect, fill: S.Fill, radii_x, radii_y, mode, factor=4.0, spread=0.0, shape=(0.0, 0.0)):
        cf = S.cfill(fill)
        self._ck(self.L.fdh_draw_rounded_rect_fill(self.h, _F4(*rect), C.byref(cf), _F4(*radii_x), _F4(*radii_y), int(mode),
                                                   factor, spread, _F2(*shape)))

    def draw_image(self, key, pos, colors, size=(0.0, 0.0), flip_y=False):
        self._ck(self.L.fdh_draw_image(self.h, int(key), _F2(*pos), _cols(colors), _F2(*size), int(bool(flip_y))))

    def draw_image_adj(self, key, pos, color, size):
        """drawImageAdj (glcontext.nim:1369-1381): the image with its uv rect pulled in by two texels on every side"""
        self._ck(self.L.fdh_draw_image_adj(self.h, int(key), _F2(*pos), S.CColor(*color), _F2(*size)))

    def set_text_lcd_filtering(self, enabled: bool):
        self._ck(self.L.fdh_set_text_lcd_filtering(self.h, int(bool(enabled))))

    def text_lcd_filtering(self) -> bool:
        out = C.c_int()
        self._ck(self.L.fdh_get_text_lcd_filtering(self.h, C.byref(out)))
        return bool(out.value)

    def comm_info(self):
        """(rank, world) of the context's communicator; (0, 1) without one"""
        r, w = C.c_int(), C.c_int()
        self._ck(self.L.fdh_comm_info(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def draw_msdf(self, key, pos, color, size, px_range, sd_threshold=0.5, stroke_weight=0.0, mtsdf=False, flip_y=False):
        self._ck(self.L.fdh_draw_msdf(self.h, int(key), _F2(*pos), S.CColor(*color), _F2(*size), px_range, sd_threshold,
                                      stroke_weight, int(bool(mtsdf)), int(bool(flip_y))))

    def draw_quadratic_bezier_sdf(self, rect, fill, p0, p1, p2, stroke_weight, cap):
        cf = S.cfill(S.fill_from_json(fill))
        self._ck(self.L.fdh_draw_quadratic_bezier_sdf(self.h, _F4(*rect), C.byref(cf), _F2(*p0), _F2(*p1), _F2(*p2),
                                                      stroke_weight, int(cap)))

    def draw_filled_quad(self, verts, colors):
        self._ck(self.L.fdh_draw_filled_quad(self.h, (C.c_float * 8)(*verts), _cols(colors)))

    def draw_rect(self, rect, color):
        self._ck(self.L.fdh_draw_rect(self.h, _F4(*rect), S.CColor(*color)))

    def draw_backdrop_blur(self, rect, radii_x, radii_y, blur_radius):
        self._ck(self.L.fdh_draw_backdrop_blur(self.h, _F4(*rect), _F4(*radii_x), _F4(*radii_y), blur_radius))

    def begin_mask(self, rect, radii_x, radii_y):
        self._ck(self.L.fdh_begin_mask(self.h, _F4(*rect), _F4(*radii_x), _F4(*radii_y)))

    def end_mask(self):
        self._ck(self.L.fdh_end_mask(self.h))

    def pop_mask(self):
        self._ck(self.L.fdh_pop_mask(self.h))

    def begin_rect_mask(self, rect, radii_x, radii_y):
        self._ck(self.L.fdh_begin_rect_mask(self.h, _F4(*rect), _F4(*radii_x), _F4(*radii_y)))

    def pop_rect_mask(self):
        self._ck(self.L.fdh_pop_rect_mask(self.h))

    def set_text_subpixel(self, enabled: bool, shift: float = 0.0, glyph_variants: bool = False):
        self._ck(self.L.fdh_set_text_subpixel_positioning(self.h, int(bool(enabled))))
        self._ck(self.L.fdh_set_text_subpixel_glyph_variants(self.h, int(bool(glyph_variants))))
        self._ck(self.L.fdh_set_text_subpixel_shift(self.h, shift))

    def set_text_subpixel_shift(self, shift: float):
        self._ck(self.L.fdh_set_text_subpixel_shift(self.h, float(shift)))

    # ---- atlas
    def put_image(self, key, rgba: np.ndarray):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_image(self.h, int(key), rgba.shape[1], rgba.shape[0], rgba.ctypes.data, out))
        return tuple(out)

    def put_glyph_outline(self, key, segs: np.ndarray, w: int, h: int, lcd_filter: bool = False, mtsdf: bool = False, sdf_range: int = 0, correct: bool = False, overlap: bool = False):
        """a glyph outline (n x 6: x0, y0, cx, cy, x1, y1; cx = NaN for a line) into the atlas, made on the device: coverage, or with
        mtsdf=True a multi-channel + true signed distance field of `sdf_range` texels (0: 4) for draw_msdf (FDH_GLYPH_MTSDF); correct=True
        adds the correction pass (FDH_GLYPH_MTSDF_CORRECT, with mtsdf only); overlap=True combines contours that overlap as non-zero winding
        fills them (FDH_GLYPH_MTSDF_OVERLAP, with mtsdf only)"""
        segs = np.ascontiguousarray(segs, dtype=np.float32).reshape(-1, 6)
        out = (C.c_int * 4)()
        flags = (1 if lcd_filter else 0) | (4 if mtsdf else 0) | (8 if correct else 0) | (32 if overlap else 0) | (int(sdf_range) << 8)
        self._ck(self.L.fdh_put_glyph_outline(self.h, int(key), int(w), int(h), segs.ctypes.data, len(segs), flags, out))
        return tuple(out)

    def put_glyph_outline_cubic(self, key, segs8: np.ndarray, w: int, h: int, lcd_filter=False, mtsdf: bool = False, sdf_range: int = 0, correct: bool = False):
        """a glyph outline with cubic segments (fdh_put_glyph_outline_cubic, include_glyphs/figdraw_hip_cubic.h): n x 8 floats x0, y0, c1x, c1y,
        c2x, c2y, x1, y1; c2x = NaN: a quadratic with control point (c1x, c1y); c1x = NaN: a line.  lcd_filter as in put_glyph_image (True,
        False or "context"); mtsdf, sdf_range and correct as in put_glyph_outline.  -> the rectangle (x, y, w, h)"""
        segs = np.ascontiguousarray(segs8, dtype=np.float32).reshape(-1, 8)
        out = (C.c_int * 4)()
        flags = (2 if lcd_filter == "context" else (1 if lcd_filter else 0)) | (4 if mtsdf else 0) | (8 if correct else 0) | (int(sdf_range) << 8)
        self._ck(self.L.fdh_put_glyph_outline_cubic(self.h, int(key), int(w), int(h), segs.ctypes.data if len(segs) else None, len(segs), flags, out))
        return tuple(out)

    def _glyph_outline_array(self, items, floats: int):
        """what the four batch calls take: items (key, segs, w, h[, range]), segs n x `floats` -> (n, the FdhGlyphOutline array, the rectangles to fill,
        the outlines, which must stay alive until the call returns)"""
        items = list(items)
        n = len(items)
        arr = (GlyphOutline * max(n, 1))()
        keep = []
        for g, it in zip(arr, items):
            segs = np.ascontiguousarray(it[1], dtype=np.float32).reshape(-1, floats)
            keep.append(segs)
            g.key, g.segs, g.n_segs, g.width, g.height = int(it[0]), segs.ctypes.data if len(segs) else None, len(segs), int(it[2]), int(it[3])
            g.sdf_range = int(it[4]) if len(it) > 4 else 0
        return n, arr, ((C.c_int * 4) * max(n, 1))(), keep

    def put_glyph_outlines(self, items, sdf_range: int = 0, correct: bool = False, overlap: bool = False):
        """a batch of distance-field glyphs in one call (fdh_put_glyph_outlines, include_glyphs/figdraw_hip_glyphs.h): `items` is a sequence of
        (key, segs, w, h) or (key, segs, w, h, range) -- a glyph's own range, 0 or absent: `sdf_range` (whose 0 is 4); correct and overlap as
        in put_glyph_outline, for every glyph.  What the same put_glyph_outline(..., mtsdf=True) calls in order would leave, from a number of
        launches that does not depend on len(items).  -> the rectangles, one (x, y, w, h) per item"""
        n, arr, out, keep = self._glyph_outline_array(items, 6)
        flags = 4 | (8 if correct else 0) | (32 if overlap else 0) | (int(sdf_range) << 8)
        self._ck(self.L.fdh_put_glyph_outlines(self.h, C.addressof(arr), n, flags, C.addressof(out)))
        return [tuple(out[i]) for i in range(n)]

    def put_glyph_outlines_cubic(self, items, sdf_range: int = 0, correct: bool = False, overlap: bool = False):
        """put_glyph_outlines for outlines with cubic segments (fdh_put_glyph_outlines_cubic, include_glyphs/figdraw_hip_cubic_batch.h): `items` as
        there, each `segs` n x 8 in the format of put_glyph_outline_cubic.  What the same put_glyph_outline_cubic(..., mtsdf=True) calls in order
        would leave; overlap only where no glyph holds a cubic.  -> the rectangles, one (x, y, w, h) per item"""
        n, arr, out, keep = self._glyph_outline_array(items, 8)
        flags = 4 | (8 if correct else 0) | (32 if overlap else 0) | (int(sdf_range) << 8)
        self._ck(self.L.fdh_put_glyph_outlines_cubic(self.h, C.addressof(arr), n, flags, C.addressof(out)))
        return [tuple(out[i]) for i in range(n)]

    def put_glyph_coverage_batch_cubic(self, items, lcd_filter=False):
        """put_glyph_coverage_batch for outlines with cubic segments (fdh_put_glyph_coverage_batch_cubic, include_glyphs/figdraw_hip_cubic_batch.h):
        `items` is a sequence of (key, segs, w, h), each `segs` n x 8; lcd_filter as in put_glyph_image, for every glyph.  What the same
        put_glyph_outline_cubic calls in order would leave.  -> the rectangles, one (x, y, w, h) per item"""
        n, arr, out, keep = self._glyph_outline_array([it[:4] for it in items], 8)
        flags = 2 if lcd_filter == "context" else (1 if lcd_filter else 0)
        self._ck(self.L.fdh_put_glyph_coverage_batch_cubic(self.h, C.addressof(arr), n, flags, C.addressof(out)))
        return [tuple(out[i]) for i in range(n)]

    def glyph_batch_stats(self) -> dict:
        """what the last put_glyph_outlines or put_glyph_outlines_cubic did: glyphs, written, dropped_by_growth, tiles, edges, launches, bytes_copied"""
        st = GlyphBatchStats()
        self._ck(self.L.fdh_glyph_batch_stats(self.h, C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in GlyphBatchStats._fields_}

    def put_glyph_coverage_batch(self, items, lcd_filter=False):
        """a batch of coverage glyphs in one call (fdh_put_glyph_coverage_batch, include_glyphs/figdraw_hip_coverage.h): `items` is a sequence of
        (key, segs, w, h); lcd_filter as in put_glyph_image (True, False or "context"), for every glyph.  What the same put_glyph_outline
        calls in order would leave, from a number of launches that does not depend on len(items).  -> the rectangles, one (x, y, w, h) per item"""
        n, arr, out, keep = self._glyph_outline_array([it[:4] for it in items], 6)
        flags = 2 if lcd_filter == "context" else (1 if lcd_filter else 0)
        self._ck(self.L.fdh_put_glyph_coverage_batch(self.h, C.addressof(arr), n, flags, C.addressof(out)))
        return [tuple(out[i]) for i in range(n)]

    def glyph_coverage_batch_stats(self) -> dict:
        """what the last put_glyph_coverage_batch or put_glyph_coverage_batch_cubic did: glyphs, written, dropped_by_growth, tiles, edges (flattened lines), launches, bytes_copied"""
        st = GlyphBatchStats()
        self._ck(self.L.fdh_glyph_coverage_batch_stats(self.h, C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in GlyphBatchStats._fields_}

    def put_glyph_image(self, key, rgba: np.ndarray, lcd_filter=False):
        """a rasterised glyph, processed on the device on its way into the atlas (LCD filter, mip chain): pixie_raster.nim:12-95"""
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        out = (C.c_int * 4)()
        flag = 2 if lcd_filter == "context" else (1 if lcd_filter else 0)  # "context": follow set_text_lcd_filtering (FDH_GLYPH_LCD_CONTEXT)
        self._ck(self.L.fdh_put_glyph_image(self.h, int(key), rgba.shape[1], rgba.shape[0], rgba.ctypes.data, flag, out))
        return tuple(out)

    def put_image_sdf(self, key, rgba: np.ndarray, channel: int = 3, pad: int = 0, sdf_range: int = 0):
        """the distance field of a coverage image (fdh_put_image_sdf, include_glyphs/figdraw_hip_image_sdf.h): byte `channel` of the h x w x 4
        texels is the coverage; the field has `pad` texels more on every side and the range sdf_range (0: 4) and draws through draw_msdf.
        -> the rectangle (x, y, w + 2 pad, h + 2 pad)"""
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_image_sdf(self.h, int(key), rgba.shape[1], rgba.shape[0], rgba.ctypes.data, int(channel), int(pad), int(sdf_range) << 8, out))
        return tuple(out)

    def put_image_sdf_of(self, src_key, key, channel: int = 3, pad: int = 0, sdf_range: int = 0):
        """put_image_sdf of the texels that src_key holds in the atlas (fdh_put_image_sdf_of): nothing crosses the bus.  -> the rectangle"""
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_image_sdf_of(self.h, int(src_key), int(key), int(channel), int(pad), int(sdf_range) << 8, out))
        return tuple(out)

    def put_image_device(self, key, ptr, width, height, pitch_bytes, format=IMAGE_RGBA8, channels=4, plane_bytes=0, straight_alpha=False):
        """an image from device (or page-locked host) memory at address `ptr` (fdh_put_image_device, include_glyphs/figdraw_hip_device_image.h):
        what put_image stores of the converted texels, made on the device.  Whatever wrote the source has finished, or is ordered on the
        context's stream (set_stream).  -> the rectangle"""
        img = DeviceImage(ptr, int(width), int(height), int(pitch_bytes), int(plane_bytes), int(format), int(channels), IMAGE_STRAIGHT_ALPHA if straight_alpha else 0, 0)
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_image_device(self.h, int(key), C.byref(img), out))
        return tuple(out)

    def update_image_device(self, key, ptr, width, height, pitch_bytes, format=IMAGE_RGBA8, channels=4, plane_bytes=0, straight_alpha=False):
        """new texels from device memory for an entry of the same size (fdh_update_image_device)"""
        img = DeviceImage(ptr, int(width), int(height), int(pitch_bytes), int(plane_bytes), int(format), int(channels), IMAGE_STRAIGHT_ALPHA if straight_alpha else 0, 0)
        self._ck(self.L.fdh_update_image_device(self.h, int(key), C.byref(img)))

    def put_video_frame(self, key, y_ptr, uv_ptr, width, height, pitch_y, pitch_uv, format=VIDEO_NV12, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0):
        """a decoded frame from device (or page-locked host) memory (fdh_put_video_frame, include_glyphs/figdraw_hip_video_frame.h): NV12 or
        P010 planes at `y_ptr` and `uv_ptr`, or BGRA8 texels at `y_ptr` (uv_ptr = 0, pitch_uv = 0, matrix = range = 0); what put_image stores
        of the converted texels, made on the device.  -> the rectangle"""
        f = video_frame(y_ptr, uv_ptr, width, height, pitch_y, pitch_uv, format, matrix, range, flags)
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_video_frame(self.h, int(key), C.byref(f), out))
        return tuple(out)

    def update_video_frame(self, key, y_ptr, uv_ptr, width, height, pitch_y, pitch_uv, format=VIDEO_NV12, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0):
        """the next frame for an entry of the same size (fdh_update_video_frame)"""
        f = video_frame(y_ptr, uv_ptr, width, height, pitch_y, pitch_uv, format, matrix, range, flags)
        self._ck(self.L.fdh_update_video_frame(self.h, int(key), C.byref(f)))

    def read_video_frame(self, y_ptr, uv_ptr, pitch_y, pitch_uv, format=VIDEO_NV12, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0, rect=None):
        """the last frame, or its rectangle `rect` = (x, y, w, h), out as NV12 or P010 planes at `y_ptr` and `uv_ptr`, or as BGRA8 texels at
        `y_ptr` (uv_ptr = 0, pitch_uv = 0, matrix = range = 0), in device or page-locked host memory (fdh_read_video_frame,
        include_video/figdraw_hip_video_out.h).  The planes are complete on return."""
        t = video_target(y_ptr, uv_ptr, pitch_y, pitch_uv, format, matrix, range, flags, rect)
        self._ck(self.L.fdh_read_video_frame(self.h, C.byref(t)))

    def put_video_planes(self, key, ptrs, width, height, pitches, format=VIDEO_I420, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0):
        """a three-plane frame from device (or page-locked host) memory (fdh_put_video_planes, include_video/figdraw_hip_video_planar.h):
        I420, I010, I444 or I410; `ptrs` and `pitches` of Y, Cb, Cr (YV12: the chroma pointers swapped); what put_image stores of the
        converted texels, made on the device.  -> the rectangle"""
        f = video_planes(ptrs, width, height, pitches, format, matrix, range, flags)
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_video_planes(self.h, int(key), C.byref(f), out))
        return tuple(out)

    def update_video_planes(self, key, ptrs, width, height, pitches, format=VIDEO_I420, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0):
        """the next frame for an entry of the same size (fdh_update_video_planes)"""
        f = video_planes(ptrs, width, height, pitches, format, matrix, range, flags)
        self._ck(self.L.fdh_update_video_planes(self.h, int(key), C.byref(f)))

    def read_video_planes(self, ptrs, pitches, format=VIDEO_I420, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0, rect=None):
        """the last frame, or its rectangle `rect` = (x, y, w, h), out as the three planes Y, Cb, Cr of I420, I010, I444 or I410 at `ptrs`,
        in device or page-locked host memory (fdh_read_video_planes, include_video/figdraw_hip_video_planar.h).  The planes are complete
        on return."""
        t = video_planes_target(ptrs, pitches, format, matrix, range, flags, rect)
        self._ck(self.L.fdh_read_video_planes(self.h, C.byref(t)))

    def put_video_422(self, key, ptrs, width, height, pitches, format=VIDEO_I422, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0):
        """a 4:2:2 frame from device (or page-locked host) memory (fdh_put_video_422, include_video/figdraw_hip_video_422.h): I422 or I210
        with `ptrs` and `pitches` of Y, Cb, Cr, or YUY2 or UYVY with (ptr, 0, 0) and (pitch, 0, 0); what put_image stores of the converted
        texels, made on the device.  -> the rectangle"""
        f = video_planes(ptrs, width, height, pitches, format, matrix, range, flags)
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_video_422(self.h, int(key), C.byref(f), out))
        return tuple(out)

    def update_video_422(self, key, ptrs, width, height, pitches, format=VIDEO_I422, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0):
        """the next frame for an entry of the same size (fdh_update_video_422)"""
        f = video_planes(ptrs, width, height, pitches, format, matrix, range, flags)
        self._ck(self.L.fdh_update_video_422(self.h, int(key), C.byref(f)))

    def read_video_422(self, ptrs, pitches, format=VIDEO_I422, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0, rect=None):
        """the last frame, or its rectangle `rect` = (x, y, w, h), out as I422 or I210 (the three planes Y, Cb, Cr at `ptrs`) or as YUY2 or
        UYVY (one plane: (ptr, 0, 0) and (pitch, 0, 0)), in device or page-locked host memory (fdh_read_video_422,
        include_video/figdraw_hip_video_422.h).  The planes are complete on return."""
        t = video_planes_target(ptrs, pitches, format, matrix, range, flags, rect)
        self._ck(self.L.fdh_read_video_422(self.h, C.byref(t)))

    def put_video_alpha(self, key, ptrs, width, height, pitches, format=VIDEO_A420, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0):
        """a frame with an alpha plane from device (or page-locked host) memory (fdh_put_video_alpha, include_video/figdraw_hip_video_alpha.h):
        A420, A444 or A410 with `ptrs` and `pitches` of Y, Cb, Cr, A, or UYVA with (ptr, 0, 0, alpha ptr) and (pitch, 0, 0, alpha pitch);
        flags: VIDEO_CHROMA_LINEAR, VIDEO_STRAIGHT_ALPHA; what put_image stores of the converted texels, made on the device.  -> the rectangle"""
        f = video_alpha_planes(ptrs, width, height, pitches, format, matrix, range, flags)
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_video_alpha(self.h, int(key), C.byref(f), out))
        return tuple(out)

    def update_video_alpha(self, key, ptrs, width, height, pitches, format=VIDEO_A420, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0):
        """the next frame for an entry of the same size (fdh_update_video_alpha)"""
        f = video_alpha_planes(ptrs, width, height, pitches, format, matrix, range, flags)
        self._ck(self.L.fdh_update_video_alpha(self.h, int(key), C.byref(f)))

    def read_video_alpha(self, ptrs, pitches, format=VIDEO_A420, matrix=VIDEO_BT709, range=VIDEO_LIMITED, flags=0, rect=None):
        """the last frame, or its rectangle `rect` = (x, y, w, h), out as A420, A444 or A410 (the four planes Y, Cb, Cr, A at `ptrs`) or as
        UYVA ((ptr, 0, 0, alpha ptr) and (pitch, 0, 0, alpha pitch)), in device or page-locked host memory; with VIDEO_STRAIGHT_ALPHA the colour
        is un-premultiplied first (fdh_read_video_alpha, include_video/figdraw_hip_video_alpha.h).  The planes are complete on return."""
        t = video_alpha_planes_target(ptrs, pitches, format, matrix, range, flags, rect)
        self._ck(self.L.fdh_read_video_alpha(self.h, C.byref(t)))

    @staticmethod
    def _video_frame_arrays(items):
        """items: (key, VideoFrame), or (key, y_ptr, uv_ptr, width, height, pitch_y, pitch_uv[, format, matrix, range, flags]) as
        put_video_frame takes them -> (n, the keys, the FdhVideoFrame array)"""
        items = list(items)
        n = len(items)
        keys, arr = (C.c_int64 * max(n, 1))(), (VideoFrame * max(n, 1))()
        for i, it in enumerate(items):
            keys[i] = int(it[0])
            f = it[1] if isinstance(it[1], VideoFrame) else video_frame(*it[1:7], *(tuple(it[7:]) + (VIDEO_NV12, VIDEO_BT709, VIDEO_LIMITED, 0)[len(it) - 7:])[:4])
            C.memmove(C.byref(arr, i * C.sizeof(VideoFrame)), C.byref(f), C.sizeof(VideoFrame))
        return n, keys, arr

    def put_video_frames(self, items):
        """a batch of decoded frames from device (or page-locked host) memory in one call (fdh_put_video_frames, include_glyphs/
        figdraw_hip_video_frames.h): `items` is a sequence of (key, VideoFrame) or of (key, y_ptr, uv_ptr, width, height, pitch_y, pitch_uv[,
        format, matrix, range, flags]).  What the same put_video_frame calls in order would leave, from at most six launches and one wait.
        -> the rectangles, one (x, y, w, h) per item"""
        n, keys, arr = self._video_frame_arrays(items)
        out = ((C.c_int * 4) * max(n, 1))()
        self._ck(self.L.fdh_put_video_frames(self.h, C.addressof(keys), C.addressof(arr), n, C.addressof(out)))
        return [tuple(out[i]) for i in range(n)]

    def update_video_frames(self, items):
        """the next frames for a batch of entries of the same sizes (fdh_update_video_frames); `items` as in put_video_frames"""
        n, keys, arr = self._video_frame_arrays(items)
        self._ck(self.L.fdh_update_video_frames(self.h, C.addressof(keys), C.addressof(arr), n))

    def video_batch_stats(self) -> dict:
        """what the last put_video_frames or update_video_frames that passed validation did: frames, written, dropped_by_growth, tiles,
        launches, bytes_copied"""
        st = VideoBatchStats()
        self._ck(self.L.fdh_video_batch_stats(self.h, C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in VideoBatchStats._fields_ if name != "reserved"}

    @staticmethod
    def _device_image_arrays(items):
        """items: (key, DeviceImage), or (key, ptr, width, height, pitch_bytes[, format, channels, plane_bytes, straight_alpha]) as
        put_image_device takes them -> (n, the keys, the FdhDeviceImage array)"""
        items = list(items)
        n = len(items)
        keys, arr = (C.c_int64 * max(n, 1))(), (DeviceImage * max(n, 1))()
        for i, it in enumerate(items):
            keys[i] = int(it[0])
            if isinstance(it[1], DeviceImage):
                C.memmove(C.byref(arr, i * C.sizeof(DeviceImage)), C.byref(it[1]), C.sizeof(DeviceImage))
                continue
            ptr, width, height, pitch = it[1:5]
            fmt, channels, plane, straight = (tuple(it[5:]) + (IMAGE_RGBA8, 4, 0, False)[len(it) - 5:])[:4]
            arr[i] = DeviceImage(ptr, int(width), int(height), int(pitch), int(plane), int(fmt), int(channels), IMAGE_STRAIGHT_ALPHA if straight else 0, 0)
        return n, keys, arr

    def put_images_device(self, items):
        """a batch of images from device (or page-locked host) memory in one call (fdh_put_images_device, include_glyphs/
        figdraw_hip_device_images.h): `items` is a sequence of (key, DeviceImage) or of (key, ptr, width, height, pitch_bytes[, format, channels,
        plane_bytes, straight_alpha]).  What the same put_image_device calls in order would leave, from at most four launches and one wait.
        -> the rectangles, one (x, y, w, h) per item"""
        n, keys, arr = self._device_image_arrays(items)
        out = ((C.c_int * 4) * max(n, 1))()
        self._ck(self.L.fdh_put_images_device(self.h, C.addressof(keys), C.addressof(arr), n, C.addressof(out)))
        return [tuple(out[i]) for i in range(n)]

    def update_images_device(self, items):
        """new texels for a batch of entries of the same sizes (fdh_update_images_device); `items` as in put_images_device"""
        n, keys, arr = self._device_image_arrays(items)
        self._ck(self.L.fdh_update_images_device(self.h, C.addressof(keys), C.addressof(arr), n))

    def image_batch_stats(self) -> dict:
        """what the last put_images_device or update_images_device that passed validation did: images, written, dropped_by_growth, tiles,
        launches, bytes_copied"""
        st = ImageBatchStats()
        self._ck(self.L.fdh_image_batch_stats(self.h, C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in ImageBatchStats._fields_ if name != "reserved"}

    def put_image_tensors(self, keys, tensors, straight_alpha=False):
        """put_images_device of tensors (tensor_images: a sequence of what put_image_tensor takes, or one N x C x H x W / N x H x W x 4 tensor
        cut along its first axis without a copy).  -> the rectangles"""
        images = tensor_images(tensors, straight_alpha)
        keys = list(keys)
        if len(keys) != len(images):
            raise ValueError(f"{len(keys)} keys for {len(images)} images")
        return self.put_images_device(zip(keys, images))

    def update_image_tensors(self, keys, tensors, straight_alpha=False):
        """update_images_device of tensors, as put_image_tensors takes them"""
        images = tensor_images(tensors, straight_alpha)
        keys = list(keys)
        if len(keys) != len(images):
            raise ValueError(f"{len(keys)} keys for {len(images)} images")
        self.update_images_device(zip(keys, images))

    def put_image_tensor(self, key, tensor, straight_alpha=False):
        """put_image_device of a tensor (tensor_image: H x W x 4 uint8, or C x H x W / H x W float32 or float16).  -> the rectangle"""
        img = tensor_image(tensor, straight_alpha)
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_image_device(self.h, int(key), C.byref(img), out))
        return tuple(out)

    def update_image_tensor(self, key, tensor, straight_alpha=False):
        img = tensor_image(tensor, straight_alpha)
        self._ck(self.L.fdh_update_image_device(self.h, int(key), C.byref(img)))

    def put_image_mips(self, key, mips):
        """Upload an explicit mip chain (premultiplied RGBA8 arrays, level 0 first), as putFlippy does."""
        mips = [np.ascontiguousarray(m, dtype=np.uint8) for m in mips]
        n = len(mips)
        ws = (C.c_int * n)(*[m.shape[1] for m in mips])
        hs = (C.c_int * n)(*[m.shape[0] for m in mips])
        ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in mips])
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_image_mips(self.h, int(key), n, ws, hs, ptrs, out))
        return tuple(out)

    def put_flippy(self, key, file_bytes: bytes):
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_put_flippy(self.h, int(key), file_bytes, len(file_bytes), out))
        return tuple(out)

    def update_image(self, key, rgba: np.ndarray):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        self._ck(self.L.fdh_update_image(self.h, int(key), rgba.shape[1], rgba.shape[0], rgba.ctypes.data))

    def has_image(self, key) -> bool:
        out = C.c_int()
        self._ck(self.L.fdh_has_image(self.h, int(key), C.byref(out)))
        return bool(out.value)

    def remove_image(self, key):
        self._ck(self.L.fdh_remove_image(self.h, int(key)))

    def compact_atlas(self, size: int = 0) -> dict:
        """repack the live entries into a fresh atlas of `size` (0: the current size), every entry kept (fdh_compact_atlas,
        include_glyphs/figdraw_hip_atlas.h); rectangles of earlier puts are stale afterwards: image_rect.  -> the move's statistics"""
        st = AtlasMoveStats()
        self._ck(self.L.fdh_compact_atlas(self.h, int(size), C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in AtlasMoveStats._fields_}

    def set_atlas_keep(self, on: bool = True):
        """keep mode: a put that does not fit compacts or grows the atlas with every entry kept instead of emptying it (fdh_set_atlas_keep)"""
        self._ck(self.L.fdh_set_atlas_keep(self.h, 1 if on else 0))

    def atlas_keep(self) -> bool:
        out = C.c_int()
        self._ck(self.L.fdh_get_atlas_keep(self.h, C.byref(out)))
        return bool(out.value)

    def image_rect(self, key):
        """where an entry is now: (x, y, w, h)"""
        out = (C.c_int * 4)()
        self._ck(self.L.fdh_image_rect(self.h, int(key), out))
        return tuple(out)

    def atlas_usage(self) -> dict:
        """size, entries, used_area, packed_area, epoch, rebuilds, compactions (fdh_atlas_usage)"""
        u = AtlasUsage()
        self._ck(self.L.fdh_atlas_usage(self.h, C.byref(u)))
        return {name: int(getattr(u, name)) for name, _ in AtlasUsage._fields_}

    def read_atlas_level(self, level: int) -> np.ndarray:
        """one whole level of the atlas, (size >> level)^2 x 4 bytes (fdh_debug_read_atlas_level)"""
        ls = self.atlas_size() >> level
        out = np.zeros((max(ls, 1), max(ls, 1), 4), dtype=np.uint8)
        self._ck(self.L.fdh_debug_read_atlas_level(self.h, int(level), out.ctypes.data, out.nbytes))
        return out

    def reset_atlas(self, minimum_size=0):
        self._ck(self.L.fdh_reset_atlas(self.h, int(minimum_size)))

    def atlas_size(self) -> int:
        out = C.c_int()
        self._ck(self.L.fdh_atlas_size(self.h, C.byref(out)))
        return out.value

    # ---- readback
    def read_pixels(self, x=0, y=0, w=0, h=0) -> np.ndarray:
        if w <= 0 or h <= 0:
            x, y, w, h = 0, 0, self.W, self.H
        out = np.zeros((h, w, 4), dtype=np.uint8)
        self._ck(self.L.fdh_read_pixels(self.h, x, y, w, h, out.ctypes.data))
        return out

    def record_begin(self):
        """start recording the backend-level calls this context receives (tests/ttransform.nim's RecordingBackend)"""
        self._ck(self.L.fdh_record_begin(self.h))

    def record_calls(self):
        import json

        return json.loads(self.L.fdh_record_json(self.h).decode())

    def debug_read_surface(self, which: int) -> np.ndarray:
        """0: frame, 1: horizontal blur pass output, 2: blurred snapshot, 4: level 0 of the atlas, atlas_size x atlas_size (diagnostic)"""
        if which == 4:
            s = self.atlas_size()
            out = np.zeros((s, s, 4), dtype=np.uint8)
        else:
            out = np.zeros((self.H, self.W, 4), dtype=np.uint8)
        self._ck(self.L.fdh_debug_read_surface(self.h, which, out.ctypes.data))
        return out

    def frame_device_ptr(self):
        p, w, h, pitch = C.c_void_p(), C.c_int(), C.c_int(), C.c_int64()
        self._ck(self.L.fdh_frame_device_ptr(self.h, C.byref(p), C.byref(w), C.byref(h), C.byref(pitch)))
        return p.value, w.value, h.value, pitch.value

    def sync(self):
        self._ck(self.L.fdh_sync(self.h))

    def flush(self):
        """every submitted frame is enqueued on the stream (no wait for the GPU)"""
        self._ck(self.L.fdh_flush(self.h))

    def set_stream(self, stream_ptr: Optional[int]):
        self._ck(self.L.fdh_set_stream(self.h, C.c_void_p(stream_ptr or 0)))

    # ---- whole scenes
    def render_frame(self, renders: S.Renders, w, h, clear=True, color=(1.0, 1.0, 1.0, 1.0), ui_scale=1.0):
        cs = renders.to_c()
        self._ck(self.L.fdh_set_ui_scale(self.h, ui_scale))
        self.W, self.H = int(w * ui_scale), int(h * ui_scale)
        self._ck(self.L.fdh_render_frame(self.h, cs.byref(), float(w), float(h), int(bool(clear)), _F4(*color)))

    # ---- retained scenes (renderfragments.nim:426-544: the tree lives in the context, edits re-decompose only what they touch)
    @staticmethod
    def _marshal_nodes(figs):
        """a node list -> (CScene keeping the arrays alive, pointer to its FdhFig array, count, pointer to the side-array scene)"""
        tmp = S.Renders()
        lst = S.RenderList()
        lst.nodes = list(figs)
        tmp.setLayer(0, lst)
        cs = tmp.to_c()
        return cs, C.cast(cs.struct.layers[0].nodes, C.c_void_p), len(lst.nodes), cs.byref()

    def scene_retain(self, renders: S.Renders, w, h, clear=True, color=(1.0, 1.0, 1.0, 1.0), ui_scale=1.0):
        cs = renders.to_c()
        self._ck(self.L.fdh_set_ui_scale(self.h, ui_scale))
        self.W, self.H = int(w * ui_scale), int(h * ui_scale)
        self._ck(self.L.fdh_scene_retain(self.h, cs.byref(), float(w), float(h), int(bool(clear)), _F4(*color)))

    def scene_update_nodes(self, layer: int, first: int, figs):
        """overwrite nodes [first, first + len(figs)) of layer number `layer` (same tree shape, new properties)"""
        cs, ptr, n, side = self._marshal_nodes(figs)
        self._ck(self.L.fdh_scene_update_nodes(self.h, int(layer), int(first), n, ptr, side))

    def scene_replace_root(self, layer: int, slot: int, figs):
        """replace the subtree under root slot `slot`; figs[0] is the new root (parent -1), later parents are relative to figs;
        an empty list removes the root"""
        cs, ptr, n, side = self._marshal_nodes(figs)
        self._ck(self.L.fdh_scene_replace_root(self.h, int(layer), int(slot), ptr if n else None, n, side))

    def scene_insert_root(self, layer: int, slot: int, figs):
        cs, ptr, n, side = self._marshal_nodes(figs)
        self._ck(self.L.fdh_scene_insert_root(self.h, int(layer), int(slot), ptr if n else None, n, side))

    def scene_render(self):
        self._ck(self.L.fdh_scene_render(self.h))

    def scene_stats(self):
        a, b = C.c_int64(), C.c_int64()
        self._ck(self.L.fdh_scene_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_upload_bytes(self) -> int:
        out = C.c_int64()
        self._ck(self.L.fdh_last_upload_bytes(self.h, C.byref(out)))
        return out.value

    def verify_upload(self):
        """fault hunting: the device's copy of the last frame's records against the host lanes (fdh_debug_verify_upload)"""
        out = (C.c_uint32 * 24)()
        self._ck(self.L.fdh_debug_verify_upload(self.h, out))
        return list(out)

    def bin_digest(self):
        """fault hunting: hash / totals of the bin kernel's output for the last frame (fdh_debug_bin_digest)"""
        out = (C.c_uint64 * 8)()
        self._ck(self.L.fdh_debug_bin_digest(self.h, out))
        return list(out)[:5]

    def record_digest(self) -> int:
        out = C.c_uint64()
        self._ck(self.L.fdh_debug_record_digest(self.h, C.byref(out)))
        return out.value

    def replay_calls(self, calls):
        """Replay a recorded BackendContext call stream (same format as the test harnesses use)."""
        for call in calls:
            name, args = call[0], call[1:]
            if name == "begin_frame":
                self.begin_frame(self.W, self.H, *args)
            else:
                getattr(self, name)(*args)

    # ---- multi-GPU / measurement
    def set_stripe(self, y0: int, y1: int):
        self._ck(self.L.fdh_set_stripe(self.h, int(y0), int(y1)))

    def set_cull(self, mode: int):
        """0: record every draw; 1 (default): drop draws / clipped subtrees no produced pixel lies under, except while the call
        recorder runs; 2: also then.  Same pixels either way."""
        self._ck(self.L.fdh_set_cull(self.h, int(mode)))

    def set_walk_threads(self, n: int):
        """pool threads the scene front-end decomposes large sibling groups on, beside the calling thread (0: serial; < 0: default)"""
        self._ck(self.L.fdh_set_walk_threads(self.h, int(n)))

    def host_times(self):
        """ns the calling thread spent in the last frame: begin_frame, upload wait, walk, end, prepare, publish, drain, groups, pool, merge"""
        out = (C.c_int64 * 12)()
        self._ck(self.L.fdh_debug_host_times(self.h, out))
        names = ["begin_frame", "wait_upload", "walk", "end", "prepare", "publish", "drain", "groups", "pool_run", "merge"]
        return {k: out[i] for i, k in enumerate(names)}

    def walk_stats(self):
        """(threads in force, sibling groups of the last frame that went to the pool)"""
        t, g = C.c_int(), C.c_int64()
        self._ck(self.L.fdh_walk_stats(self.h, C.byref(t), C.byref(g)))
        return t.value, g.value

    def culled_draws(self) -> int:
        out = C.c_int64()
        self._ck(self.L.fdh_culled_draws(self.h, C.byref(out)))
        return out.value

    def set_blur_route(self, route: int):
        """blur routes: 1 the one-kernel routes (k_blur_fx / k_blur_small), 0 two passes per node, -1 the library's default = the one-kernel routes (same pixels either way)"""
        self._ck(self.L.fdh_set_blur_route(self.h, int(route)))

    # ---- damage tracking (include/figdraw_hip_damage.h)
    def set_damage_tracking(self, on: bool):
        """composite only the 64x64 bins whose inputs changed since this context's previous frame (the rest of the surface keeps its
        bytes); the surface is bit for bit what a full render of the last frame gives.  Refused on record-only contexts and under
        set_stripe."""
        self._ck(self.L.fdh_set_damage_tracking(self.h, 1 if on else 0))

    def _bins(self, fn) -> np.ndarray:
        bx, by, n = C.c_int(), C.c_int(), C.c_int()
        self._ck(fn(self.h, None, 0, C.byref(bx), C.byref(by), C.byref(n)))
        m = np.zeros((by.value, bx.value), dtype=np.uint8)
        self._ck(fn(self.h, m.ctypes.data, m.size, C.byref(bx), C.byref(by), C.byref(n)))
        return m.astype(bool)

    def damage_bins(self) -> np.ndarray:
        """which bins the last submitted frame composited: bool array (bins_y, bins_x); every bin for a frame rendered in full"""
        return self._bins(self.L.fdh_damage_bins)

    def damage_changed_bins(self) -> np.ndarray:
        """the bins whose signature changed, before the blur rule (diagnostic)"""
        return self._bins(self.L.fdh_damage_changed_bins)

    @staticmethod
    def damage_closure(changed, nodes=()) -> np.ndarray:
        """the blur rule on the host: changed = bool array (bins_y, bins_x), nodes = [((x0, y0, x1, y1), radius), ...] (footprints in
        pixels, exclusive ends; radius as given to draw_backdrop_blur) -> the closed damage, bool array of the same shape"""
        L = load()
        ch = np.ascontiguousarray(np.asarray(changed, dtype=bool).astype(np.uint8))
        by, bx = ch.shape
        rects = np.ascontiguousarray(np.array([r for r, _ in nodes], dtype=np.int32).reshape(-1, 4))
        radii = np.ascontiguousarray(np.array([rad for _, rad in nodes], dtype=np.float32))
        out = np.zeros_like(ch)
        rc = L.fdh_damage_closure(ch.ctypes.data, bx, by, rects.ctypes.data if len(nodes) else None, radii.ctypes.data if len(nodes) else None,
                                  len(nodes), out.ctypes.data)
        if rc != 0:
            raise FigdrawHipError(rc, L.fdh_last_error().decode())
        return out.astype(bool)

    # ---- damage readback (include/figdraw_hip_readback.h)
    TILE_PX, TILE_PITCH, TILE_BYTES = 64, 256, 16384  # FDH_TILE_*

    def set_damage_readback(self, on: bool):
        """keep the set of bins composited since the last read_damage / read_damage_into, so that a read moves only those to the host.
        Turning it on makes every bin pending.  Refused on record-only contexts and under set_stripe."""
        self._ck(self.L.fdh_set_damage_readback(self.h, 1 if on else 0))

    def read_damage(self):
        """the pending bins of the last frame -> (tiles int32 (n, 4): x, y, w, h in row-major bin order; pixels uint8 (n, 64, 64, 4):
        tile i's w x h pixels at [i, :h, :w], zeros beyond; full: every bin of the grid is among them).  The arrays are copies: the
        library's buffer is reused by the next read.  Empties the pending set."""
        t, p = C.c_void_p(), C.c_void_p()
        n, full = C.c_int(), C.c_int()
        self._ck(self.L.fdh_read_damage(self.h, C.byref(t), C.byref(p), C.byref(n), None, None, C.byref(full)))
        k = n.value
        if k == 0:
            return np.zeros((0, 4), np.int32), np.zeros((0, self.TILE_PX, self.TILE_PX, 4), np.uint8), bool(full.value)
        tiles = np.ctypeslib.as_array(C.cast(t, C.POINTER(C.c_int32)), shape=(k, 4)).copy()
        pixels = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(k, self.TILE_PX, self.TILE_PX, 4)).copy()
        return tiles, pixels, bool(full.value)

    def read_damage_into(self, image: np.ndarray) -> int:
        """read_damage applied to `image`, the application's mirror of the frame: uint8 (H, W, 4), rows contiguous (any row stride).
        Returns the number of tiles copied.  An image of another size than the last frame is refused and nothing is consumed."""
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 4 or image.strides[2] != 1 or image.strides[1] != 4:
            raise ValueError("read_damage_into: the image must be uint8 (H, W, 4) with contiguous rows")
        if not image.flags.writeable:
            raise ValueError("read_damage_into: the image is read-only")
        n = C.c_int()
        self._ck(self.L.fdh_read_damage_into(self.h, image.ctypes.data, image.strides[0], image.shape[1], image.shape[0], C.byref(n)))
        return n.value

    @staticmethod
    def apply_damage(image: np.ndarray, tiles, pixels) -> None:
        """host only (no context, no GPU): copy the tiles read_damage returned into `image`, uint8 (H, W, 4) with contiguous rows"""
        L = load()
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 4 or image.strides[2] != 1 or image.strides[1] != 4:
            raise ValueError("apply_damage: the image must be uint8 (H, W, 4) with contiguous rows")
        if not image.flags.writeable:
            raise ValueError("apply_damage: the image is read-only")
        t = np.ascontiguousarray(np.asarray(tiles, dtype=np.int32).reshape(-1, 4))
        px = np.ascontiguousarray(np.asarray(pixels, dtype=np.uint8))
        if px.size != len(t) * HipContext.TILE_BYTES:
            raise ValueError("apply_damage: pixels must hold 16384 bytes per tile")
        rc = L.fdh_apply_damage(image.ctypes.data, image.strides[0], image.shape[1], image.shape[0], t.ctypes.data if len(t) else None,
                                px.ctypes.data if len(t) else None, len(t))
        if rc != 0:
            raise FigdrawHipError(rc, L.fdh_last_error().decode())

    # ---- coded damage readback (include/figdraw_hip_stream.h)
    TILE_SOLID, TILE_PAL, TILE_RUNS, TILE_RAW = 0, 1, 2, 3  # FDH_TILE_*
    CODED_TILE = np.dtype([("x", "<i2"), ("y", "<i2"), ("w", "<i2"), ("h", "<i2"), ("mode", "u1"), ("bits", "u1"), ("n", "<u2"), ("offset", "<u4"),
                           ("size", "<u4"), ("solid", "<u4")])  # FdhCodedTile

    def read_damage_coded(self):
        """the pending bins of the last frame, coded on the GPU -> (tiles: structured array (n,) of CODED_TILE in row-major bin order;
        payload: bytes, the blob the tiles' offsets point into; full: every bin of the grid is among them).  Copies: the library's
        buffers are reused by the next read.  Empties the pending set, as read_damage does."""
        t, p = C.c_void_p(), C.c_void_p()
        n, full, nbytes = C.c_int(), C.c_int(), C.c_int64()
        self._ck(self.L.fdh_read_damage_coded(self.h, C.byref(t), C.byref(p), C.byref(n), C.byref(nbytes), None, None, C.byref(full)))
        if n.value == 0:
            return np.zeros(0, self.CODED_TILE), b"", bool(full.value)
        tiles = np.frombuffer(C.string_at(t.value, n.value * self.CODED_TILE.itemsize), self.CODED_TILE).copy()
        return tiles, C.string_at(p.value, nbytes.value) if nbytes.value else b"", bool(full.value)

    @staticmethod
    def decode_damage(image: np.ndarray, tiles, payload) -> None:
        """host only (no context, no GPU): decode what read_damage_coded returned -- or what arrived over a wire -- into `image`, uint8
        (H, W, 4) with contiguous rows.  A stream that does not validate raises FigdrawHipError and leaves the image as it was."""
        L = load()
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 4 or image.strides[2] != 1 or image.strides[1] != 4:
            raise ValueError("decode_damage: the image must be uint8 (H, W, 4) with contiguous rows")
        if not image.flags.writeable:
            raise ValueError("decode_damage: the image is read-only")
        t = np.ascontiguousarray(np.asarray(tiles, dtype=HipContext.CODED_TILE).reshape(-1))
        blob = np.frombuffer(bytes(payload), np.uint8) if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload, np.uint8).reshape(-1)
        rc = L.fdh_decode_damage(image.ctypes.data, image.strides[0], image.shape[1], image.shape[0], t.ctypes.data if len(t) else None, len(t),
                                 blob.ctypes.data if blob.size else None, blob.size)
        if rc != 0:
            raise FigdrawHipError(rc, L.fdh_last_error().decode())

    @staticmethod
    def coded_damage_bound(w: int, h: int) -> int:
        """an upper bound of a coded read's payload bytes for a w x h frame"""
        return int(load().fdh_coded_damage_bound(int(w), int(h)))

    # ---- exact damage readback (include/figdraw_hip_exact.h)
    def set_damage_exact(self, on: bool):
        """a sub-mode of damage readback: every read first drops the pending bins whose pixels are what the last read left with the
        application (a device mirror of that frame, one more buffer of the grid's size), so its tiles are exactly the bins that
        changed.  Acts while damage readback is on; the first read afterwards is a fresh one.  Refused on record-only contexts."""
        self._ck(self.L.fdh_set_damage_exact(self.h, 1 if on else 0))

    def damage_exact_stats(self):
        """the last read with exact damage readback on -> (n_pending: bins pending before the filter, n_changed: bins it kept,
        fresh: the read filled the mirror and filtered nothing)"""
        a, b, f = C.c_int(), C.c_int(), C.c_int()
        self._ck(self.L.fdh_damage_exact_stats(self.h, C.byref(a), C.byref(b), C.byref(f)))
        return a.value, b.value, bool(f.value)

    # ---- moved damage readback (include_readback/figdraw_hip_moves.h)
    TILE_COPY = 4                                     # FDH_TILE_COPY
    DAMAGE_MOVES_MAX, DAMAGE_SHIFT_MAX = 8, 256       # FDH_DAMAGE_MOVES_MAX, FDH_DAMAGE_SHIFT_MAX
    DAMAGE_MOVE = np.dtype([("dx", "<i2"), ("dy", "<i2")])  # FdhDamageMove

    def read_damage_moved(self, moves=()):
        """read_damage_coded in stream version 2, with exact damage readback on: a changed tile that equals the rectangle at (dx, dy) from it
        of the image the receiver holds, for the first such (dx, dy) of `moves` (at most 8 pairs), comes as a COPY entry without payload
        -> (tiles, payload, full, n_copied).  Decode with decode_damage_moved."""
        mv = np.ascontiguousarray(np.asarray(moves, dtype=np.int16).reshape(-1, 2))
        t, p = C.c_void_p(), C.c_void_p()
        n, full, copied, nbytes = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        self._ck(self.L.fdh_read_damage_moved(self.h, mv.ctypes.data if len(mv) else None, len(mv), C.byref(t), C.byref(p), C.byref(n), C.byref(nbytes),
                                              None, None, C.byref(full), C.byref(copied)))
        if n.value == 0:
            return np.zeros(0, self.CODED_TILE), b"", bool(full.value), 0
        tiles = np.frombuffer(C.string_at(t.value, n.value * self.CODED_TILE.itemsize), self.CODED_TILE).copy()
        return tiles, C.string_at(p.value, nbytes.value) if nbytes.value else b"", bool(full.value), copied.value

    @staticmethod
    def decode_damage_moved(image: np.ndarray, tiles, payload) -> None:
        """host only: decode_damage for stream version 2 -- a COPY tile takes its pixels from `image` as it was before the call.  A stream
        that does not validate raises FigdrawHipError and leaves the image as it was."""
        L = load()
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 4 or image.strides[2] != 1 or image.strides[1] != 4:
            raise ValueError("decode_damage_moved: the image must be uint8 (H, W, 4) with contiguous rows")
        if not image.flags.writeable:
            raise ValueError("decode_damage_moved: the image is read-only")
        t = np.ascontiguousarray(np.asarray(tiles, dtype=HipContext.CODED_TILE).reshape(-1))
        blob = np.frombuffer(bytes(payload), np.uint8) if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload, np.uint8).reshape(-1)
        rc = L.fdh_decode_damage_moved(image.ctypes.data, image.strides[0], image.shape[1], image.shape[0], t.ctypes.data if len(t) else None, len(t),
                                       blob.ctypes.data if blob.size else None, blob.size)
        if rc != 0:
            raise FigdrawHipError(rc, L.fdh_last_error().decode())

    def find_damage_moves(self, max_shift: int = 64, cap: int = 8):
        """the mover: the scroll vectors the pending bins of the last frame vote for against the image the receiver holds -> (moves int16
        (n, 2): dx, dy; votes int32 (n,)), best first.  Changes nothing; what it proposes, read_damage_moved confirms pixel for pixel."""
        mv, votes, n = np.zeros((max(cap, 0), 2), np.int16), np.zeros(max(cap, 0), np.int32), C.c_int()
        self._ck(self.L.fdh_find_damage_moves(self.h, int(max_shift), mv.ctypes.data if cap > 0 else None, votes.ctypes.data if cap > 0 else None, int(cap),
                                              C.byref(n)))
        return mv[:n.value].copy(), votes[:n.value].copy()

    # ---- picking (include/figdraw_hip_pick.h)
    PICK_SHADOWS = 1  # FDH_PICK_SHADOWS
    PICK_HIT = np.dtype([("zlevel", "<i4"), ("id", "<i4"), ("draw", "<i4"), ("alpha", "u1"), ("mode", "u1"), ("reserved", "<u2")])

    def set_pick(self, on: bool):
        """keep each frame's record tags from the next frame begun on, so that pick_points / pick_region can say which draw and which
        node owns a pixel of the last submitted frame"""
        self._ck(self.L.fdh_set_pick(self.h, 1 if on else 0))

    def set_pick_tag(self, zlevel: int, id: int):
        """the tag (zlevel, id) of the draw calls that follow (call-level frames; begin_frame resets it to (-1, -1))"""
        self._ck(self.L.fdh_set_pick_tag(self.h, int(zlevel), int(id)))

    def pick_points(self, xy, threshold: int = 128, flags: int = 0, max_hits: int = 1):
        """hits at points xy (N x 2, frame pixels), front to back: (hits, counts) -- hits a structured array (N, max_hits) of PICK_HIT,
        counts[i] the hits of point i"""
        pts = np.ascontiguousarray(np.asarray(xy, dtype=np.float32).reshape(-1, 2))
        n = pts.shape[0]
        hits = np.zeros((n, int(max_hits)), dtype=self.PICK_HIT)
        counts = np.zeros(n, dtype=np.int32)
        self._ck(self.L.fdh_pick_points(self.h, pts.ctypes.data, n, int(threshold), int(flags), int(max_hits), hits.ctypes.data, counts.ctypes.data))
        return hits, counts

    def top_node_at(self, x: float, y: float, threshold: int = 128):
        """(zlevel, id) of the front-most draw that hits pixel (x, y), or None (topFigAtPoint)"""
        hits, counts = self.pick_points([(x, y)], threshold=threshold, max_hits=1)
        return (int(hits[0, 0]["zlevel"]), int(hits[0, 0]["id"])) if counts[0] else None

    def pick_region(self, x: int = 0, y: int = 0, w: Optional[int] = None, h: Optional[int] = None, threshold: int = 128, flags: int = 0) -> np.ndarray:
        """the front-most hit's draw index per pixel of the rectangle (default: the whole frame), -1 where nothing hits: int32 (h, w)"""
        w = self.W - x if w is None else int(w)
        h = self.H - y if h is None else int(h)
        out = np.empty((max(h, 0), max(w, 0)), dtype=np.int32)
        self._ck(self.L.fdh_pick_region(self.h, int(x), int(y), w, h, int(threshold), int(flags), out.ctypes.data))
        return out

    def pick_draw_tags(self) -> np.ndarray:
        """the tag of every record of the last frame, painter's order: int32 (n, 2) of (zlevel, id); works on record-only contexts"""
        n = C.c_int()
        self._ck(self.L.fdh_pick_draw_tags(self.h, None, None, 0, C.byref(n)))
        z = np.zeros(n.value, dtype=np.int32)
        i = np.zeros(n.value, dtype=np.int32)
        self._ck(self.L.fdh_pick_draw_tags(self.h, z.ctypes.data, i.ctypes.data, n.value, C.byref(n)))
        return np.stack([z, i], axis=1)

    def visible_pixels(self, threshold: int = 128, flags: int = 0) -> dict:
        """exact visibility (figVisibility): {(zlevel, id): pixels of the frame whose front-most hit is a draw of that tag}"""
        region = self.pick_region(threshold=threshold, flags=flags)
        tags = self.pick_draw_tags()
        draws, n = np.unique(region[region >= 0], return_counts=True)
        out: dict = {}
        for d, c in zip(draws.tolist(), n.tolist()):
            key = (int(tags[d, 0]), int(tags[d, 1]))
            out[key] = out.get(key, 0) + int(c)
        return out

    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId through the library (rank 0 makes it; the host carries the 128 bytes to the other ranks)"""
        L = load()
        buf = C.create_string_buffer(128)
        rc = L.fdh_comm_unique_id(buf)
        if rc != 0:
            raise FigdrawHipError(rc, L.fdh_last_error().decode())
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        self._ck(self.L.fdh_comm_init(self.h, unique_id, int(rank), int(world)))

    def comm_share(self, owner: "HipContext"):
        """use `owner`'s communicator (several contexts of one process share one)"""
        self._ck(self.L.fdh_comm_share(self.h, owner.h))

    def comm_destroy(self):
        self._ck(self.L.fdh_comm_destroy(self.h))

    def gather_stripes(self, dst_rank: int = 0, dst_ptr: Optional[int] = None):
        """row-stripe mode: this rank's rows (fdh_stripe_rows) go to dst_rank's image (device pointer; None: its own surface)"""
        self._ck(self.L.fdh_gather_stripes(self.h, int(dst_rank), C.c_void_p(dst_ptr or 0)))

    def gather_frames(self, dst_rank: int = 0, dst_ptrs=None):
        """frame-parallel mode: every rank's whole frame goes to dst_rank's dst_ptrs[r] (device pointers)"""
        arr = (C.c_void_p * len(dst_ptrs))(*dst_ptrs) if dst_ptrs else None
        self._ck(self.L.fdh_gather_frames(self.h, int(dst_rank), arr))

    def replay(self, times: int = 1):
        self._ck(self.L.fdh_replay(self.h, int(times)))

    def replay_async(self, times: int = 1):
        self._ck(self.L.fdh_replay_async(self.h, int(times)))

    def replay_timed(self, times: int):
        """Per-frame stream times (ms) of `times` back-to-back frames."""
        out = (C.c_float * int(times))()
        self._ck(self.L.fdh_replay_timed(self.h, int(times), out))
        return np.array(out, dtype=np.float32)

    def profile(self, times: int = 1):
        self._ck(self.L.fdh_profile(self.h, int(times)))

    def frame_stats(self) -> FrameStats:
        st = FrameStats()
        self._ck(self.L.fdh_get_frame_stats(self.h, C.byref(st)))
        return st

    def block_wave_bins(self) -> int:
        """bins of the last frame's full-frame compositor launch that had one wave per 32 x 32 block; -1: the launch did not take that form"""
        n = C.c_int(0)
        self._ck(self.L.fdh_block_wave_bins(self.h, C.byref(n)))
        return n.value
