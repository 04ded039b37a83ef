// fdh_video_export.h -- the parameter block of k_video_export (k_video_export.hip), the kernel behind fdh_read_video_frame (the
// specification: include_video/figdraw_hip_video_out.h), and the table of the conversion's coefficients.  Plain C++, no HIP and no context:
// fdh_video_out.cpp fills the block, tests/video_out_emu compiles it as it stands, with the kernel beside it.
#pragma once
#include <cstdint>

namespace fdh {
namespace video_export {

enum : uint32_t { kBgra8 = 0, kNv12 = 1, kP010 = 2 };       // FdhVideoTarget::format (the values of fdh_video_import.h)
enum : uint32_t { kChromaLinear = 1, kIgnoreAlpha = 4 };     // FdhVideoTarget::flags

// The tile of a workgroup of kGroup lanes: kTileW x kTileH texels of the rectangle, a lane per run of four texels by two rows -- 32 runs
// across, 8 row pairs down; a wave covers two row pairs of the tile's whole width.
constexpr int kGroup = 256, kRun = 4, kTileW = 128, kTileH = 16;

// Yoff, Coff, kYR, kYG, kYB, kUR, kUG, kUB, kVR, kVG, kVB: derived in the specification with exact rationals (tests/test_video_out_host.py
// derives them again).  Rows: matrix (BT601, BT709, BT2020) x range (limited, full), 8 bit then 10.
constexpr int32_t kCoefficients[2][3][2][11] = {
    {{{16, 128, 4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170}, {0, 128, 4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332}},
     {{16, 128, 2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660}, {0, 128, 3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751}},
     {{16, 128, 3696, 9541, 834, -2010, -5186, 7196, 7196, -6617, -579}, {0, 128, 4304, 11108, 972, -2288, -5904, 8192, 8192, -7533, -659}}},
    {{{64, 512, 16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681}, {0, 512, 19653, 38583, 7493, -11091, -21773, 32864, 32864, -27519, -5345}},
     {{64, 512, 11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639}, {0, 512, 13974, 47009, 4746, -7531, -25333, 32864, 32864, -29851, -3013}},
     {{64, 512, 14786, 38160, 3338, -8038, -20746, 28784, 28784, -26469, -2315}, {0, 512, 17267, 44564, 3898, -9178, -23686, 32864, 32864, -30221, -2643}}}};

struct Params {
  const uint32_t* src;   // texel (0, 0) of the rectangle in the frame surface, RGBA8
  int64_t src_pitch;     // between rows of the surface, texels
  int32_t w, h;          // of the rectangle = of the luma plane; the chroma plane is ceil(w / 2) x ceil(h / 2) pairs
  void* luma;            // planes[0] as the device addresses it: the luma samples, or the BGRA texels
  void* chroma;          // planes[1]: the Cb, Cr pairs (BGRA8: unused)
  int64_t pitch_y, pitch_c;  // between rows of either plane, bytes
  uint32_t format;       // kBgra8, kNv12, kP010: with kChromaLinear, which build of k_video_export takes the launch
  uint32_t flags;
  int32_t wide_src;      // src and src_pitch are multiples of a run's 16 bytes and w >= 4: a whole run is one load
  int32_t wide_y;        // luma and pitch_y are multiples of a run's bytes (NV12 4, P010 8, BGRA8 16) and w >= 4: a whole run is one store
  int32_t wide_c;        // chroma and pitch_c are multiples of two pairs' bytes (NV12 4, P010 8) and ceil(w / 2) >= 2: two pairs are one store
  int32_t yoff, coff;    // the conversion (a row of kCoefficients)
  int32_t ky[3], ku[3], kv[3];  // the rows of R, G, B
};

}  // namespace video_export
}  // namespace fdh
