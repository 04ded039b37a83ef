// fdh_video_out.h -- fdh_read_video_frame's host side (the specification: include_video/figdraw_hip_video_out.h): the rules of an
// FdhVideoTarget, the parameter block of k_video_export and its launch.  Free functions, no state: Context::read_video_frame drains,
// checks that there is a frame, synchronises and hands over the stream, the surface that holds the frame and what may not be written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include_video/figdraw_hip_video_out.h"     // FdhVideoTarget
#include "../../include_video/figdraw_hip_video_alpha.h"  // FdhVideoAlphaPlanesTarget; through it figdraw_hip_video_422.h (the 4:2:2 formats) and
                                                          // figdraw_hip_video_planar.h (FdhVideoPlanesTarget)

namespace fdh {
namespace video_out {

// fdh_check_video_target: every rule that needs no device, for a frame of frame_w x frame_h; throws Error(FDH_ERR_INVALID, who + ": " + why)
void check_target(const char* who, const FdhVideoTarget* t, int frame_w, int frame_h);
// fdh_video_out_coefficients: a row of video_export::kCoefficients (fdh_video_export.h)
void coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[11]);
// memory of the context's that no plane may touch: a frame surface, a level of the atlas
struct Own { const void* base; size_t bytes; const char* what; };
// fdh_read_video_frame behind the context's part: check_target, the planes' addresses on `device` and their distance from `own`, one
// launch of k_video_export on `s` reading the W x H surface, and the wait for it
void read(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoTarget* t, const Own* own, int n_own);

// The same for three planes, I420, I010, I444 and I410 (the specification: include_video/figdraw_hip_video_planar.h).
// fdh_check_video_planes_target: every rule that needs no device
void check_planes_target(const char* who, const FdhVideoPlanesTarget* t, int frame_w, int frame_h);
// fdh_read_video_planes behind the context's part: one launch of k_video_planar_export on `s`, and the wait for it
void read_planes(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoPlanesTarget* t, const Own* own, int n_own);

// The same for 4:2:2, I422 and I210 in three planes, YUY2 and UYVY in one (the specification: include_video/figdraw_hip_video_422.h).
// fdh_check_video_422_target: every rule that needs no device
void check_422_target(const char* who, const FdhVideoPlanesTarget* t, int frame_w, int frame_h);
// fdh_read_video_422 behind the context's part: one launch of k_video_422_export on `s`, and the wait for it
void read_422(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoPlanesTarget* t, const Own* own, int n_own);

// The same with an alpha plane, A420, A444 and A410 in four planes, UYVA in two (the specification: include_video/figdraw_hip_video_alpha.h).
// fdh_check_video_alpha_target: every rule that needs no device
void check_alpha_target(const char* who, const FdhVideoAlphaPlanesTarget* t, int frame_w, int frame_h);
// fdh_read_video_alpha behind the context's part: one launch of k_video_alpha_export on `s`, and the wait for it
void read_alpha(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoAlphaPlanesTarget* t, const Own* own, int n_own);

}  // namespace video_out
}  // namespace fdh
