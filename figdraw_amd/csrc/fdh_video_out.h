// fdh_video_out.h -- the host side of the four calls that hand the rendered frame out: fdh_read_video_frame (NV12, P010, BGRA8;
// include_video/figdraw_hip_video_out.h), fdh_read_video_planes (I420, I010, I444, I410; figdraw_hip_video_planar.h), fdh_read_video_422
// (I422, I210, YUY2, UYVY; figdraw_hip_video_422.h) and fdh_read_video_alpha (A420, A444, A410, UYVA; figdraw_hip_video_alpha.h): a
// target's rules, the parameter block of the family's export kernel and its launch.  Free functions, no state: Context::read_video drains,
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

// fdh_check_video_target, _planes_target, _422_target, _alpha_target: every rule that needs no device, for a frame of frame_w x frame_h;
// throw Error(FDH_ERR_INVALID, who + ": " + why)
void check_target(const char* who, const FdhVideoTarget* t, int frame_w, int frame_h);
void check_planes_target(const char* who, const FdhVideoPlanesTarget* t, int frame_w, int frame_h);
void check_422_target(const char* who, const FdhVideoPlanesTarget* t, int frame_w, int frame_h);
void check_alpha_target(const char* who, const FdhVideoAlphaPlanesTarget* t, int frame_w, int frame_h);
// fdh_video_out_coefficients: a row of video_export::kCoefficients (fdh_video_export.h)
void coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[11]);
// memory of the context's that no plane may touch: a frame surface, a level of the atlas
struct Own { const void* base; size_t bytes; const char* what; };
// the four calls behind the context's part: the target's check, the planes' addresses on `device` and their distance from `own` and from
// each other, one launch of k_video_export, k_video_planar_export, k_video_422_export or k_video_alpha_export on `s` reading the W x H
// surface, and the wait for it
void read(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoTarget* t, const Own* own, int n_own);
void read_planes(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoPlanesTarget* t, const Own* own, int n_own);
void read_422(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoPlanesTarget* t, const Own* own, int n_own);
void read_alpha(hipStream_t s, int device, const uint32_t* surface, int W, int H, const FdhVideoAlphaPlanesTarget* t, const Own* own, int n_own);

}  // namespace video_out
}  // namespace fdh
