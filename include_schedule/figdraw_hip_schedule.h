/* figdraw_hip_schedule.h -- what the compositor's full-frame launch of the last frame was scheduled as, for libfigdraw_hip.so.  Same
 * conventions as figdraw_hip.h (plain C, every call returns 0 or a negative FdhStatus, fdh_last_error() says why).  The header lives in
 * include_schedule/ and reaches figdraw_hip.h by its relative path: -I include_schedule is all a caller adds.  No counterpart in the
 * reference.
 *
 * Block waves.  The launch that starts a frame shades 32 x 8 strips, one wavefront each.  Where the frame has no partial strip (width a
 * multiple of 32, height of 8, no row stripe), the previous frame's order of bins is at hand and the launch is the one of the builds
 * without clips, atlas quads or rotated quads, a bin whose list holds at most a threshold of draws can get one wavefront per 32 x 32
 * block instead -- four strips shaded one after the other.  The library does that while other contexts have frames in flight on the
 * device (FDH_BLOCK_MAX=n in the environment: always, with threshold n; FDH_BLOCK_WAVES=0: never).  It is a schedule: no pixel depends
 * on it. */
#ifndef FIGDRAW_HIP_SCHEDULE_H
#define FIGDRAW_HIP_SCHEDULE_H
#include "../include/figdraw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* *out = how many bins of the LAST frame's full-frame compositor launch had one wavefront per 32 x 32 block; -1: that launch did not take
 * the form (a frame size with partial strips, a striped context, a context's first frame, a launch with deep strips, a frame of a handful
 * of draws, a tracked frame that was not rendered in full, FDH_BLOCK_WAVES=0, or no other context was rendering).  Waits for the
 * context's submit thread, not for the GPU. */
FDH_API int fdh_block_wave_bins(FdhContext*, int* out);

#ifdef __cplusplus
}
#endif
#endif
