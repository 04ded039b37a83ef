/* fdh_read_video_frame, fdh_check_video_target and fdh_video_out_coefficients through the C ABI in C99
 * (include_video/figdraw_hip_video_out.h): no GPU needed -- the check and the coefficients need no context, and a record-only context
 * refuses the read.  tests/test_video_out_host.py compiles this with -std=c99 -Wall -Wextra -Werror -pedantic -I include_video and runs it. */
#include "figdraw_hip_video_out.h"
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  static uint32_t luma[16 * 9], chroma[8 * 5];  /* stand for device memory: nothing here touches it */
  const float black[4] = {0.0f, 0.0f, 0.0f, 1.0f};
  FdhVideoTarget t, bad;
  int32_t k[11];
  CHECK(sizeof(FdhVideoTarget) == 72);
  OK(fdh_video_out_coefficients(FDH_VIDEO_NV12, FDH_VIDEO_BT709, FDH_VIDEO_LIMITED, k));
  CHECK(k[0] == 16 && k[1] == 128 && k[2] == 2991 && k[3] == 10064 && k[4] == 1016 && k[5] == -1649 && k[6] == -5547 && k[7] == 7196);
  CHECK(k[8] == 7196 && k[9] == -6536 && k[10] == -660);
  OK(fdh_video_out_coefficients(FDH_VIDEO_P010, FDH_VIDEO_BT2020, FDH_VIDEO_FULL, k));
  CHECK(k[0] == 0 && k[1] == 512 && k[2] == 17267 && k[10] == -2643);
  CHECK(fdh_video_out_coefficients(FDH_VIDEO_BGRA8, 0, 0, k) == FDH_ERR_INVALID);
  CHECK(fdh_video_out_coefficients(FDH_VIDEO_NV12, 3, 0, k) == FDH_ERR_INVALID);
  memset(&t, 0, sizeof t);
  t.planes[0] = luma; t.planes[1] = chroma; t.pitch_bytes[0] = 16; t.pitch_bytes[1] = 16;
  t.format = FDH_VIDEO_NV12; t.matrix = FDH_VIDEO_BT709; t.range = FDH_VIDEO_LIMITED; t.flags = FDH_VIDEO_CHROMA_LINEAR;
  OK(fdh_check_video_target(&t, 16, 9));
  t.rect[0] = 2; t.rect[1] = 4; t.rect[2] = 13; t.rect[3] = 5;
  OK(fdh_check_video_target(&t, 16, 9));
  bad = t; bad.rect[0] = 3;
  CHECK(fdh_check_video_target(&bad, 16, 9) == FDH_ERR_INVALID);                 /* an odd x */
  CHECK(strstr(fdh_last_error(), "check_video_target: ") == fdh_last_error());
  bad = t; bad.rect[2] = 15;
  CHECK(fdh_check_video_target(&bad, 16, 9) == FDH_ERR_INVALID);                 /* outside the frame */
  bad = t; bad.planes[1] = NULL;
  CHECK(fdh_check_video_target(&bad, 16, 9) == FDH_ERR_INVALID);
  bad = t; bad.flags = FDH_VIDEO_STRAIGHT_ALPHA;
  CHECK(fdh_check_video_target(&bad, 16, 9) == FDH_ERR_INVALID);
  bad = t; bad.reserved[1] = 1;
  CHECK(fdh_check_video_target(&bad, 16, 9) == FDH_ERR_INVALID);
  bad = t; bad.planes[1] = (char*)luma + 32;
  CHECK(fdh_check_video_target(&bad, 16, 9) == FDH_ERR_INVALID);                 /* the planes overlap */
  CHECK(fdh_check_video_target(NULL, 16, 9) == FDH_ERR_INVALID);
  bad = t; bad.format = FDH_VIDEO_BGRA8; bad.planes[1] = NULL; bad.pitch_bytes[0] = 64; bad.pitch_bytes[1] = 0;
  bad.matrix = 0; bad.range = 0; bad.flags = FDH_VIDEO_IGNORE_ALPHA; bad.rect[0] = 1;
  OK(fdh_check_video_target(&bad, 16, 9));                                       /* BGRA8 takes an odd x */
  /* a record-only context has no frame to hand out */
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  OK(fdh_begin_frame(c, 16, 9, 1, black));
  OK(fdh_end_frame(c));
  CHECK(fdh_read_video_frame(c, &t) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "read_video_frame: ") == fdh_last_error());
  CHECK(fdh_read_video_frame(NULL, &t) == FDH_ERR_INVALID);
  fdh_destroy(c);
  printf("video_out_abi_smoke: OK\n");
  return 0;
}
