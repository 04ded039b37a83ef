/* fdh_put_video_frame, fdh_update_video_frame and fdh_video_coefficients through the C ABI in C99 (include_glyphs/figdraw_hip_video_frame.h),
 * on a record-only context: no GPU needed, and the planes are never read.  tests/test_video_frame_host.py compiles this with -std=c99 -Wall
 * -Wextra -Werror -pedantic -I include_glyphs and runs it. */
#include "figdraw_hip_video_frame.h"
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  static uint32_t luma[16 * 9], chroma[8 * 5];  /* stand for device memory: a record-only context touches none of it */
  FdhVideoFrame f, bad;
  int32_t k[7];
  int rect[4], has = 0;
  CHECK(sizeof(FdhVideoFrame) == 64);
  OK(fdh_video_coefficients(FDH_VIDEO_NV12, FDH_VIDEO_BT709, FDH_VIDEO_LIMITED, k));
  CHECK(k[0] == 16 && k[1] == 128 && k[2] == 19077 && k[3] == 29372 && k[4] == 3494 && k[5] == 8731 && k[6] == 34610);
  OK(fdh_video_coefficients(FDH_VIDEO_P010, FDH_VIDEO_BT2020, FDH_VIDEO_FULL, k));
  CHECK(k[0] == 0 && k[1] == 512 && k[2] == 4084 && k[6] == 7684);
  CHECK(fdh_video_coefficients(FDH_VIDEO_BGRA8, 0, 0, k) == FDH_ERR_INVALID);
  CHECK(fdh_video_coefficients(FDH_VIDEO_NV12, 3, 0, k) == FDH_ERR_INVALID);
  memset(&f, 0, sizeof f);
  f.planes[0] = luma; f.planes[1] = chroma; f.pitch_bytes[0] = 16; f.pitch_bytes[1] = 16; f.width = 16; f.height = 9;
  f.format = FDH_VIDEO_NV12; f.matrix = FDH_VIDEO_BT709; f.range = FDH_VIDEO_LIMITED; f.flags = FDH_VIDEO_CHROMA_LINEAR;
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  OK(fdh_put_video_frame(c, 1, &f, rect));
  CHECK(rect[2] == 16 && rect[3] == 9 && rect[0] >= 0 && rect[1] >= 0);
  OK(fdh_has_image(c, 1, &has)); CHECK(has);
  OK(fdh_update_video_frame(c, 1, &f));
  bad = f; bad.format = FDH_VIDEO_P010; bad.pitch_bytes[0] = 32; bad.pitch_bytes[1] = 32; bad.flags = 0;   /* 16 x 9 words */
  OK(fdh_put_video_frame(c, 2, &bad, NULL));
  bad = f; bad.format = FDH_VIDEO_BGRA8; bad.planes[1] = NULL; bad.pitch_bytes[0] = 64; bad.pitch_bytes[1] = 0;
  bad.matrix = 0; bad.range = 0; bad.flags = FDH_VIDEO_IGNORE_ALPHA;
  OK(fdh_put_video_frame(c, 3, &bad, rect));
  CHECK(rect[2] == 16 && rect[3] == 9);
  /* refusals, each before anything is placed */
  CHECK(fdh_put_video_frame(c, 9, NULL, rect) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "put_video_frame") != NULL);
  bad = f; bad.planes[0] = NULL;
  CHECK(fdh_put_video_frame(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = f; bad.planes[1] = NULL;
  CHECK(fdh_put_video_frame(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = f; bad.width = 0;
  CHECK(fdh_put_video_frame(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = f; bad.format = 3;
  CHECK(fdh_put_video_frame(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = f; bad.flags = FDH_VIDEO_STRAIGHT_ALPHA;
  CHECK(fdh_put_video_frame(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = f; bad.reserved[1] = 1;
  CHECK(fdh_put_video_frame(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = f; bad.pitch_bytes[1] = 14;
  CHECK(fdh_put_video_frame(c, 9, &bad, rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_video_frame(NULL, 9, &f, rect) == FDH_ERR_INVALID);
  CHECK(fdh_update_video_frame(c, 77, &f) == FDH_ERR_INVALID);                  /* an unknown key */
  CHECK(strstr(fdh_last_error(), "update_video_frame") != NULL);
  bad = f; bad.height = 8;
  CHECK(fdh_update_video_frame(c, 1, &bad) == FDH_ERR_INVALID);                 /* not the entry's size */
  OK(fdh_has_image(c, 9, &has)); CHECK(!has);
  fdh_destroy(c);
  printf("video_frame_abi_smoke: OK\n");
  return 0;
}
