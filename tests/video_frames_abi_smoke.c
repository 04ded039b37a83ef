/* fdh_put_video_frames, fdh_update_video_frames and fdh_video_batch_stats through the C ABI in C99 (include_glyphs/
 * figdraw_hip_video_frames.h), on a record-only context: no GPU needed, and the planes are never read.  tests/test_video_frames_host.py
 * compiles this with -std=c99 -Wall -Wextra -Werror -pedantic -I include_glyphs and runs it. */
#include "figdraw_hip_video_frames.h"
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  static uint32_t bytes[64 * 40];  /* stands for device memory: a record-only context touches none of it */
  FdhVideoFrame f[3];
  FdhVideoBatchStats st;
  int64_t keys[3] = {11, 12, 13}, twice[3] = {11, 12, 11};
  int rects[3][4], has = 0, i;
  CHECK(sizeof(FdhVideoFrame) == 64 && fdh_sizeof_video_frame() == 64);
  CHECK(sizeof(FdhVideoBatchStats) == 32);
  memset(f, 0, sizeof f);
  memset(rects, 0xFF, sizeof rects);
  f[0].planes[0] = bytes; f[0].planes[1] = bytes + 1024; f[0].pitch_bytes[0] = 64; f[0].pitch_bytes[1] = 64; f[0].width = 64; f[0].height = 40;
  f[0].format = FDH_VIDEO_NV12; f[0].matrix = FDH_VIDEO_BT709; f[0].range = FDH_VIDEO_LIMITED; f[0].flags = FDH_VIDEO_CHROMA_LINEAR;
  f[1].planes[0] = bytes; f[1].planes[1] = bytes + 1024; f[1].pitch_bytes[0] = 30; f[1].pitch_bytes[1] = 32; f[1].width = 15; f[1].height = 9;
  f[1].format = FDH_VIDEO_P010; f[1].matrix = FDH_VIDEO_BT2020; f[1].range = FDH_VIDEO_FULL;
  f[2].planes[0] = bytes; f[2].pitch_bytes[0] = 32; f[2].width = 8; f[2].height = 1;
  f[2].format = FDH_VIDEO_BGRA8; f[2].flags = FDH_VIDEO_STRAIGHT_ALPHA;
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  OK(fdh_put_video_frames(c, keys, f, 0, NULL));   /* nothing */
  OK(fdh_put_video_frames(c, keys, f, 3, rects));
  for (i = 0; i < 3; i++) {
    CHECK(rects[i][2] == f[i].width && rects[i][3] == f[i].height && rects[i][0] >= 0 && rects[i][1] >= 0);
    OK(fdh_has_image(c, keys[i], &has)); CHECK(has);
  }
  OK(fdh_video_batch_stats(c, &st));
  /* (a frame 1 texel high keeps its tile) */
  CHECK(st.frames == 3 && st.written == 3 && st.dropped_by_growth == 0 && st.tiles == 4 + 1 + 1 && st.launches == 0 && st.reserved == 0 && st.bytes_copied == 0);
  OK(fdh_update_video_frames(c, keys, f, 3));
  OK(fdh_update_video_frames(c, keys + 1, f + 1, 2));
  OK(fdh_video_batch_stats(c, &st));
  CHECK(st.frames == 2 && st.written == 2);
  OK(fdh_put_video_frames(c, keys, f, 3, NULL));   /* out_rects may be NULL */
  /* refusals, each before anything is placed or begun; the stats stay the last good batch's */
  CHECK(fdh_put_video_frames(c, keys, f, -1, rects) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "put_video_frames") != NULL);
  CHECK(fdh_put_video_frames(c, NULL, f, 3, rects) == FDH_ERR_INVALID);
  CHECK(fdh_put_video_frames(c, keys, NULL, 3, rects) == FDH_ERR_INVALID);
  CHECK(fdh_put_video_frames(c, twice, f, 3, rects) == FDH_ERR_INVALID);
  CHECK(fdh_update_video_frames(c, twice, f, 3) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "update_video_frames") != NULL);
  f[2].width = 2049; f[2].pitch_bytes[0] = 4 * 2049;
  CHECK(fdh_put_video_frames(c, keys, f, 3, rects) == FDH_ERR_INVALID);
  f[2].width = 8; f[2].pitch_bytes[0] = 32; f[2].reserved[1] = 1;
  CHECK(fdh_put_video_frames(c, keys, f, 3, rects) == FDH_ERR_INVALID);
  f[2].reserved[1] = 0;
  keys[2] = 77;
  CHECK(fdh_update_video_frames(c, keys, f, 3) == FDH_ERR_INVALID);                /* an unknown key */
  CHECK(fdh_put_video_frames(NULL, keys, f, 3, rects) == FDH_ERR_INVALID);
  CHECK(fdh_video_batch_stats(c, NULL) == FDH_ERR_INVALID);
  OK(fdh_has_image(c, 77, &has)); CHECK(!has);
  OK(fdh_video_batch_stats(c, &st));
  CHECK(st.frames == 3 && st.written == 3);
  fdh_destroy(c);
  printf("video_frames_abi_smoke: OK\n");
  return 0;
}
