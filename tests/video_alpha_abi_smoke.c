/* fdh_put_video_alpha, fdh_update_video_alpha, fdh_read_video_alpha and fdh_check_video_alpha_target through the C ABI in C99
 * (include_video/figdraw_hip_video_alpha.h): no GPU needed -- the check needs no context, and a record-only context validates and places
 * on the way in and refuses the read.  tests/test_video_alpha_host.py compiles this with -std=c99 -Wall -Wextra -Werror -pedantic
 * -I include_video and runs it. */
#include "figdraw_hip_video_alpha.h"
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  static uint32_t y[16 * 9], cb[16 * 9], cr[16 * 9], a[16 * 9];  /* stand for device memory: nothing here touches it */
  const float black[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  FdhVideoAlphaPlanes f, badf;
  FdhVideoAlphaPlanesTarget t, bad;
  int rect[4], has = 0, p;
  CHECK(sizeof(FdhVideoAlphaPlanes) == 96 && sizeof(FdhVideoAlphaPlanesTarget) == 104);
  CHECK(FDH_VIDEO_A420 == 11 && FDH_VIDEO_A444 == 12 && FDH_VIDEO_A410 == 13 && FDH_VIDEO_UYVA == 14);
  /* the way out: the rules that need no device */
  memset(&t, 0, sizeof t);
  t.planes[0] = y; t.planes[1] = cb; t.planes[2] = cr; t.planes[3] = a;
  for (p = 0; p < 4; p++) t.pitch_bytes[p] = 16;
  t.format = FDH_VIDEO_A444; t.matrix = FDH_VIDEO_BT709; t.range = FDH_VIDEO_FULL; t.flags = FDH_VIDEO_STRAIGHT_ALPHA;
  OK(fdh_check_video_alpha_target(&t, 16, 9));
  t.rect[0] = 3; t.rect[1] = 3; t.rect[2] = 13; t.rect[3] = 5;
  OK(fdh_check_video_alpha_target(&t, 16, 9));                                   /* 4:4:4: any rectangle inside the frame */
  bad = t; bad.format = FDH_VIDEO_A420; bad.pitch_bytes[1] = 8; bad.pitch_bytes[2] = 8;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);           /* A420: x and y even */
  CHECK(strstr(fdh_last_error(), "check_video_alpha_target: ") == fdh_last_error());
  bad.rect[0] = 2; bad.rect[1] = 4; bad.flags |= FDH_VIDEO_CHROMA_LINEAR;
  OK(fdh_check_video_alpha_target(&bad, 16, 9));
  bad = t; bad.planes[3] = NULL;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);           /* the alpha plane is not optional */
  bad = t; bad.format = FDH_VIDEO_I444;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);
  bad = t; bad.format = 15;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);
  bad = t; bad.flags = FDH_VIDEO_IGNORE_ALPHA;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);
  bad = t; bad.flags = FDH_VIDEO_CHROMA_LINEAR;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);           /* 4:4:4 has a chroma sample per texel */
  bad = t; bad.reserved[1] = 1;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);
  bad = t; bad.planes[3] = (char*)cr + 4;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);           /* Cr and A overlap */
  bad = t; bad.format = FDH_VIDEO_A410;
  for (p = 0; p < 4; p++) bad.pitch_bytes[p] = 32;
  OK(fdh_check_video_alpha_target(&bad, 16, 9));
  bad.planes[3] = (char*)a + 1;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);           /* a 16-bit sample at an odd address */
  bad = t; bad.format = FDH_VIDEO_UYVA;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);           /* UYVA has two planes, and an even x */
  bad.planes[1] = NULL; bad.planes[2] = NULL; bad.pitch_bytes[1] = 0; bad.pitch_bytes[2] = 0; bad.pitch_bytes[0] = 28; bad.pitch_bytes[3] = 13;
  bad.rect[0] = 2;
  OK(fdh_check_video_alpha_target(&bad, 16, 9));                                 /* 13 columns: seven groups; an odd y is fine */
  bad.planes[3] = (char*)y + 28 * 4 + 28;
  OK(fdh_check_video_alpha_target(&bad, 16, 9));                                 /* one block: the alpha plane right behind the UYVY plane */
  bad.planes[3] = (char*)y + 28 * 4 + 27;
  CHECK(fdh_check_video_alpha_target(&bad, 16, 9) == FDH_ERR_INVALID);
  CHECK(fdh_check_video_alpha_target(NULL, 16, 9) == FDH_ERR_INVALID);
  /* the way in on a record-only context: validated and placed, no memory touched */
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  memset(&f, 0, sizeof f);
  f.planes[0] = y; f.planes[1] = cb; f.planes[2] = cr; f.planes[3] = a;
  f.pitch_bytes[0] = 16; f.pitch_bytes[1] = 8; f.pitch_bytes[2] = 8; f.pitch_bytes[3] = 16;
  f.width = 16; f.height = 9; f.format = FDH_VIDEO_A420; f.matrix = FDH_VIDEO_BT601; f.range = FDH_VIDEO_FULL;
  f.flags = FDH_VIDEO_CHROMA_LINEAR | FDH_VIDEO_STRAIGHT_ALPHA;
  OK(fdh_put_video_alpha(c, 7, &f, rect));
  OK(fdh_has_image(c, 7, &has));
  CHECK(rect[2] == 16 && rect[3] == 9 && has);
  badf = f; badf.planes[3] = f.planes[0];
  OK(fdh_update_video_alpha(c, 7, &badf));                                       /* the planes may alias on the way in */
  badf = f; badf.format = FDH_VIDEO_UYVA; badf.planes[1] = NULL; badf.planes[2] = NULL; badf.pitch_bytes[0] = 32; badf.pitch_bytes[1] = 0; badf.pitch_bytes[2] = 0;
  OK(fdh_update_video_alpha(c, 7, &badf));                                       /* the next frame may come in another format */
  badf.pitch_bytes[2] = 8;
  CHECK(fdh_update_video_alpha(c, 7, &badf) == FDH_ERR_INVALID);
  badf = f; badf.width = 15;
  CHECK(fdh_update_video_alpha(c, 7, &badf) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "update_video_alpha: ") == fdh_last_error());
  CHECK(fdh_update_video_alpha(c, 8, &f) == FDH_ERR_INVALID);
  badf = f; badf.pitch_bytes[3] = 15;
  CHECK(fdh_put_video_alpha(c, 8, &badf, NULL) == FDH_ERR_INVALID);
  badf = f; badf.flags = FDH_VIDEO_IGNORE_ALPHA;
  CHECK(fdh_put_video_alpha(c, 8, &badf, NULL) == FDH_ERR_INVALID);
  OK(fdh_has_image(c, 8, &has));
  CHECK(!has);
  CHECK(fdh_put_video_alpha(c, 8, NULL, NULL) == FDH_ERR_INVALID);
  /* ... and it has no frame to hand out */
  OK(fdh_begin_frame(c, 16, 9, 1, black));
  OK(fdh_end_frame(c));
  t.rect[0] = 0; t.rect[1] = 0; t.rect[2] = 0; t.rect[3] = 0;
  CHECK(fdh_read_video_alpha(c, &t) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "read_video_alpha: ") == fdh_last_error());
  CHECK(fdh_read_video_alpha(NULL, &t) == FDH_ERR_INVALID);
  fdh_destroy(c);
  printf("video_alpha_abi_smoke: OK\n");
  return 0;
}
