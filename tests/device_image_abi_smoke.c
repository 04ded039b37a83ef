/* fdh_put_image_device and fdh_update_image_device through the C ABI in C99 (include_glyphs/figdraw_hip_device_image.h), on a record-only
 * context: no GPU needed, and the source is never read.  tests/test_device_image_host.py compiles this with -std=c99 -Wall -Wextra -Werror
 * -pedantic -I include_glyphs and runs it. */
#include "figdraw_hip_device_image.h"
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  static uint32_t texels[16 * 9];  /* stands for device memory: a record-only context touches none of it */
  FdhDeviceImage img, bad;
  int rect[4], has = 0;
  CHECK(sizeof(FdhDeviceImage) == 48);
  memset(&img, 0, sizeof img);
  img.data = texels; img.width = 16; img.height = 9; img.pitch_bytes = 64;
  img.format = FDH_IMAGE_RGBA8; img.channels = 4; img.flags = FDH_IMAGE_STRAIGHT_ALPHA;
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  OK(fdh_put_image_device(c, 1, &img, rect));
  CHECK(rect[2] == 16 && rect[3] == 9 && rect[0] >= 0 && rect[1] >= 0);
  OK(fdh_has_image(c, 1, &has)); CHECK(has);
  OK(fdh_update_image_device(c, 1, &img));
  bad = img; bad.format = FDH_IMAGE_PLANAR_F32; bad.channels = 1; bad.flags = 0;   /* 16 x 9 floats in one plane */
  OK(fdh_put_image_device(c, 2, &bad, NULL));
  bad.format = FDH_IMAGE_PLANAR_F16; bad.channels = 3; bad.pitch_bytes = 32; bad.plane_bytes = 32 * 9;
  bad.width = 8; bad.height = 2;                                                    /* three planes of 8 x 2 halves inside the array */
  OK(fdh_put_image_device(c, 3, &bad, rect));
  CHECK(rect[2] == 8 && rect[3] == 2);
  /* refusals, each before anything is placed */
  CHECK(fdh_put_image_device(c, 9, NULL, rect) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "put_image_device") != NULL);
  bad = img; bad.data = NULL;
  CHECK(fdh_put_image_device(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = img; bad.width = 0;
  CHECK(fdh_put_image_device(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = img; bad.format = 3;
  CHECK(fdh_put_image_device(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = img; bad.flags = 2;
  CHECK(fdh_put_image_device(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = img; bad.reserved = 1;
  CHECK(fdh_put_image_device(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = img; bad.channels = 3;
  CHECK(fdh_put_image_device(c, 9, &bad, rect) == FDH_ERR_INVALID);
  bad = img; bad.pitch_bytes = 60;
  CHECK(fdh_put_image_device(c, 9, &bad, rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_image_device(NULL, 9, &img, rect) == FDH_ERR_INVALID);
  CHECK(fdh_update_image_device(c, 77, &img) == FDH_ERR_INVALID);                  /* an unknown key */
  CHECK(strstr(fdh_last_error(), "update_image_device") != NULL);
  bad = img; bad.height = 8;
  CHECK(fdh_update_image_device(c, 1, &bad) == FDH_ERR_INVALID);                   /* not the entry's size */
  OK(fdh_has_image(c, 9, &has)); CHECK(!has);
  fdh_destroy(c);
  printf("device_image_abi_smoke: OK\n");
  return 0;
}
