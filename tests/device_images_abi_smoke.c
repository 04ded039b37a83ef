/* fdh_put_images_device, fdh_update_images_device and fdh_image_batch_stats through the C ABI in C99 (include_glyphs/
 * figdraw_hip_device_images.h), on a record-only context: no GPU needed, and the sources are never read.  tests/test_device_images_host.py
 * compiles this with -std=c99 -Wall -Wextra -Werror -pedantic -I include_glyphs and runs it. */
#include "figdraw_hip_device_images.h"
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  static uint32_t texels[64 * 40];  /* stands for device memory: a record-only context touches none of it */
  FdhDeviceImage img[3];
  FdhImageBatchStats st;
  int64_t keys[3] = {11, 12, 13}, twice[3] = {11, 12, 11};
  int rects[3][4], has = 0, i;
  CHECK(sizeof(FdhDeviceImage) == 48 && fdh_sizeof_device_image() == 48);
  CHECK(sizeof(FdhImageBatchStats) == 32);
  memset(img, 0, sizeof img);
  memset(rects, 0xFF, sizeof rects);
  img[0].data = texels; img[0].width = 64; img[0].height = 40; img[0].pitch_bytes = 256;
  img[0].format = FDH_IMAGE_RGBA8; img[0].channels = 4; img[0].flags = FDH_IMAGE_STRAIGHT_ALPHA;
  img[1].data = texels; img[1].width = 16; img[1].height = 9; img[1].pitch_bytes = 64;
  img[1].format = FDH_IMAGE_PLANAR_F32; img[1].channels = 1;
  img[2].data = texels; img[2].width = 8; img[2].height = 2; img[2].pitch_bytes = 32; img[2].plane_bytes = 64;
  img[2].format = FDH_IMAGE_PLANAR_F16; img[2].channels = 3;
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  OK(fdh_put_images_device(c, keys, img, 0, NULL));   /* nothing */
  OK(fdh_put_images_device(c, keys, img, 3, rects));
  for (i = 0; i < 3; i++) {
    CHECK(rects[i][2] == img[i].width && rects[i][3] == img[i].height && rects[i][0] >= 0 && rects[i][1] >= 0);
    OK(fdh_has_image(c, keys[i], &has)); CHECK(has);
  }
  OK(fdh_image_batch_stats(c, &st));
  CHECK(st.images == 3 && st.written == 3 && st.dropped_by_growth == 0 && st.tiles == 4 + 1 + 1 && st.launches == 0 && st.reserved == 0);
  OK(fdh_update_images_device(c, keys, img, 3));
  OK(fdh_update_images_device(c, keys + 1, img + 1, 2));
  OK(fdh_image_batch_stats(c, &st));
  CHECK(st.images == 2 && st.written == 2);
  OK(fdh_put_images_device(c, keys, img, 3, NULL));   /* out_rects may be NULL */
  /* refusals, each before anything is placed or begun; the stats stay the last good batch's */
  CHECK(fdh_put_images_device(c, keys, img, -1, rects) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "put_images_device") != NULL);
  CHECK(fdh_put_images_device(c, NULL, img, 3, rects) == FDH_ERR_INVALID);
  CHECK(fdh_put_images_device(c, keys, NULL, 3, rects) == FDH_ERR_INVALID);
  CHECK(fdh_put_images_device(c, twice, img, 3, rects) == FDH_ERR_INVALID);
  CHECK(fdh_update_images_device(c, twice, img, 3) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "update_images_device") != NULL);
  img[2].width = 2049; img[2].pitch_bytes = 2 * 2049 + 2; img[2].plane_bytes = 2 * img[2].pitch_bytes;
  CHECK(fdh_put_images_device(c, keys, img, 3, rects) == FDH_ERR_INVALID);
  img[2].width = 8; img[2].pitch_bytes = 32; img[2].plane_bytes = 64; img[2].reserved = 1;
  CHECK(fdh_put_images_device(c, keys, img, 3, rects) == FDH_ERR_INVALID);
  img[2].reserved = 0;
  keys[2] = 77;
  CHECK(fdh_update_images_device(c, keys, img, 3) == FDH_ERR_INVALID);                /* an unknown key */
  CHECK(fdh_put_images_device(NULL, keys, img, 3, rects) == FDH_ERR_INVALID);
  CHECK(fdh_image_batch_stats(c, NULL) == FDH_ERR_INVALID);
  OK(fdh_has_image(c, 77, &has)); CHECK(!has);
  OK(fdh_image_batch_stats(c, &st));
  CHECK(st.images == 3 && st.written == 3);
  fdh_destroy(c);
  printf("device_images_abi_smoke: OK\n");
  return 0;
}
