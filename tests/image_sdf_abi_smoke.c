/* fdh_put_image_sdf and fdh_put_image_sdf_of through the C ABI in C99 (include_glyphs/figdraw_hip_image_sdf.h), on a record-only context: no
 * GPU needed.  tests/test_image_sdf_host.py compiles this with -std=c99 -Wall -Wextra -Werror -pedantic -I include_glyphs and runs it. */
#include "figdraw_hip_image_sdf.h"
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  uint8_t img[7 * 5 * 4];
  int rect[4], other[4], has = 0;
  size_t i;
  for (i = 0; i < sizeof img; i++) img[i] = (uint8_t)(i * 37u);
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  OK(fdh_put_image_sdf(c, 1, 7, 5, img, 3, 4, FDH_GLYPH_SDF_RANGE(8), rect));
  CHECK(rect[2] == 7 + 8 && rect[3] == 5 + 8 && rect[0] >= 0 && rect[1] >= 0);
  OK(fdh_has_image(c, 1, &has)); CHECK(has);
  OK(fdh_put_image_sdf(c, 2, 7, 5, img, 0, 0, 0, NULL));                          /* no pad, the default range, no out_rect */
  OK(fdh_put_image_sdf_of(c, 1, 3, 3, 2, FDH_GLYPH_SDF_RANGE(64), other));        /* the field of a field */
  CHECK(other[2] == rect[2] + 4 && other[3] == rect[3] + 4);
  OK(fdh_has_image(c, 1, &has)); CHECK(has);
  /* refusals, each before anything is packed */
  CHECK(fdh_put_image_sdf(c, 9, 0, 5, img, 3, 0, 0, rect) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "put_image_sdf") != NULL);
  CHECK(fdh_put_image_sdf(c, 9, 7, 5, NULL, 3, 0, 0, rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_image_sdf(c, 9, 7, 5, img, 4, 0, 0, rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_image_sdf(c, 9, 7, 5, img, 3, 65, 0, rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_image_sdf(c, 9, 7, 5, img, 3, 0, FDH_GLYPH_MTSDF, rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_image_sdf(c, 9, 7, 5, img, 3, 0, FDH_GLYPH_SDF_RANGE(65), rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_image_sdf(NULL, 9, 7, 5, img, 3, 0, 0, rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_image_sdf_of(c, 77, 9, 3, 0, 0, rect) == FDH_ERR_INVALID);        /* an unknown source */
  CHECK(strstr(fdh_last_error(), "put_image_sdf_of") != NULL);
  CHECK(fdh_put_image_sdf_of(c, 1, 1, 3, 0, 0, rect) == FDH_ERR_INVALID);         /* the source's own key */
  CHECK(fdh_put_image_sdf_of(c, 1, 9, -1, 0, 0, rect) == FDH_ERR_INVALID);
  OK(fdh_has_image(c, 9, &has)); CHECK(!has);
  fdh_destroy(c);
  printf("image_sdf_abi_smoke: OK\n");
  return 0;
}
