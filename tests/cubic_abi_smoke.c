/* fdh_put_glyph_outline_cubic through the C ABI in C99 (include_glyphs/figdraw_hip_cubic.h), on a record-only context: no GPU needed.
 * tests/test_msdf_cubic_host.py compiles this with -std=c99 -Wall -Wextra -Werror -pedantic -I include_glyphs and runs it. */
#include "figdraw_hip_cubic.h"
#include <math.h>
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  const float n = (float)NAN;
  /* a box whose top side is a cubic; the same box with a quadratic there, in both formats */
  float box[4 * 8] = {2, 4, 4, -2, 8, 8, 10, 4,   10, 4, 0, 0, 0, 0, 10, 9,   10, 9, 0, 0, 0, 0, 2, 9,   2, 9, 0, 0, 0, 0, 2, 4};
  float quad8[4 * 8], quad6[4 * 6];
  int rect[4], other[4], has = 0, i, k;
  for (i = 1; i < 4; i++) for (k = 2; k < 6; k++) box[8 * i + k] = n;
  memcpy(quad8, box, sizeof box);
  quad8[2] = 6; quad8[3] = 0; quad8[4] = quad8[5] = n;
  for (i = 0; i < 4; i++) {
    for (k = 0; k < 4; k++) quad6[6 * i + k] = quad8[8 * i + k];
    quad6[6 * i + 4] = quad8[8 * i + 6]; quad6[6 * i + 5] = quad8[8 * i + 7];
  }
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  OK(fdh_put_glyph_outline_cubic(c, 1, 12, 11, box, 4, FDH_GLYPH_MTSDF | FDH_GLYPH_SDF_RANGE(4) | FDH_GLYPH_MTSDF_CORRECT, rect));
  CHECK(rect[2] == 12 && rect[3] == 11 && rect[0] >= 0 && rect[1] >= 0);
  OK(fdh_has_image(c, 1, &has)); CHECK(has);
  OK(fdh_put_glyph_outline_cubic(c, 2, 12, 11, box, 4, 0, rect));                      /* coverage */
  OK(fdh_put_glyph_outline_cubic(c, 3, 12, 11, box, 4, FDH_GLYPH_LCD_FILTER, rect));
  OK(fdh_put_glyph_outline_cubic(c, 4, 12, 11, NULL, 0, FDH_GLYPH_MTSDF, rect));       /* no segments: no error */
  /* refusals, each before anything is packed */
  CHECK(fdh_put_glyph_outline_cubic(c, 9, 12, 11, box, 4, FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_OVERLAP, rect) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "put_glyph_outline_cubic") != NULL);
  CHECK(fdh_put_glyph_outline_cubic(c, 9, 12, 11, box, 3, FDH_GLYPH_MTSDF, rect) == FDH_ERR_INVALID);      /* an open contour */
  CHECK(fdh_put_glyph_outline_cubic(c, 9, 12, 11, box, 4, FDH_GLYPH_MTSDF | FDH_GLYPH_LCD_FILTER, rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_glyph_outline_cubic(c, 9, 12, 11, box, 4, FDH_GLYPH_SDF_RANGE(4), rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_glyph_outline_cubic(c, 9, 12, 11, box, 4, FDH_GLYPH_MTSDF | FDH_GLYPH_SDF_RANGE(65), rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_glyph_outline_cubic(c, 9, 0, 11, box, 4, FDH_GLYPH_MTSDF, rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_glyph_outline_cubic(c, 9, 12, 11, NULL, 4, FDH_GLYPH_MTSDF, rect) == FDH_ERR_INVALID);
  CHECK(fdh_put_glyph_outline_cubic(NULL, 9, 12, 11, box, 4, FDH_GLYPH_MTSDF, rect) == FDH_ERR_INVALID);
  OK(fdh_has_image(c, 9, &has)); CHECK(!has);
  /* without a cubic the call is fdh_put_glyph_outline: the same rectangle on a second context, FDH_GLYPH_MTSDF_OVERLAP allowed */
  { FdhContext* d = NULL;
    OK(fdh_create(&d, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
    OK(fdh_put_glyph_outline(d, 1, 12, 11, quad6, 4, FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_OVERLAP, other));
    fdh_destroy(d);
    OK(fdh_create(&d, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
    OK(fdh_put_glyph_outline_cubic(d, 1, 12, 11, quad8, 4, FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_OVERLAP, rect));
    CHECK(memcmp(rect, other, sizeof rect) == 0);
    fdh_destroy(d); }
  fdh_destroy(c);
  printf("cubic_abi_smoke: OK\n");
  return 0;
}
