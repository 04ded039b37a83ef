/* The two cubic batches through the C ABI in C99 (include_glyphs/figdraw_hip_cubic_batch.h), on a record-only context: no GPU needed.
 * tests/test_msdf_cubic_batch_host.py compiles this with -std=c99 -Wall -Wextra -Werror -pedantic -I include_glyphs and runs it. */
#include "figdraw_hip_cubic_batch.h"
#include <math.h>
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  const float n = (float)NAN;
  /* a box whose top side is a cubic; a triangle of lines */
  float box[4 * 8] = {2, 4, 4, -2, 8, 8, 10, 4,   10, 4, 0, 0, 0, 0, 10, 9,   10, 9, 0, 0, 0, 0, 2, 9,   2, 9, 0, 0, 0, 0, 2, 4};
  float tri[3 * 8] = {2, 2, 0, 0, 0, 0, 10, 2,   10, 2, 0, 0, 0, 0, 6, 9,   6, 9, 0, 0, 0, 0, 2, 2};
  FdhGlyphOutline g[3];
  FdhGlyphBatchStats st;
  int rects[3][4], single[4], i, k;
  for (i = 1; i < 4; i++) for (k = 2; k < 6; k++) box[8 * i + k] = n;
  for (i = 0; i < 3; i++) for (k = 2; k < 6; k++) tri[8 * i + k] = n;
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  memset(g, 0, sizeof g);
  g[0].key = 1; g[0].segs = box; g[0].n_segs = 4; g[0].width = 12; g[0].height = 11; g[0].sdf_range = 2;
  g[1].key = 2; g[1].segs = tri; g[1].n_segs = 3; g[1].width = 12; g[1].height = 11;
  g[2].key = 3; g[2].segs = NULL; g[2].n_segs = 0; g[2].width = 1; g[2].height = 9;
  /* distance fields */
  OK(fdh_put_glyph_outlines_cubic(c, g, 3, FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT | FDH_GLYPH_SDF_RANGE(8), rects));
  CHECK(rects[0][2] == 12 && rects[0][3] == 11 && rects[1][2] == 12 && rects[1][3] == 11 && rects[2][2] == 1 && rects[2][3] == 9);
  for (i = 0; i < 3; i++) { int has = 0; OK(fdh_has_image(c, g[i].key, &has)); CHECK(has); }
  OK(fdh_glyph_batch_stats(c, &st));
  CHECK(st.glyphs == 3 && st.written == 3 && st.dropped_by_growth == 0 && st.launches == 0 && st.bytes_copied == 0);
  { FdhContext* d = NULL;  /* the same packing as single calls: a second context */
    OK(fdh_create(&d, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
    for (i = 0; i < 3; i++) {
      OK(fdh_put_glyph_outline_cubic(d, g[i].key, g[i].width, g[i].height, g[i].segs, g[i].n_segs, FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT, single));
      CHECK(memcmp(single, rects[i], sizeof single) == 0);
    }
    fdh_destroy(d); }
  CHECK(fdh_put_glyph_outlines_cubic(c, g, 3, FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_OVERLAP, rects) == FDH_ERR_INVALID); /* a cubic in glyph 0 */
  CHECK(strstr(fdh_last_error(), "put_glyph_outlines_cubic") != NULL);
  OK(fdh_put_glyph_outlines_cubic(c, g + 1, 2, FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_OVERLAP, NULL));                    /* none: fdh_put_glyph_outlines */
  CHECK(fdh_put_glyph_outlines_cubic(c, g, 3, FDH_GLYPH_MTSDF | FDH_GLYPH_LCD_FILTER, rects) == FDH_ERR_INVALID);
  CHECK(fdh_put_glyph_outlines_cubic(c, NULL, 3, FDH_GLYPH_MTSDF, rects) == FDH_ERR_INVALID);
  CHECK(fdh_put_glyph_outlines_cubic(NULL, g, 3, FDH_GLYPH_MTSDF, rects) == FDH_ERR_INVALID);
  OK(fdh_glyph_batch_stats(c, &st));
  CHECK(st.glyphs == 2);
  OK(fdh_put_glyph_outlines_cubic(c, NULL, 0, FDH_GLYPH_MTSDF, NULL));
  OK(fdh_glyph_batch_stats(c, &st));
  CHECK(st.glyphs == 0);
  /* coverage */
  g[0].sdf_range = 0;
  OK(fdh_glyph_coverage_batch_stats(c, &st));
  CHECK(st.glyphs == 0 && st.launches == 0);
  OK(fdh_put_glyph_coverage_batch_cubic(c, g, 3, FDH_GLYPH_LCD_FILTER, rects));
  CHECK(rects[0][2] == 12 && rects[0][3] == 11 && rects[2][2] == 1 && rects[2][3] == 9);
  OK(fdh_glyph_coverage_batch_stats(c, &st));
  CHECK(st.glyphs == 3 && st.written == 3 && st.launches == 0 && st.bytes_copied == 0);
  CHECK(fdh_put_glyph_coverage_batch_cubic(c, g, 3, FDH_GLYPH_MTSDF, rects) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "put_glyph_coverage_batch_cubic") != NULL);
  g[1].sdf_range = 4;
  CHECK(fdh_put_glyph_coverage_batch_cubic(c, g, 3, 0, rects) == FDH_ERR_INVALID);
  g[1].sdf_range = 0;
  OK(fdh_glyph_coverage_batch_stats(c, &st));
  CHECK(st.glyphs == 3);
  OK(fdh_put_glyph_coverage_batch_cubic(c, g, 3, FDH_GLYPH_LCD_CONTEXT, NULL));
  OK(fdh_put_glyph_coverage_batch_cubic(c, NULL, 0, 0, NULL));
  OK(fdh_glyph_coverage_batch_stats(c, &st));
  CHECK(st.glyphs == 0);
  fdh_destroy(c);
  printf("cubic_batch_abi_smoke: OK\n");
  return 0;
}
