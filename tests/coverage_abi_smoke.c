/* The coverage batch through the C ABI in C99 (include_glyphs/figdraw_hip_coverage.h), on a record-only context: no GPU needed.
 * tests/test_coverage_batch_host.py compiles this with -std=c99 -Wall -Wextra -Werror -pedantic -I include_glyphs and runs it. */
#include "figdraw_hip_coverage.h"
#include <math.h>
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  const float n = (float)NAN;
  float square[4 * 6] = {2, 2, 0, 0, 10, 2,   10, 2, 0, 0, 10, 9,   10, 9, 0, 0, 2, 9,   2, 9, 0, 0, 2, 2};
  float arch[2 * 6] = {1, 6, 5, -2, 9, 6,   9, 6, 0, 0, 1, 6};
  FdhGlyphOutline g[3];
  FdhGlyphBatchStats st;
  int rects[3][4], single[4], i;
  for (i = 0; i < 4; i++) square[6 * i + 2] = square[6 * i + 3] = n;
  arch[8] = arch[9] = n;
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  OK(fdh_glyph_coverage_batch_stats(c, &st));
  CHECK(st.glyphs == 0 && st.launches == 0);
  memset(g, 0, sizeof g);
  g[0].key = 1; g[0].segs = square; g[0].n_segs = 4; g[0].width = 12; g[0].height = 11;
  g[1].key = 2; g[1].segs = arch; g[1].n_segs = 2; g[1].width = 10; g[1].height = 8;
  g[2].key = 3; g[2].segs = NULL; g[2].n_segs = 0; g[2].width = 1; g[2].height = 9;
  OK(fdh_put_glyph_coverage_batch(c, g, 3, FDH_GLYPH_LCD_FILTER, rects));
  CHECK(rects[0][2] == 12 && rects[0][3] == 11 && rects[1][2] == 10 && rects[1][3] == 8 && rects[2][2] == 1 && rects[2][3] == 9);
  for (i = 0; i < 3; i++) { int has = 0; OK(fdh_has_image(c, g[i].key, &has)); CHECK(has); }
  OK(fdh_glyph_coverage_batch_stats(c, &st));
  CHECK(st.glyphs == 3 && st.written == 3 && st.dropped_by_growth == 0 && st.launches == 0 && st.bytes_copied == 0);
  /* the same packing as single calls: a second context */
  { FdhContext* d = NULL;
    OK(fdh_create(&d, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
    for (i = 0; i < 3; i++) {
      OK(fdh_put_glyph_outline(d, g[i].key, g[i].width, g[i].height, g[i].segs, g[i].n_segs, FDH_GLYPH_LCD_FILTER, single));
      CHECK(memcmp(single, rects[i], sizeof single) == 0);
    }
    fdh_destroy(d); }
  /* refusals: nothing is placed, the figures stay */
  CHECK(fdh_put_glyph_coverage_batch(c, g, 3, FDH_GLYPH_MTSDF, rects) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "put_glyph_coverage_batch") != NULL);
  CHECK(fdh_put_glyph_coverage_batch(c, g, 3, FDH_GLYPH_SDF_RANGE(4), rects) == FDH_ERR_INVALID);
  g[1].sdf_range = 4;
  CHECK(fdh_put_glyph_coverage_batch(c, g, 3, 0, rects) == FDH_ERR_INVALID);
  g[1].sdf_range = 0;
  CHECK(fdh_put_glyph_coverage_batch(c, NULL, 3, 0, rects) == FDH_ERR_INVALID);
  OK(fdh_glyph_coverage_batch_stats(c, &st));
  CHECK(st.glyphs == 3);
  OK(fdh_put_glyph_coverage_batch(c, g, 3, FDH_GLYPH_LCD_CONTEXT, NULL)); /* no rectangles wanted */
  OK(fdh_put_glyph_coverage_batch(c, NULL, 0, 0, NULL));
  OK(fdh_glyph_coverage_batch_stats(c, &st));
  CHECK(st.glyphs == 0);
  CHECK(fdh_put_glyph_coverage_batch(NULL, g, 3, 0, rects) == FDH_ERR_INVALID);
  CHECK(fdh_glyph_coverage_batch_stats(c, NULL) == FDH_ERR_INVALID);
  CHECK(fdh_glyph_coverage_batch_stats(NULL, &st) == FDH_ERR_INVALID);
  fdh_destroy(c);
  printf("coverage_abi_smoke: OK\n");
  return 0;
}
