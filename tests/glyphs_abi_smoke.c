/* glyphs_abi_smoke.c -- every entry point include_glyphs/figdraw_hip_glyphs.h declares, called from C99.
 *
 * Test infrastructure (tests/test_msdf_batch_host.py compiles it with the flags of tests/abi_smoke.c and runs it in the CPU suite) on a
 * FDH_CREATE_RECORD_ONLY context: a batch of three squares is packed where three single calls pack them, a batch with an open contour in
 * the middle is refused whole, and the stats are those of the last batch that was accepted.
 * usage: glyphs_abi_smoke */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "figdraw_hip_glyphs.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("glyphs_abi_smoke: FAILED %s:%d: %s   (last error: %s)\n", __FILE__, __LINE__, #cond, fdh_last_error()); failures++; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext *c = NULL, *d = NULL;
  float sq[4][6] = {{2, 2, 0, 0, 10, 2}, {10, 2, 0, 0, 10, 9}, {10, 9, 0, 0, 2, 9}, {2, 9, 0, 0, 2, 2}};
  FdhGlyphOutline g[3];
  FdhGlyphBatchStats st;
  int rects[3][4], single[4], i, k, has = -7;
  int64_t area = 0, area_single = 0;
  for (i = 0; i < 4; i++) sq[i][2] = sq[i][3] = (float)NAN;
  CHECK(fdh_sizeof_glyph_outline() == (int)sizeof(FdhGlyphOutline));
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY | FDH_CREATE_SYNC_SUBMIT));
  OK(fdh_create(&d, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY | FDH_CREATE_SYNC_SUBMIT));
  memset(&st, 0xFF, sizeof st);
  OK(fdh_glyph_batch_stats(c, &st));
  CHECK(st.glyphs == 0 && st.launches == 0 && st.bytes_copied == 0); /* before the first batch */
  for (i = 0; i < 3; i++) {
    g[i].key = 100 + i; g[i].segs = &sq[0][0]; g[i].n_segs = 4; g[i].width = 12 + i; g[i].height = 11; g[i].sdf_range = i == 1 ? 2u : 0u;
  }
  OK(fdh_put_glyph_outlines(c, g, 3, FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT | FDH_GLYPH_SDF_RANGE(8), rects));
  for (i = 0; i < 3; i++) {
    OK(fdh_put_glyph_outline(d, 100 + i, 12 + i, 11, &sq[0][0], 4, FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT | FDH_GLYPH_SDF_RANGE(8), single));
    for (k = 0; k < 4; k++) CHECK(rects[i][k] == single[k]);
    OK(fdh_has_image(c, 100 + i, &has));
    CHECK(has == 1);
  }
  OK(fdh_atlas_packed_area(c, &area));
  OK(fdh_atlas_packed_area(d, &area_single));
  CHECK(area == area_single && area > 0);
  OK(fdh_glyph_batch_stats(c, &st));
  CHECK(st.glyphs == 3 && st.written == 3 && st.dropped_by_growth == 0 && st.launches == 0 && st.bytes_copied == 0);
  /* an open contour in the middle: nothing of the batch is placed */
  for (i = 0; i < 3; i++) g[i].key = 200 + i;
  g[1].n_segs = 3;
  CHECK(fdh_put_glyph_outlines(c, g, 3, FDH_GLYPH_MTSDF, rects) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "put_glyph_outlines") != NULL);
  OK(fdh_has_image(c, 200, &has));
  CHECK(has == 0);
  OK(fdh_atlas_packed_area(c, &area));
  CHECK(area == area_single);
  g[1].n_segs = 4;
  CHECK(fdh_put_glyph_outlines(c, g, 3, FDH_GLYPH_MTSDF | FDH_GLYPH_LCD_FILTER, rects) == FDH_ERR_INVALID);
  CHECK(fdh_put_glyph_outlines(c, g, 3, FDH_GLYPH_MTSDF_CORRECT, rects) == FDH_ERR_INVALID);
  CHECK(fdh_put_glyph_outlines(c, NULL, 3, FDH_GLYPH_MTSDF, rects) == FDH_ERR_INVALID);
  OK(fdh_put_glyph_outlines(c, NULL, 0, FDH_GLYPH_MTSDF, NULL));
  OK(fdh_put_glyph_outlines(c, g, 3, FDH_GLYPH_MTSDF, NULL)); /* no rectangles wanted */
  OK(fdh_has_image(c, 202, &has));
  CHECK(has == 1);
  CHECK(fdh_put_glyph_outlines(NULL, g, 3, FDH_GLYPH_MTSDF, rects) == FDH_ERR_INVALID);
  CHECK(fdh_glyph_batch_stats(c, NULL) == FDH_ERR_INVALID);
  CHECK(fdh_glyph_batch_stats(NULL, &st) == FDH_ERR_INVALID);
  OK(fdh_destroy(c));
  OK(fdh_destroy(d));
  if (failures) return 1;
  printf("glyphs_abi_smoke: OK\n");
  return 0;
}
