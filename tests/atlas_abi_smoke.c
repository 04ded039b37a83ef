/* Atlas compaction through the C ABI in C99 (include_glyphs/figdraw_hip_atlas.h), on a record-only context: no GPU needed.
 * tests/test_atlas_move_host.py compiles this with -std=c99 -Wall -Wextra -Werror -pedantic -I include_glyphs and runs it. */
#include "figdraw_hip_atlas.h"
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, fdh_last_error()); return 1; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

static uint8_t img[200 * 200 * 4];

int main(void) {
  FdhContext* c = NULL;
  FdhAtlasMoveStats st;
  FdhAtlasUsage u;
  int rect[4], now[4], has = 0, keep = 7, size = 0;
  memset(img, 200, sizeof img);
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY));
  OK(fdh_get_atlas_keep(c, &keep)); CHECK(keep == 0);                              /* off by default */
  OK(fdh_put_image(c, 1, 20, 10, img, rect));
  OK(fdh_put_image(c, 2, 30, 40, img, NULL));
  OK(fdh_put_image(c, 3, 30, 40, img, NULL));
  OK(fdh_image_rect(c, 1, now)); CHECK(memcmp(now, rect, sizeof now) == 0);
  CHECK(fdh_image_rect(c, 99, now) == FDH_ERR_INVALID);
  OK(fdh_remove_image(c, 2));
  OK(fdh_atlas_usage(c, &u));
  CHECK(u.size == 256 && u.entries == 2 && u.used_area == 20 * 10 + 30 * 40 && u.packed_area > u.used_area && u.rebuilds == 0 && u.compactions == 0);
  OK(fdh_compact_atlas(c, 0, &st));                                                /* key 3 (taller) first, then key 1 */
  CHECK(st.entries == 2 && st.size_before == 256 && st.size_after == 256 && st.packed_after < st.packed_before && st.launches == 0);
  OK(fdh_image_rect(c, 3, now)); CHECK(now[0] == 4 && now[1] == 4 && now[2] == 30 && now[3] == 40);
  OK(fdh_image_rect(c, 1, now)); CHECK(now[0] == 4 + 30 + 8 && now[1] == 4);
  OK(fdh_compact_atlas(c, 100, NULL));                                             /* rounded up to 128, no statistics wanted */
  OK(fdh_atlas_size(c, &size)); CHECK(size == 128);
  CHECK(fdh_compact_atlas(c, 32, &st) == FDH_ERR_ATLAS_FULL);                      /* 30 x 40 does not fit 32: nothing changes */
  OK(fdh_atlas_size(c, &size)); CHECK(size == 128);
  CHECK(fdh_compact_atlas(c, -1, NULL) == FDH_ERR_INVALID);
  CHECK(fdh_compact_atlas(c, 16385, NULL) == FDH_ERR_INVALID);
  CHECK(fdh_compact_atlas(NULL, 0, NULL) == FDH_ERR_INVALID);
  OK(fdh_atlas_usage(c, &u)); CHECK(u.compactions == 2 && u.size == 128 && u.entries == 2);
  /* keep mode: an image that does not fit leaves a larger atlas with every key in it */
  OK(fdh_set_atlas_keep(c, 1));
  OK(fdh_get_atlas_keep(c, &keep)); CHECK(keep == 1);
  OK(fdh_put_image(c, 4, 100, 100, img, rect));
  OK(fdh_atlas_size(c, &size)); CHECK(size == 256);
  OK(fdh_has_image(c, 1, &has)); CHECK(has);
  OK(fdh_has_image(c, 3, &has)); CHECK(has);
  OK(fdh_image_rect(c, 4, now)); CHECK(memcmp(now, rect, sizeof now) == 0);
  OK(fdh_atlas_usage(c, &u)); CHECK(u.compactions == 3 && u.rebuilds == 0);
  /* keep off: the growth of old */
  OK(fdh_set_atlas_keep(c, 0));
  OK(fdh_put_image(c, 5, 100, 100, img, NULL));
  OK(fdh_put_image(c, 6, 200, 200, img, NULL));
  OK(fdh_has_image(c, 1, &has)); CHECK(!has);
  OK(fdh_atlas_usage(c, &u)); CHECK(u.rebuilds == 1 && u.size == 512);
  CHECK(fdh_debug_read_atlas_level(c, 0, img, (int64_t)sizeof img) == FDH_ERR_NO_DEVICE);   /* a record-only context has no texels */
  CHECK(fdh_atlas_usage(c, NULL) == FDH_ERR_INVALID);
  fdh_destroy(c);
  printf("atlas_abi_smoke: OK\n");
  return 0;
}
