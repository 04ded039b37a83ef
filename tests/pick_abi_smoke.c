/* pick_abi_smoke.c -- every entry point include/figdraw_hip_pick.h declares, called from C99.
 *
 * Test infrastructure (tests/test_pick_host.py compiles it with the flags of tests/abi_smoke.c and runs it in the CPU suite) on a
 * FDH_CREATE_RECORD_ONLY context: picking and tags work there (the tag table is host memory), the pixel queries fail with
 * FDH_ERR_NO_DEVICE, and the tag table of a frame rendered with picking off is refused.
 * usage: pick_abi_smoke */
#include <stdio.h>
#include <string.h>

#include "figdraw_hip_pick.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("pick_abi_smoke: FAILED %s:%d: %s   (last error: %s)\n", __FILE__, __LINE__, #cond, fdh_last_error()); failures++; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  const float clear[4] = {1, 1, 1, 1}, r0[4] = {0, 0, 32, 32}, r1[4] = {8, 8, 8, 8};
  const FdhColor red = {255, 0, 0, 255};
  int32_t z[4], id[4], region[4];
  int n = -1, counts[2] = {-1, -1};
  const float xy[4] = {10.0f, 10.0f, 100.0f, 100.0f};
  FdhPickHit hits[2];
  CHECK(sizeof(FdhPickHit) == 16);
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY | FDH_CREATE_SYNC_SUBMIT));
  /* before any frame, and for a frame rendered with picking off: no tag table */
  CHECK(fdh_pick_draw_tags(c, z, id, 4, &n) == FDH_ERR_INVALID);
  OK(fdh_begin_frame(c, 64, 64, 1, clear));
  OK(fdh_draw_rect(c, r0, red));
  OK(fdh_end_frame(c));
  CHECK(fdh_pick_draw_tags(c, z, id, 4, &n) == FDH_ERR_INVALID);
  /* picking on: the tag of each call's record; begin_frame resets the tag to (-1, -1) */
  OK(fdh_set_pick(c, 1));
  OK(fdh_set_pick_tag(c, 5, 6));
  OK(fdh_begin_frame(c, 64, 64, 1, clear));
  OK(fdh_draw_rect(c, r0, red));
  OK(fdh_set_pick_tag(c, 2, 9));
  OK(fdh_draw_rect(c, r1, red));
  OK(fdh_end_frame(c));
  OK(fdh_pick_draw_tags(c, NULL, NULL, 0, &n));
  CHECK(n == 2);
  memset(z, 0, sizeof z);
  memset(id, 0, sizeof id);
  OK(fdh_pick_draw_tags(c, z, id, 4, &n));
  CHECK(n == 2 && z[0] == -1 && id[0] == -1 && z[1] == 2 && id[1] == 9);
  CHECK(fdh_pick_draw_tags(c, NULL, id, 4, &n) == FDH_ERR_INVALID);
  /* no pixels on a record-only context */
  CHECK(fdh_pick_points(c, xy, 2, 128, 0u, 1, hits, counts) == FDH_ERR_NO_DEVICE);
  CHECK(fdh_pick_region(c, 0, 0, 2, 2, 128, FDH_PICK_SHADOWS, region) == FDH_ERR_NO_DEVICE);
  /* bad arguments are refused before anything else */
  CHECK(fdh_pick_points(c, xy, 2, 128, 0u, 0, hits, counts) == FDH_ERR_INVALID);
  CHECK(fdh_pick_points(c, xy, 2, 128, 0u, FDH_PICK_MAX_HITS + 1, hits, counts) == FDH_ERR_INVALID);
  CHECK(fdh_pick_region(c, 0, 0, -1, 2, 128, 0u, region) == FDH_ERR_INVALID);
  /* turned off again: the next frame keeps no tags */
  OK(fdh_set_pick(c, 0));
  OK(fdh_begin_frame(c, 64, 64, 1, clear));
  OK(fdh_draw_rect(c, r0, red));
  OK(fdh_end_frame(c));
  CHECK(fdh_pick_draw_tags(c, z, id, 4, &n) == FDH_ERR_INVALID);
  OK(fdh_destroy(c));
  CHECK(fdh_set_pick(NULL, 1) == FDH_ERR_INVALID);
  if (failures) return 1;
  printf("pick_abi_smoke: OK\n");
  return 0;
}
