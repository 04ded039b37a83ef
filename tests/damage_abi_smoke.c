/* damage_abi_smoke.c -- every entry point include/figdraw_hip_damage.h declares, called from C99.
 *
 * Test infrastructure (tests/test_damage.py compiles it with the flags of tests/abi_smoke.c and runs it in the CPU suite) on a
 * FDH_CREATE_RECORD_ONLY context: the mode is refused there (nothing is composited), turning it off is accepted, the bin queries
 * fail with FDH_ERR_NO_DEVICE, and the host-only blur rule gives known answers.
 * usage: damage_abi_smoke */
#include <stdio.h>
#include <string.h>

#include "figdraw_hip_damage.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("damage_abi_smoke: FAILED %s:%d: %s   (last error: %s)\n", __FILE__, __LINE__, #cond, fdh_last_error()); failures++; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  uint8_t mask[64];
  int bx = -1, by = -1, n = -1, x, y;
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY | FDH_CREATE_SYNC_SUBMIT));
  CHECK(fdh_set_damage_tracking(c, 1) == FDH_ERR_INVALID);
  OK(fdh_set_damage_tracking(c, 0));
  CHECK(fdh_damage_bins(c, mask, (int)sizeof mask, &bx, &by, &n) == FDH_ERR_NO_DEVICE);
  CHECK(fdh_damage_changed_bins(c, mask, (int)sizeof mask, &bx, &by, &n) == FDH_ERR_NO_DEVICE);
  OK(fdh_destroy(c));

  /* the blur rule on an 8 x 8 grid: bin (1, 1) changed; a node over pixels [256, 320) x [256, 320) with radius 4 does not reach it ... */
  {
    uint8_t changed[64], out[64];
    int rect[4] = {256, 256, 320, 320};
    float radius = 4.0f;
    memset(changed, 0, sizeof changed);
    changed[1 * 8 + 1] = 1;
    OK(fdh_damage_closure(changed, 8, 8, rect, &radius, 1, out));
    n = 0;
    for (x = 0; x < 64; x++) n += out[x];
    CHECK(n == 1 && out[9] == 1);
    /* ... a change inside its reach turns the bin-rounded footprint + reach (bins 3..5 on both axes) into damage */
    changed[4 * 8 + 3] = 1;
    OK(fdh_damage_closure(changed, 8, 8, rect, &radius, 1, out));
    for (y = 0; y < 8; y++)
      for (x = 0; x < 8; x++) CHECK(out[y * 8 + x] == ((x >= 3 && x <= 5 && y >= 3 && y <= 5) || (x == 1 && y == 1)));
    /* no nodes: the changed bins themselves; bad arguments refused */
    OK(fdh_damage_closure(changed, 8, 8, NULL, NULL, 0, out));
    CHECK(memcmp(changed, out, sizeof out) == 0);
    CHECK(fdh_damage_closure(changed, 8, 8, NULL, NULL, 1, out) == FDH_ERR_INVALID);
    CHECK(fdh_damage_closure(NULL, 8, 8, NULL, NULL, 0, out) == FDH_ERR_INVALID);
  }
  if (failures) return 1;
  printf("damage_abi_smoke: OK\n");
  return 0;
}
