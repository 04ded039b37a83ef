/* exact_abi_smoke.c -- every entry point include/figdraw_hip_exact.h declares, called from C99.
 *
 * Test infrastructure (tests/test_damage_exact_host.py compiles it with the flags of tests/abi_smoke.c and runs it in the CPU suite) on a
 * FDH_CREATE_RECORD_ONLY context: turning the mode on is refused there, turning it off is accepted, and there are no stats of a read.
 * usage: exact_abi_smoke */
#include <stdio.h>
#include <string.h>

#include "figdraw_hip_exact.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("exact_abi_smoke: FAILED %s:%d: %s   (last error: %s)\n", __FILE__, __LINE__, #cond, fdh_last_error()); failures++; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  int pending = -7, changed = -7, fresh = -7;
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY | FDH_CREATE_SYNC_SUBMIT));
  CHECK(fdh_set_damage_exact(c, 1) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "fdh_set_damage_exact") != NULL);
  OK(fdh_set_damage_exact(c, 0));
  CHECK(fdh_damage_exact_stats(c, &pending, &changed, &fresh) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "fdh_damage_exact_stats") != NULL);
  CHECK(fdh_damage_exact_stats(c, NULL, NULL, NULL) == FDH_ERR_INVALID);
  CHECK(pending == -7 && changed == -7 && fresh == -7); /* a refused call writes nothing */
  CHECK(fdh_set_damage_exact(NULL, 1) == FDH_ERR_INVALID);
  CHECK(fdh_damage_exact_stats(NULL, &pending, &changed, &fresh) == FDH_ERR_INVALID);
  OK(fdh_destroy(c));
  if (failures) return 1;
  printf("exact_abi_smoke: OK\n");
  return 0;
}
