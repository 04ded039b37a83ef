/* readback_abi_smoke.c -- every entry point include/figdraw_hip_readback.h declares, called from C99.
 *
 * Test infrastructure (tests/test_damage_readback.py compiles it with the flags of tests/abi_smoke.c and runs it in the CPU suite) on a
 * FDH_CREATE_RECORD_ONLY context: the mode is refused there (nothing is composited), turning it off is accepted, the reads fail with
 * FDH_ERR_NO_DEVICE, and the host-only fdh_apply_damage gives known answers on a small image.
 * usage: readback_abi_smoke */
#include <stdio.h>
#include <string.h>

#include "figdraw_hip_readback.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("readback_abi_smoke: FAILED %s:%d: %s   (last error: %s)\n", __FILE__, __LINE__, #cond, fdh_last_error()); failures++; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

enum { W = 70, H = 66, PITCH = 4 * W + 12 };  /* a 2 x 2 grid: the last column is 6 pixels wide, the last row 2 high */
static uint8_t image[H * PITCH], before[H * PITCH], slots[2 * FDH_TILE_BYTES];

int main(void) {
  FdhContext* c = NULL;
  const FdhDamageTile* tiles = NULL;
  const uint8_t* pixels = NULL;
  int n = -1, fw = -1, fh = -1, full = -1, x, y, k;
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY | FDH_CREATE_SYNC_SUBMIT));
  CHECK(fdh_set_damage_readback(c, 1) == FDH_ERR_INVALID);
  OK(fdh_set_damage_readback(c, 0));
  CHECK(fdh_read_damage(c, &tiles, &pixels, &n, &fw, &fh, &full) == FDH_ERR_NO_DEVICE);
  CHECK(fdh_read_damage_into(c, image, PITCH, W, H, &n) == FDH_ERR_NO_DEVICE);
  OK(fdh_destroy(c));

  /* fdh_apply_damage: bins (1, 0) and (0, 1) of the grid; slot bytes past a tile's edge are 0xEE and must not arrive */
  {
    FdhDamageTile t[2] = {{64, 0, 6, 64}, {0, 64, 64, 2}};
    memset(image, 0xAB, sizeof image);
    memset(slots, 0xEE, sizeof slots);
    for (k = 0; k < 2; k++)
      for (y = 0; y < t[k].h; y++)
        for (x = 0; x < 4 * t[k].w; x++) slots[k * FDH_TILE_BYTES + y * FDH_TILE_PITCH + x] = (uint8_t)(1 + k * 100 + (y * 7 + x) % 90);
    OK(fdh_apply_damage(image, PITCH, W, H, t, slots, 2));
    for (y = 0; y < H; y++)
      for (x = 0; x < PITCH; x++) {
        uint8_t want = 0xAB;
        for (k = 0; k < 2; k++)
          if (y >= t[k].y && y < t[k].y + t[k].h && x >= 4 * t[k].x && x < 4 * (t[k].x + t[k].w))
            want = (uint8_t)(1 + k * 100 + ((y - t[k].y) * 7 + (x - 4 * t[k].x)) % 90);
        CHECK(image[y * PITCH + x] == want);
      }
    /* refusals leave the image as it is */
    memcpy(before, image, sizeof image);
    OK(fdh_apply_damage(NULL, PITCH, W, H, NULL, NULL, 0));
    CHECK(fdh_apply_damage(image, PITCH, W, H, t, slots, -1) == FDH_ERR_INVALID);
    CHECK(fdh_apply_damage(NULL, PITCH, W, H, t, slots, 2) == FDH_ERR_INVALID);
    CHECK(fdh_apply_damage(image, PITCH, W, H, NULL, slots, 2) == FDH_ERR_INVALID);
    CHECK(fdh_apply_damage(image, PITCH, W, H, t, NULL, 2) == FDH_ERR_INVALID);
    CHECK(fdh_apply_damage(image, 4 * W - 1, W, H, t, slots, 2) == FDH_ERR_INVALID);
    t[1].w = 65;
    CHECK(fdh_apply_damage(image, PITCH, W, H, t, slots, 2) == FDH_ERR_INVALID);
    t[1].w = 64; t[1].h = 3;  /* one row past the image */
    CHECK(fdh_apply_damage(image, PITCH, W, H, t, slots, 2) == FDH_ERR_INVALID);
    CHECK(memcmp(before, image, sizeof image) == 0);
  }
  if (failures) return 1;
  printf("readback_abi_smoke: OK\n");
  return 0;
}
