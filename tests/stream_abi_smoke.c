/* stream_abi_smoke.c -- every entry point include/figdraw_hip_stream.h declares, called from C99.
 *
 * Test infrastructure (tests/test_damage_stream_host.py compiles it with the flags of tests/abi_smoke.c and runs it in the CPU suite) on a
 * FDH_CREATE_RECORD_ONLY context: the coded read fails with FDH_ERR_NO_DEVICE there, and the host-only fdh_decode_damage and
 * fdh_coded_damage_bound give known answers on a hand-built stream of four tiles, one per mode.
 * usage: stream_abi_smoke */
#include <stdio.h>
#include <string.h>

#include "figdraw_hip_stream.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("stream_abi_smoke: FAILED %s:%d: %s   (last error: %s)\n", __FILE__, __LINE__, #cond, fdh_last_error()); failures++; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

enum { W = 70, H = 66, PITCH = 4 * W + 12 };  /* a 2 x 2 grid: the last column is 6 pixels wide, the last row 2 high */
static uint8_t image[H * PITCH], before[H * PITCH], want[H * PITCH];
static uint32_t blob[(64 + 16 + 48) / 4]; /* PAL at 0 (36 bytes), RUNS at 64 (12 bytes), RAW at 80 (48 bytes) */

static void put(int x, int y, uint32_t c) {
  want[y * PITCH + 4 * x] = (uint8_t)c; want[y * PITCH + 4 * x + 1] = (uint8_t)(c >> 8);
  want[y * PITCH + 4 * x + 2] = (uint8_t)(c >> 16); want[y * PITCH + 4 * x + 3] = (uint8_t)(c >> 24);
}

int main(void) {
  FdhContext* c = NULL;
  const FdhCodedTile* tiles = NULL;
  const uint8_t* payload = NULL;
  int n = -1, fw = -1, fh = -1, full = -1, x, y, i;
  int64_t bytes = -1;
  FdhCodedTile t[4];
  CHECK(sizeof(FdhCodedTile) == 24);
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY | FDH_CREATE_SYNC_SUBMIT));
  CHECK(fdh_read_damage_coded(c, &tiles, &payload, &n, &bytes, &fw, &fh, &full) == FDH_ERR_NO_DEVICE);
  CHECK(fdh_read_damage_coded(NULL, &tiles, &payload, &n, &bytes, &fw, &fh, &full) == FDH_ERR_INVALID);
  OK(fdh_destroy(c));
  CHECK(fdh_coded_damage_bound(W, H) == 4 * 16384);
  CHECK(fdh_coded_damage_bound(3840, 2160) == (int64_t)60 * 34 * 16384);
  CHECK(fdh_coded_damage_bound(0, 10) == 0 && fdh_coded_damage_bound(10, -1) == 0);

  memset(t, 0, sizeof t);
  memset(image, 0xAB, sizeof image);
  memset(want, 0xAB, sizeof want);
  /* bin (0, 0), SOLID */
  t[0].x = 0; t[0].y = 0; t[0].w = 64; t[0].h = 64; t[0].mode = FDH_TILE_SOLID; t[0].solid = 0xFF102030u;
  for (y = 0; y < 64; y++) for (x = 0; x < 64; x++) put(x, y, 0xFF102030u);
  /* the top 16 rows of bin (1, 0), 6 x 16, PAL: three colours at two bits, pixel i has index i % 3; 4 * 3 + 4 * ceil(96 * 2 / 32) = 36 bytes */
  t[1].x = 64; t[1].y = 0; t[1].w = 6; t[1].h = 16; t[1].mode = FDH_TILE_PAL; t[1].bits = 2; t[1].n = 3; t[1].offset = 0; t[1].size = 36;
  blob[0] = 0x00000001u; blob[1] = 0x80000000u; blob[2] = 0xFFFFFFFFu; /* ascending as unsigned */
  for (i = 0; i < 96; i++) {
    blob[3 + (2 * i) / 32] |= (uint32_t)(i % 3) << ((2 * i) % 32);
    put(64 + i % 6, i / 6, blob[i % 3]);
  }
  /* bin (0, 1), 64 x 2, RUNS: 100 pixels of one colour (the run crosses the row end), then 28 of another; 4 * ceil(12 / 4) = 12 bytes */
  t[2].x = 0; t[2].y = 64; t[2].w = 64; t[2].h = 2; t[2].mode = FDH_TILE_RUNS; t[2].n = 2; t[2].offset = 64; t[2].size = 12;
  blob[16] = 0x11223344u; blob[17] = 0x55667788u; blob[18] = 99u | 27u << 16;
  for (i = 0; i < 128; i++) put(i % 64, 64 + i / 64, i < 100 ? 0x11223344u : 0x55667788u);
  /* bin (1, 1), 6 x 2, RAW: 48 bytes */
  t[3].x = 64; t[3].y = 64; t[3].w = 6; t[3].h = 2; t[3].mode = FDH_TILE_RAW; t[3].offset = 80; t[3].size = 48;
  for (i = 0; i < 12; i++) { blob[20 + i] = 0x01010101u * (uint32_t)(i + 1); put(64 + i % 6, 64 + i / 6, blob[20 + i]); }

  OK(fdh_decode_damage(image, PITCH, W, H, t, 4, (const uint8_t*)blob, (int64_t)sizeof blob));
  CHECK(memcmp(image, want, sizeof image) == 0);
  /* refusals leave the image as it is */
  memset(image, 0xCD, sizeof image);
  memcpy(before, image, sizeof image);
  OK(fdh_decode_damage(NULL, PITCH, W, H, NULL, 0, NULL, 0));
  CHECK(fdh_decode_damage(image, PITCH, W, H, t, -1, (const uint8_t*)blob, (int64_t)sizeof blob) == FDH_ERR_INVALID);
  CHECK(fdh_decode_damage(NULL, PITCH, W, H, t, 4, (const uint8_t*)blob, (int64_t)sizeof blob) == FDH_ERR_INVALID);
  CHECK(fdh_decode_damage(image, PITCH, W, H, NULL, 4, (const uint8_t*)blob, (int64_t)sizeof blob) == FDH_ERR_INVALID);
  CHECK(fdh_decode_damage(image, PITCH, W, H, t, 4, NULL, (int64_t)sizeof blob) == FDH_ERR_INVALID);
  CHECK(fdh_decode_damage(image, PITCH, W, H, t, 4, (const uint8_t*)blob, (int64_t)sizeof blob - 1) == FDH_ERR_INVALID); /* RAW is cut short */
  CHECK(fdh_decode_damage(image, 4 * W - 1, W, H, t, 4, (const uint8_t*)blob, (int64_t)sizeof blob) == FDH_ERR_INVALID);
  t[3].mode = 4;
  CHECK(fdh_decode_damage(image, PITCH, W, H, t, 4, (const uint8_t*)blob, (int64_t)sizeof blob) == FDH_ERR_INVALID);
  t[3].mode = FDH_TILE_RAW; t[3].h = 3; t[3].size = 72; /* one row past the image */
  CHECK(fdh_decode_damage(image, PITCH, W, H, t, 4, (const uint8_t*)blob, (int64_t)sizeof blob) == FDH_ERR_INVALID);
  t[3].h = 2; t[3].size = 48; blob[18] = 99u | 28u << 16; /* the runs sum to 129 */
  CHECK(fdh_decode_damage(image, PITCH, W, H, t, 4, (const uint8_t*)blob, (int64_t)sizeof blob) == FDH_ERR_INVALID);
  blob[18] = 99u | 27u << 16; blob[3] |= 3u; /* index 3 of a palette of 3 */
  CHECK(fdh_decode_damage(image, PITCH, W, H, t, 4, (const uint8_t*)blob, (int64_t)sizeof blob) == FDH_ERR_INVALID);
  CHECK(memcmp(before, image, sizeof image) == 0);
  if (failures) return 1;
  printf("stream_abi_smoke: OK\n");
  return 0;
}
