/* moves_abi_smoke.c -- every entry point include_readback/figdraw_hip_moves.h declares, called from C99.
 *
 * Test infrastructure (tests/test_damage_moves_host.py compiles it with the flags of tests/abi_smoke.c and runs it in the CPU suite) on a
 * FDH_CREATE_RECORD_ONLY context: the read and the mover answer FDH_ERR_NO_DEVICE there; the decoder needs no context and decodes a
 * two-tile stream by hand, a COPY whose source is the tile a SOLID of the same stream overwrites.
 * usage: moves_abi_smoke */
#include <stdio.h>
#include <string.h>

#include "figdraw_hip_moves.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("moves_abi_smoke: FAILED %s:%d: %s   (last error: %s)\n", __FILE__, __LINE__, #cond, fdh_last_error()); failures++; } } while (0)
#define OK(call) CHECK((call) == FDH_OK)

int main(void) {
  FdhContext* c = NULL;
  FdhDamageMove moves[FDH_DAMAGE_MOVES_MAX], found[4];
  const FdhCodedTile* tiles = NULL;
  const uint8_t* payload = NULL;
  int n_tiles = -7, w = -7, h = -7, full = -7, n_copied = -7, n_out = -7, votes[4], i;
  int64_t bytes = -7;
  static uint32_t image[2 * 8]; /* 8 x 2 pixels: two tiles of 4 x 2 */
  FdhCodedTile stream[2];
  memset(moves, 0, sizeof moves);
  moves[0].dy = -17;
  OK(fdh_create(&c, 256, 1.0f, 0, FDH_CREATE_RECORD_ONLY | FDH_CREATE_SYNC_SUBMIT));
  CHECK(fdh_read_damage_moved(c, moves, 1, &tiles, &payload, &n_tiles, &bytes, &w, &h, &full, &n_copied) == FDH_ERR_NO_DEVICE);
  CHECK(strstr(fdh_last_error(), "fdh_read_damage_moved") != NULL);
  CHECK(n_tiles == -7 && bytes == -7 && n_copied == -7 && tiles == NULL); /* a refused call writes nothing */
  CHECK(fdh_find_damage_moves(c, FDH_DAMAGE_SHIFT_MAX, found, votes, 4, &n_out) == FDH_ERR_NO_DEVICE);
  CHECK(strstr(fdh_last_error(), "fdh_find_damage_moves") != NULL);
  CHECK(n_out == -7);
  CHECK(fdh_read_damage_moved(NULL, moves, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == FDH_ERR_INVALID);
  CHECK(fdh_find_damage_moves(NULL, 8, found, votes, 4, &n_out) == FDH_ERR_INVALID);
  OK(fdh_destroy(c));
  /* the decoder: tile 0 becomes one colour, tile 1 becomes what tile 0 held before this stream */
  for (i = 0; i < 16; i++) image[i] = 100u + (uint32_t)i;
  memset(stream, 0, sizeof stream);
  stream[0].w = stream[1].w = 4; stream[0].h = stream[1].h = 2;
  stream[0].mode = FDH_TILE_SOLID; stream[0].solid = 0xFF0000FFu;
  stream[1].x = 4; stream[1].mode = FDH_TILE_COPY; stream[1].solid = (uint32_t)(uint16_t)(int16_t)-4; /* dx = -4, dy = 0 */
  CHECK(fdh_decode_damage((uint8_t*)image, 32, 8, 2, stream, 2, NULL, 0) == FDH_ERR_INVALID); /* version 1 knows no mode 4 */
  CHECK(image[0] == 100u && image[15] == 115u);
  OK(fdh_decode_damage_moved((uint8_t*)image, 32, 8, 2, stream, 2, NULL, 0));
  for (i = 0; i < 16; i++) CHECK(image[i] == ((i & 7) < 4 ? 0xFF0000FFu : 100u + (uint32_t)i - 4u));
  stream[1].solid = (uint32_t)(uint16_t)(int16_t)-5; /* the source leaves the image */
  CHECK(fdh_decode_damage_moved((uint8_t*)image, 32, 8, 2, stream, 2, NULL, 0) == FDH_ERR_INVALID);
  CHECK(strstr(fdh_last_error(), "fdh_decode_damage_moved") != NULL);
  if (failures) return 1;
  printf("moves_abi_smoke: OK\n");
  return 0;
}
