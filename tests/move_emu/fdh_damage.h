// tests/move_emu/fdh_damage.h -- the shim's side of the header of that name: the library's fdh_damage_move.h itself (and through it
// fdh_damage_read.h), both copied beside it
#pragma once
#include "fdh_damage_move.h"
