// tests/emu/fdh_damage.h -- the host shims' side of the library's header of that name: the library's own fdh_damage_read.h and, where a test
// copied it beside this file, fdh_damage_move.h (the parameter blocks and the device code the damage kernels share)
#pragma once
#include "fdh_damage_read.h"
#if __has_include("fdh_damage_move.h")
#include "fdh_damage_move.h"
#endif
