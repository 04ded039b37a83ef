// fdh_plain.h -- the host side's vocabulary that needs no HIP header: the library's exception, the affine matrix, a record's pick tag, and
// what a run of records adds to its phase.  Compiles with a plain host compiler; fdh_retained.h builds on nothing else of the library's.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/figdraw_hip.h"
#include "fdh_types.h"

#if defined(__GNUC__)
#define FDH_ALWAYS_INLINE inline __attribute__((always_inline))
#else
#define FDH_ALWAYS_INLINE inline
#endif

namespace fdh {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// 2D affine part of the vmath Mat4 stack: [a c tx; b d ty]
struct Aff {
  float a = 1, b = 0, c = 0, d = 1, tx = 0, ty = 0;
};

inline bool bbox_empty(const BBox& b) { return b.x1 <= b.x0 || b.y1 <= b.y0; }
inline void bbox_union(BBox& a, const BBox& b) {
  if (bbox_empty(b)) return;
  if (bbox_empty(a)) { a = b; return; }
  a.x0 = std::min(a.x0, b.x0); a.y0 = std::min(a.y0, b.y0); a.x1 = std::max(a.x1, b.x1); a.y1 = std::max(a.y1, b.y1);
}

// Picking (include/figdraw_hip_pick.h): each record's tag, kept beside the records of its lane while the frame has picking on.
struct PickTag { int32_t z, id; };

// what a phase's draws ask of its compositor launch: a Phase has them, and so has the summary of every run of records that goes into one
struct PhaseFlags {
  bool has_masks = false; // clip / rect-mask ops present
  bool has_atlas = false; // axis-aligned atlas quads at >= 1:1 present (k_composite_tiles<2> unless has_slow)
  bool has_slow = false;  // some draw needs k_composite_tiles<true> (atlas / rotated quad / bezier / rect-mask setup)
  bool has_slow_atlas = false;  // ... and one of them is an atlas quad off the 4-wide path (rotated, or minified over mip levels): the 168-register form of that build
  bool has_rot = false;   // rotated / skewed SDF quads whose edge functions fit 32 bits (F_EDGE32): the 4-wide path of builds <8> and <3>
  FDH_ALWAYS_INLINE void merge_flags(const PhaseFlags& s) {
    has_masks = has_masks || s.has_masks;
    has_atlas = has_atlas || s.has_atlas;
    has_slow = has_slow || s.has_slow;
    has_slow_atlas = has_slow_atlas || s.has_slow_atlas;
    has_rot = has_rot || s.has_rot;
  }
};

// what a run of records adds to its phase (kept per parallel chunk by the walk pool's threads, merged by the calling thread)
struct PhaseSum : PhaseFlags {
  BBox u{0, 0, 0, 0};  // union of the records' final bounds
  int deepest = 0;     // deepest clip nesting reached, relative to the run's start
  int64_t frag_mode[4] = {0, 0, 0, 0}, frag_ellip = 0, frag_other = 0;  // covered fragments by SdfMode 3 / 7 / 9 / 12
  // a run that starts at clip depth `depth_base` of this one joins it (once per spliced root of a retained frame: left to itself the
  // compiler emits this out of line and calls it, which a retained frame's record time shows)
  FDH_ALWAYS_INLINE void merge(const PhaseSum& s, int depth_base) {
    merge_flags(s);
    bbox_union(u, s.u);
    deepest = std::max(deepest, depth_base + s.deepest);
    for (int k = 0; k < 4; k++) frag_mode[k] += s.frag_mode[k];
    frag_ellip += s.frag_ellip;
    frag_other += s.frag_other;
  }
};

}  // namespace fdh
