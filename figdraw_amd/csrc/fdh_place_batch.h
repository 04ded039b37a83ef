// fdh_place_batch.h -- what the host sources that put things into the atlas share and nobody else sees: Refusal, a refusal under the name of
// the call that makes it (fdh_glyphs.cpp, fdh_import.cpp, fdh_video_out.cpp), and place_batch, pass 2 of every batch (the glyph batches of
// fdh_glyphs.cpp, the image and video batches of fdh_import.cpp).  Host only: no kernel unit includes it.
#pragma once
#include <cstdint>
#include <exception>
#include <string>

#include "../../include/figdraw_hip.h"  // FDH_ERR_INVALID
#include "fdh_atlas.h"
#include "fdh_plain.h"  // Error

namespace fdh {

struct Refusal {
  const char* who;
  Error operator()(const std::string& what) const { return Error(FDH_ERR_INVALID, std::string(who) + ": " + what); }
};

// Pass 2 of a batch of glyphs, of images or of frames: every item through place(), in order; item(i, &key, &w, &h) names it, placed_at(i, entry)
// takes its place.  A placement that grows the atlas has dropped every entry before it: item i is then the first of the new atlas (*first).
// *placed: the items that got a place; the exception that ended the loop (FDH_ERR_ATLAS_FULL, or no memory for a larger atlas) is returned:
// the items before that one get their texels, as after single calls.
template <typename Item, typename PlacedAt>
std::exception_ptr place_batch(hipStream_t s, Atlas& atlas, int n, int (*out_rects)[4], Stored stored, Item item, PlacedAt placed_at, int* first, int* placed) {
  std::exception_ptr failed;
  int f = 0, p = 0;
  for (; p < n; p++) {
    const int before = atlas.size();
    try {
      int64_t key;
      int w, h;
      item(p, &key, &w, &h);
      placed_at(p, atlas.place(s, key, w, h, out_rects ? out_rects[p] : nullptr, stored));
    } catch (...) {
      failed = std::current_exception();
    }
    if (atlas.size() != before) f = p;
    if (failed) break;
  }
  *first = f; *placed = p;
  return failed;
}

}  // namespace fdh
