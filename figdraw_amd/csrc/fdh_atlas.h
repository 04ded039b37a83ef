// fdh_atlas.h -- the image atlas (fdh_atlas.cpp): the directory of entries, the skyline packer and the level chains in device memory: one
// member of Context.  The context quiesces its stream (a frame in flight may sample the atlas) and hands it over with every call; the
// atlas does not know the context.  Glyphs made on the device are GlyphMaker's (fdh_glyphs.h), which places them here.
#pragma once
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "fdh_memory.h"  // hipStream_t
#include "fdh_types.h"   // AtlasView, kMaxMips

namespace fdh {

// An atlas entry and, when its level-0 texels were seen on the host (fdh_put_image), the bounds of what is IN it: for eight
// levels t = 0, 16, .. 112 the box (entry-relative texels, x1 / y1 exclusive) of texels whose alpha, and whose largest colour
// channel, exceeds t.  A draw whose coverage is exactly 0 wherever the sampled value is <= t (a glyph image: alpha 0; an MSDF
// image: distance below threshold - 0.5 / screen range) shrinks its pixel bounds to the image of that box: the strips outside
// would blend with alpha 0, which leaves every texel as it is (Recorder::shrink_to_ink).
constexpr int kInkLevels = 8;
struct InkBox { int16_t x0, y0, x1, y1; };
struct AtlasEntry {
  int x, y, w, h;
  bool has_ink = false;
  InkBox ink_a[kInkLevels], ink_rgb[kInkLevels];
};

class Atlas {
 public:
  // ---- directory and packer: no device needed (a record-only context has both)
  void init(int size, bool device, hipStream_t s);  // a context's first atlas; `device`: the levels exist (else only the directory and the packer)
  const AtlasEntry* find(int64_t key) const {       // (the walk pool's threads call this while they record)
    auto it = entries_.find(key);
    return it == entries_.end() ? nullptr : &it->second;
  }
  bool has(int64_t key) const { return entries_.count(key) != 0; }
  void remove(int64_t key) { entries_.erase(key); epoch_++; }
  int size() const { return size_; }
  int n_levels() const { return n_levels_; }
  // moves with every put, update, remove and reset: cached draw records of image nodes carry atlas positions (RetainedRoot::atlas_epoch)
  uint64_t epoch() const { return epoch_; }
  int64_t packed_area() const;
  void reset(int minimum_size, hipStream_t s);
  // ---- what the kernels sample, and level 0 for fdh_debug_read_surface
  AtlasView view() const;
  const uint32_t* level0() const { return levels_[0]; }
  // ---- what a put from outside (GlyphMaker) needs: THE placement -- rect (growing as needed, which drops every entry), entry, epoch,
  // out_rect; whether the levels exist; a level's texels (valid until the next placement); and updateSubImage's level chain
  // (textures.nim:106-119): step(level, x, y, w, h) for the image minified `level` times, while width > 1 and height > 1
  AtlasEntry& place(hipStream_t s, int64_t key, int w, int h, int out_rect[4]);
  bool has_device() const { return device_; }
  uint32_t* level(int l) const { return levels_[l]; }
  template <typename Step> void each_level(int x, int y, int w, int h, Step step) const {
    for (int level = 0; w > 1 && h > 1 && level < n_levels_; level++, x /= 2, y /= 2, w = (w + 1) / 2, h = (h + 1) / 2) step(level, x, y, w, h);
  }
  // ---- texel work.  Every put validates and only then takes a place: one that throws before its texels are on their way leaves no
  // entry and no epoch bump behind.
  void put_image(hipStream_t s, int64_t key, int w, int h, const uint8_t* rgba, int out_rect[4]);
  void put_mips(hipStream_t s, int64_t key, int n, const int* ws, const int* hs, const uint8_t* const* premul_rgba, int out_rect[4]);
  void put_flippy(hipStream_t s, int64_t key, const uint8_t* data, size_t n, int out_rect[4]);
  void update_image(int64_t key, int w, int h, const uint8_t* rgba);
  void release() { release_levels(); }  // (the stream is idle)

 private:
  void alloc(int size, hipStream_t s);  // new levels first, then the old ones go and the empty atlas is committed
  void release_levels();
  void upload_rect(int level, int x, int y, int w, int h, const uint8_t* rgba);
  void put_levels(int x, int y, int w, int h, const uint8_t* rgba);

  bool device_ = false;
  int size_ = 0, initial_size_ = 0, margin_ = 4, n_levels_ = 0;
  uint32_t* levels_[kMaxMips] = {};
  std::vector<uint16_t> heights_;  // the skyline
  std::unordered_map<int64_t, AtlasEntry> entries_;
  uint64_t epoch_ = 1;
};

}  // namespace fdh
